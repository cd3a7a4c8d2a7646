"""Variable-length embedding bags (include/ff_hip_pad.h) without a GPU: the surface of the extension, the numpy restatements,
the flags, and every refusal of compile() on the CPU oracle -- which has no pad extension, so no padded model runs there at all."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import dlrm_helpers as H

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
LAUNCHER = os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py")
FLAG = "--embedding-padding"
SMALL = ["-b", "16", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "50-7-300", "--arch-mlp-bot", "13-16-8", "--arch-mlp-top", "32-16-1",
         "--data-size", "64", "--epochs", "1"]


def _driver(*flags, small=SMALL):
    return subprocess.run([EXE, "--backend", H.oracle_backend(), *small, *flags], capture_output=True, text=True, timeout=120)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


# ---- the extension's surface -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_pad_extension(oracle):
    from dlrm_flexflow_amd import build
    syms = capi.pad_header_symbols()
    assert set(syms) == set(capi._SIGS_PAD) and len(syms) == len(set(syms)) == 7
    body = open(capi.PAD_HEADER_PATH).read().split("#define FFH_PAD_API_LIST")[0]
    assert set(re.findall(r"\b(ffh_[a-z0-9_]+)\s*\(", body)) - {"ffh_u24", "ffh_hash"} == set(syms)      # every declared function is in the list
    exp = _exported(build.build_hip())
    assert not [s for s in syms if s not in exp]
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)                                          # loads without a GPU
    lib.ffh_pad_abi_version.restype = ctypes.c_int
    assert lib.ffh_pad_abi_version() == capi.pad_header_abi_version() == 1
    assert capi.EMB_PAD_ID == -1 and re.search(r"#define FFH_EMB_PAD_ID \(-1\)", open(capi.PAD_HEADER_PATH).read())
    for other in (capi.header_symbols(), capi.bags_header_symbols(), capi.bags_update_header_symbols(), capi.bags_sort_header_symbols()):
        assert set(syms).isdisjoint(other)
    assert len(capi.bags_header_symbols()) == 4 and len(capi.bags_update_header_symbols()) == 4 and len(capi.bags_sort_header_symbols()) == 3
    assert not set(syms) & _exported(oracle.ORACLE_LIB)
    o = capi.FFHLib(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no pad extension"):
        capi.pad_api(o)
    o.close()


def test_kernel_arguments_still_fit():
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name in ("ffh_bags_kernarg_bytes", "ffh_bags_update_kernarg_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
        assert 0 < getattr(lib, name)() <= 4096


def test_bindings():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    s = capi._SIGS_PAD
    assert s["ffh_embedding_fwd_multi_bags_pad"] == capi._SIGS_BAGS["ffh_embedding_fwd_multi_bags"]
    assert s["ffh_embedding_fwd_multi_bags_pad_bf16"] == capi._SIGS_BAGS["ffh_embedding_fwd_multi_bags_bf16"]
    for name in ("fused", "sort", "apply"):
        assert s[f"ffh_embedding_bwd_{name}_multi_bags_pad"] == capi._SIGS_BAGS_UPDATE["ffh_embedding_bwd_fused_multi_bags"]
    assert s["ffh_pad_mask_indices"] == (I, [P, P, L, ctypes.c_uint64, L, ctypes.c_float, P])
    host = _exported(HOST_LIB)
    hdr = open(os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel_c.h")).read()
    for name in ("flexflow_config_set_embedding_padding", "flexflow_dlrm_get_bag_fill"):
        assert name in host and name in hdr and hasattr(ffmodel.lib(), name)
    c = ffmodel.FFConfig(argv=["-b", "8"], backend=H.oracle_backend())
    assert c.set(embedding_padding=True) is c and c.set(embedding_padding=False) is c


# ---- the numpy restatements ----------------------------------------------------------------------------------------------------------------
def _mix64(z):
    """ffh_mix64 of include/ffh_rng.h in Python integers"""
    M = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_pad_mask_reference_against_values_computed_by_hand():
    """ffh_u24(ffh_hash(seed, first + i)) < fill, the hash in exact integer arithmetic: u24 = (h >> 40) / 2^24."""
    for seed, first, n in ((1, 0, 64), (2**63 + 5, 1000, 64), (7, 2**40, 16)):
        u = [(_mix64((_mix64(seed) + first + i) & ((1 << 64) - 1)) >> 40) / 16777216.0 for i in range(n)]
        for fill in (0.5, 0.25, 0.9):
            assert ffmodel.pad_mask_reference(seed, first, n, fill).tolist() == [v < float(np.float32(fill)) for v in u], (seed, first, fill)
    # written out: the 24-bit draws of seed 1, elements 0 .. 5 (splitmix64 by hand), against 0.5 = 8388608 / 2^24
    draws = [6177195, 8836861, 12376539, 11617309, 14611508, 7804634]
    assert [(_mix64((_mix64(1) + i) & ((1 << 64) - 1)) >> 40) for i in range(6)] == draws
    assert ffmodel.pad_mask_reference(1, 0, 6, 0.5).tolist() == [d < 8388608 for d in draws] == [True, False, False, False, False, True]
    assert ffmodel.pad_mask_reference(3, 0, 1000, 1.0).all() and not ffmodel.pad_mask_reference(3, 0, 1000, 0.0).any()
    keep = ffmodel.pad_mask_reference(3, 0, 100000, 0.5)
    assert abs(keep.mean() - 0.5) < 0.01
    np.testing.assert_array_equal(ffmodel.pad_mask_reference(3, 777, 500, 0.5), keep[777:1277])      # a continuation of the stream


def test_padded_bag_reference():
    W = np.array([[1, 2], [10, 20], [-0.0, -0.0], [0.5, 0.25]], np.float32)
    idx = np.array([[0, 1, 3], [-1, 1, -1], [-1, -1, -1], [2, -1, -1], [3, 3, -1]])
    out = ffmodel.padded_bag_reference(W, idx)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, np.array([[11.5, 22.25], [10, 20], [0, 0], [0, 0], [1, 0.5]], np.float32))
    assert not out[2].view(np.uint32).any() and not out[3].view(np.uint32).any()      # only pads, and (+0) + (-0): the bit pattern of +0
    rng = np.random.default_rng(0)
    W = rng.standard_normal((9, 5)).astype(np.float32)
    idx = rng.integers(-1, 9, (40, 6))
    ext = np.concatenate([W, np.zeros((1, 5), np.float32)])      # the zero-row reference in numpy
    acc = np.zeros((40, 5), np.float32)
    for j in range(6):
        acc = acc + ext[np.where(idx[:, j] < 0, 9, idx[:, j])]
    np.testing.assert_array_equal(ffmodel.padded_bag_reference(W, idx).view(np.uint32), acc.view(np.uint32))


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spelling", [(FLAG,), (FLAG + "=1",)], ids=["switch", "equals-one"])
def test_the_oracle_backend_is_refused_naming_the_backend(spelling):
    r = _driver(*spelling)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    for w in (FLAG, "without the pad extension", "include/ff_hip_pad.h", "--backend"):
        assert w in r.stderr, (w, r.stderr[-2000:])


def test_flag_off_spellings_leave_the_run_as_it_was():
    base, off = _driver(), _driver(FLAG + "=0")
    assert base.returncode == 0 and off.returncode == 0, off.stderr[-2000:]
    pick = lambda out: [l for l in out.splitlines() if l.startswith("[DLRM]") or "loss" in l]
    assert pick(base.stdout) == pick(off.stdout) and "embedding padding" not in base.stdout


@pytest.mark.parametrize("value", ["0", "-0.5", "1.5", "nan"])
def test_bag_fill_outside_its_range_is_refused(value):
    for spelling in (("--synthetic-bag-fill", value), ("--synthetic-bag-fill=" + value,)):
        r = _driver(FLAG, *spelling)
        assert r.returncode != 0 and "--synthetic-bag-fill" in r.stderr and "must be in (0, 1]" in r.stderr, r.stderr[-2000:]


def test_bag_fill_without_the_flag_is_refused():
    for spelling in (("--synthetic-bag-fill", "0.5"), ("--synthetic-bag-fill=1",)):
        r = _driver(*spelling)
        assert r.returncode != 0 and "add --embedding-padding" in r.stderr and "extension" not in r.stderr, r.stderr[-2000:]


# ---- the refusals of compile(): each names the flag to drop, and comes before the library check ------------------------------------------------
@pytest.mark.parametrize("extra,words", [
    (["--dense-embedding-update"], ["--dense-embedding-update"]),
    (["--no-ragged-gather"], ["--no-ragged-gather"]),
    (["--no-ragged-update"], ["--no-ragged-update"]),
    (["--eval-batches", "2", "--eval-embedding-dtype", "int8"], ["--eval-embedding-dtype int8", "no pad form"]),
], ids=["dense-update", "no-ragged-gather", "no-ragged-update", "int8-evaluation"])
def test_compile_refuses_what_the_pad_kernels_do_not_cover(extra, words):
    r = _driver(FLAG, *extra)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    for w in words + ["drop " + FLAG]:
        assert w in r.stderr, (w, r.stderr[-2000:])
    assert "extension" not in r.stderr


def test_mean_pooling_is_refused():
    c = ffmodel.FFConfig(argv=["-b", "8"], backend=H.oracle_backend())
    c.set(embedding_padding=True)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dlrm_flexflow_amd import capi, ffmodel\n"
            "c = ffmodel.FFConfig(argv=['-b', '8'], backend=%r); c.set(embedding_padding=True)\n"
            "m = ffmodel.FFModel(c); s = m.create_tensor([8, 2], ffmodel.DT_INT64)\n"
            "z = m.dense(m.embedding(s, 10, 4, capi.AGGR_MODE_AVG), 1); m.set_sgd_optimizer(lr=0.1); m.compile()\n" % (ROOT, H.oracle_backend()))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    for w in (FLAG, "AGGR_MODE_AVG", "drop " + FLAG):
        assert w in r.stderr, (w, r.stderr[-2000:])
    assert "extension" not in r.stderr


def test_sharded_and_replicated_tables_are_refused_in_a_two_rank_job():
    """--row-shard-rows, --column-shard-rows and --replicate-embedding-rows place tables that way only with more than one rank: two driver ranks on
    the oracle (gloo)."""
    for flag, value, word in (("--column-shard-rows", "150", "is column-sharded"), ("--replicate-embedding-rows", "60", "is replicated"),
                              ("--row-shard-rows", "150", "is row-sharded")):
        r = subprocess.run([sys.executable, LAUNCHER, "-ll:gpu", "2", "--backend", H.oracle_backend(), *SMALL, FLAG, flag, value],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
        assert word in r.stderr and flag in r.stderr and "drop " + FLAG in r.stderr, (flag, r.stderr[-2000:])
        assert "extension" not in r.stderr
