"""Mean pooling over variable-length embedding bags (include/ff_hip_pad_mean.h) without a GPU: the surface of the extension, the numpy
restatements, the workspace query, and the driver's --embedding-pooling on the CPU oracle -- which has no pad extension, so mean pooling runs
there only without --embedding-padding, on the existing AVG paths."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import dlrm_helpers as H

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
FLAG = "--embedding-pooling"
SMALL = ["-b", "16", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "50-7-300", "--arch-mlp-bot", "13-16-8", "--arch-mlp-top", "32-16-1",
         "--data-size", "64", "--epochs", "1", "--embedding-bag-size", "3"]


def _driver(*flags, small=SMALL):
    return subprocess.run([EXE, "--backend", H.oracle_backend(), *small, *flags], capture_output=True, text=True, timeout=120)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def _lib():
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)      # loads without a GPU
    for name, (res, args) in capi._SIGS_PAD_MEAN.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


# ---- the extension's surface -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_pad_mean_extension(oracle):
    from dlrm_flexflow_amd import build
    syms = capi.pad_mean_header_symbols()
    assert set(syms) == set(capi._SIGS_PAD_MEAN) and len(syms) == len(set(syms)) == 6
    body = open(capi.PAD_MEAN_HEADER_PATH).read().split("#define FFH_PAD_MEAN_API_LIST")[0]
    assert set(re.findall(r"\b(ffh_[a-z0-9_]+)\s*\(", body)) == set(syms)      # every declared function is in the list
    exp = _exported(build.build_hip())
    assert not [s for s in syms if s not in exp]
    assert _lib().ffh_pad_mean_abi_version() == capi.pad_mean_header_abi_version() == 1
    for other in (capi.header_symbols(), capi.bags_header_symbols(), capi.bags_update_header_symbols(), capi.bags_sort_header_symbols(), capi.pad_header_symbols()):
        assert set(syms).isdisjoint(other)
    assert len(capi.pad_header_symbols()) == 7 and capi.pad_header_abi_version() == 1      # include/ff_hip_pad.h keeps its list and its version
    assert not set(syms) & _exported(oracle.ORACLE_LIB)
    o = capi.FFHLib(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no pad-mean extension"):
        capi.pad_mean_api(o)
    o.close()


def test_kernel_arguments_still_fit():
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name in ("ffh_bags_kernarg_bytes", "ffh_bags_update_kernarg_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
        assert 0 < getattr(lib, name)() <= 4096
    # the count pointer of the mean forms lies in the update's argument structs
    assert lib.ffh_bags_update_kernarg_bytes() >= 64 * (40 + 8 + 8 + 2) + 8


def test_bindings():
    s = capi._SIGS_PAD_MEAN
    assert s["ffh_embedding_fwd_multi_bags_pad_mean"] == capi._SIGS_PAD["ffh_embedding_fwd_multi_bags_pad"]
    assert s["ffh_embedding_fwd_multi_bags_pad_mean_bf16"] == capi._SIGS_PAD["ffh_embedding_fwd_multi_bags_pad_bf16"]
    for name in ("fused", "apply"):
        assert s[f"ffh_embedding_bwd_{name}_multi_bags_pad_mean"] == capi._SIGS_PAD[f"ffh_embedding_bwd_{name}_multi_bags_pad"]
    assert s["ffh_embedding_bwd_bags_pad_mean_workspace_bytes"] == capi._SIGS_BAGS_UPDATE["ffh_embedding_bwd_bags_workspace_bytes"]
    for m in ("fwd", "fwd_rc", "fused", "fused_rc", "apply", "apply_rc", "workspace_bytes"):
        assert callable(getattr(capi.PadMeanApi, m))
    assert not hasattr(capi.PadMeanApi, "sort")      # the pad sort serves either apply
    host = _exported(HOST_LIB)
    hdr = open(os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel_c.h")).read()
    assert "flexflow_dlrm_get_embedding_pooling" in host and "flexflow_dlrm_get_embedding_pooling" in hdr
    assert hasattr(ffmodel.lib(), "flexflow_dlrm_get_embedding_pooling") and isinstance(ffmodel.DLRM.embedding_pooling, property)


# ---- the workspace query -------------------------------------------------------------------------------------------------------------------
def _bytes(lib, name, bags, D, batch):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    arr = (ctypes.c_int * max(len(bags), 1))(*bags) if bags is not None else None
    return fn(arr, len(bags) if bags is not None else 1, D, batch)


@pytest.mark.parametrize("bags,D,batch", [((1, 7, 32), 16, 64), ((7, 1, 100), 6, 500), ((1,), 4, 1), ((3,) * 26, 128, 8192), ((65535,), 4, 3)])
def test_workspace_is_the_old_layout_plus_a_count_per_bag(bags, D, batch):
    lib = _lib()
    old = _bytes(lib, "ffh_embedding_bwd_bags_workspace_bytes", bags, D, batch)
    new = _bytes(lib, "ffh_embedding_bwd_bags_pad_mean_workspace_bytes", bags, D, batch)
    assert old > 0 and new >= old + 2 * len(bags) * batch      # 16 bits per (table, bag), behind the layout
    assert new <= old + 2 * len(bags) * batch + 32             # ... and two roundings to 16 bytes at the most


def test_workspace_query_returns_zero_on_bad_arguments():
    lib = _lib()
    q = lambda *a: _bytes(lib, "ffh_embedding_bwd_bags_pad_mean_workspace_bytes", *a)
    assert q((1, 7), 16, 64) > 0
    assert q(None, 16, 64) == 0 and q((), 16, 64) == 0 and q((1, 0), 16, 64) == 0 and q((1, 7), 0, 64) == 0 and q((1, 7), 16, 0) == 0
    assert q((1, 65536), 16, 64) == 0 and q((1, 7), 16, 2**31) == 0 and q((1,) * 65, 16, 64) == 0


# ---- the numpy restatements ----------------------------------------------------------------------------------------------------------------
def test_padded_bag_counts_and_the_mean_reference_against_values_written_out_by_hand():
    W = np.array([[1, 2], [10, 20], [-0.0, -0.0], [0.5, 0.25]], np.float32)
    idx = np.array([[0, 1, 3], [-1, 1, -1], [-1, -1, -1], [2, -1, -1], [3, 3, -1], [2, 2, 2]])
    cnt = ffmodel.padded_bag_counts(idx)
    assert cnt.dtype == np.int64 and cnt.tolist() == [3, 1, 0, 1, 2, 3]
    third = np.float32(1) / np.float32(3)
    want = np.array([[np.float32(11.5) * third, np.float32(22.25) * third], [10, 20], [0, 0], [0, 0], [0.5, 0.25], [0, 0]], np.float32)
    out = ffmodel.padded_bag_reference(W, idx, mean=True)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out.view(np.uint32), want.view(np.uint32))
    for b in (2, 3, 5):      # only pads; (+0) + (-0); three times the -0 row: the bit pattern of +0
        assert not out[b].view(np.uint32).any()
    # the keyword defaults to the sum of before
    np.testing.assert_array_equal(ffmodel.padded_bag_reference(W, idx), np.array([[11.5, 22.25], [10, 20], [0, 0], [0, 0], [1, 0.5], [0, 0]], np.float32))
    np.testing.assert_array_equal(ffmodel.padded_bag_reference(W, idx).view(np.uint32), ffmodel.padded_bag_reference(W, idx, mean=False).view(np.uint32))
    # one reciprocal and one multiply, not a division: 1 / 3 * 0.3 and 0.3 / 3 differ in float32 for some values
    rng = np.random.default_rng(0)
    W = rng.standard_normal((9, 5)).astype(np.float32)
    idx = rng.integers(-1, 9, (200, 7))
    s = ffmodel.padded_bag_reference(W, idx)
    inv = np.float32(1) / np.maximum(ffmodel.padded_bag_counts(idx), 1).astype(np.float32)
    np.testing.assert_array_equal(ffmodel.padded_bag_reference(W, idx, mean=True).view(np.uint32), (s * inv[:, None]).view(np.uint32))
    assert set(ffmodel.padded_bag_counts(idx).tolist()) >= {4, 5, 6, 7}


# ---- the driver's flag on the oracle ---------------------------------------------------------------------------------------------------------
def _pick(out):
    return [l for l in out.splitlines() if l.startswith("[DLRM]") or "loss" in l]


def _metrics(r):
    """the run's loss lines: the driver prints its metrics (the mean squared error among them) on stderr"""
    return [l for l in r.stderr.splitlines() if l.startswith("[Metrics]")]


def test_sum_leaves_the_run_as_it_was_and_mean_moves_the_loss():
    base = _driver()
    assert base.returncode == 0 and "embedding pooling" not in base.stdout, base.stderr[-2000:]
    for spelling in ((FLAG, "sum"), (FLAG + "=sum",)):
        r = _driver(*spelling)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "[DLRM] embedding pooling: sum" in r.stdout
        assert [l for l in _pick(r.stdout) if "embedding pooling" not in l] == _pick(base.stdout)
        assert _metrics(r) == _metrics(base)
    outs = []
    for spelling in ((FLAG, "mean"), (FLAG + "=mean",)):
        r = _driver(*spelling)
        assert r.returncode == 0 and "THROUGHPUT" in r.stdout, r.stderr[-2000:]
        assert "[DLRM] embedding pooling: mean (over L_t slots)" in r.stdout
        outs.append(_pick(r.stdout))
    assert outs[0] == outs[1]
    assert _metrics(base) and _metrics(r) != _metrics(base), "mean pooling left the loss where the sum had it"


@pytest.mark.parametrize("spelling", [(FLAG, "max"), (FLAG + "=avg",), (FLAG + "=",)], ids=["max", "avg", "empty"])
def test_another_value_is_refused_naming_the_flag(spelling):
    r = _driver(*spelling)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    assert FLAG in r.stderr and "'sum' or 'mean'" in r.stderr, r.stderr[-2000:]


def test_mean_over_padded_bags_is_refused_on_the_oracle():
    r = _driver("--embedding-padding", FLAG, "mean")
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    for w in ("--embedding-padding", "AGGR_MODE_AVG", "drop --embedding-padding", "include/ff_hip_pad_mean.h"):
        assert w in r.stderr, (w, r.stderr[-2000:])
    assert "extension" not in r.stderr
