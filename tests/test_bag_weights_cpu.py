"""Per-sample weights on embedding bags (include/ffh_bag_weights.h) without a GPU: the surface of the extension, the numpy restatement, and the
driver's --embedding-per-sample-weights on the CPU oracle -- which lacks the extension, so every weighted run ends in a refusal of compile()."""
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

EXT = capi.EXTENSIONS["bag_weights"]
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
LAUNCHER = os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py")
FLAG = "--embedding-per-sample-weights"
SMALL = ["-b", "16", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "50-7-300", "--arch-mlp-bot", "13-16-8", "--arch-mlp-top", "32-16-1",
         "--data-size", "64", "--epochs", "1"]


def _driver(*flags, ranks=1):
    cmd = [EXE] if ranks == 1 else [sys.executable, LAUNCHER, "-ll:gpu", str(ranks)]
    return subprocess.run(cmd + ["--backend", H.oracle_backend(), *SMALL, *flags], capture_output=True, text=True, timeout=300, cwd=ROOT)


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_library_exports_the_extension_and_the_oracle_does_not(oracle):
    from dlrm_flexflow_amd import build
    syms = EXT.header_symbols()
    assert set(syms) == set(capi._SIGS_BAG_WEIGHTS) and len(syms) == len(set(syms)) == 5
    body = open(EXT.header_path).read().split("#define FFH_BAG_WEIGHTS_API_LIST")[0]
    assert set(re.findall(r"\b(ffh_[a-z0-9_]+)\s*\(", body)) == set(syms)      # every declared function is in the list
    assert not [s for s in syms if s not in _exported(build.build_hip())]
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)               # loads without a GPU
    assert lib.ffh_bag_weights_abi_version() == EXT.header_abi_version() == 1
    assert len(capi.pad_header_symbols()) == 7 and len(capi.pad_mean_header_symbols()) == 6      # the pad headers keep their lists
    assert not set(syms) & _exported(oracle.ORACLE_LIB)
    assert not hasattr(capi, "BAG_WEIGHTS_HEADER_PATH")
    o = capi.FFHLib(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no bag-weights extension.*include/ffh_bag_weights.h"):
        capi.bag_weights_api(o)
    o.close()


def test_weighted_bag_reference_equals_a_triple_loop():
    rng = np.random.default_rng(5)
    W = rng.standard_normal((9, 5)).astype(np.float32)
    idx = rng.integers(-1, 9, (40, 7))
    idx[3] = -1
    w = rng.standard_normal(idx.shape).astype(np.float32)
    w[idx < 0] = np.nan                                   # a pad's weight is never looked at
    w[0, idx[0] >= 0] = [0.0, -0.0, -1.5, 1.0, 2.0, 3.0, 4.0][:int((idx[0] >= 0).sum())]
    want = np.zeros((40, 5), np.float32)
    for b in range(40):
        for d in range(5):
            acc = np.float32(0)
            for j in range(7):
                if idx[b, j] >= 0:
                    acc = np.float32(acc + np.float32(w[b, j] * W[idx[b, j], d]))
            want[b, d] = acc
    got = ffmodel.weighted_bag_reference(W, idx, w)
    assert got.dtype == np.float32 and not got[3].view(np.uint32).any()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(ffmodel.weighted_bag_reference(W, idx, np.ones(idx.shape, np.float32)).view(np.uint32),
                                  ffmodel.padded_bag_reference(W, idx).view(np.uint32))


# ---- the driver's flag on the oracle: every refusal of compile() names the flag to drop ------------------------------------------------------
@pytest.mark.parametrize("extra,ranks,names", [
    ([FLAG + "=1"], 1, ["include/ffh_bag_weights.h", "bag-weights extension", "--backend"]),
    ([FLAG, "--embedding-pooling", "mean"], 1, ["AGGR_MODE_AVG", "drop --embedding-pooling mean"]),
    ([FLAG, "--dense-embedding-update"], 1, ["drop --dense-embedding-update"]),
    ([FLAG, "--no-ragged-gather"], 1, ["drop --no-ragged-gather"]),
    ([FLAG, "--no-ragged-update"], 1, ["drop --no-ragged-update"]),
    ([FLAG, "--eval-batches", "2", "--eval-embedding-dtype", "int8"], 1, ["drop --eval-embedding-dtype int8"]),
    ([FLAG, "--dataset", "criteo.h5"], 1, ["drop --dataset", "no weight column"]),
    ([FLAG, "--row-shard-rows", "150"], 2, ["is row-sharded", "drop --row-shard-rows"]),
    ([FLAG, "--column-shard-rows", "150"], 2, ["is column-sharded", "drop --column-shard-rows"]),
    ([FLAG, "--replicate-embedding-rows", "60"], 2, ["is replicated", "drop --replicate-embedding-rows"]),
], ids=["library", "avg", "dense-update", "no-ragged-gather", "no-ragged-update", "int8", "hdf5", "row-sharded", "column-sharded", "replicated"])
def test_compile_refuses_what_the_weighted_forms_do_not_cover(extra, ranks, names):
    """(Sharded and replicated placements exist only with more than one rank: two driver ranks on the oracle, over gloo.)"""
    r = _driver(*extra, ranks=ranks)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout, r.stdout[-1000:]
    for n in names + ["per-sample weights", FLAG]:
        assert n in r.stderr, (n, r.stderr[-2000:])
    assert ("extension" in r.stderr) == (names[0] == "include/ffh_bag_weights.h")      # the library check comes last


def test_flag_off_leaves_the_run_as_it_was():
    base, off = _driver(), _driver(FLAG + "=0")
    assert base.returncode == 0 and off.returncode == 0, off.stderr[-2000:]
    pick = lambda out: [l for l in out.splitlines() if l.startswith("[DLRM]") or "loss" in l]
    assert pick(base.stdout) == pick(off.stdout) and "embedding weights" not in base.stdout
