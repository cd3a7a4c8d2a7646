"""CPU tests of the shuffled data order (--data-randomize total; include/ffh_perm.h, include/ff_hip_data.h): the order against a numpy
restatement of the header's construction, the stripe rule, the symbol list against the libraries and the bindings, and the flags and
refusals of the driver with the CPU oracle as kernel library (no GPU is opened).  What the gather kernel and the model do with the order
is tests/test_gpu_shuffle.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import build, capi, ffmodel
import shuffle_helpers as SH

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "512", "--epochs", "1"]
SIZES = [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 4096, 4097, 65537]        # tiny n and n = 4^k + 1 (the longest walks) among them
SEEDS = [0, 0xD1CEDA7A5EED1234]
EPOCHS = [0, 1, 7]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def _oracle():
    import dlrm_helpers as H
    return H.oracle_backend()


def _driver(*extra):
    return subprocess.run([EXE, "--backend", _oracle(), *SMALL, *extra], capture_output=True, text=True, timeout=300)


# ---- 1. the order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_shuffle_index_equals_the_restatement_and_is_a_bijection(n):
    orders = {}
    for seed in SEEDS:
        for epoch in EPOCHS:
            got = ffmodel.shuffle_indices(seed, epoch, n)
            assert np.array_equal(got, SH.perm(seed, epoch, n)), (n, seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(n)), (n, seed, epoch)
            orders[seed, epoch] = got
    # the scalar binding is the same function
    for i in sorted({0, n // 2, n - 1}):
        assert ffmodel.shuffle_index(SEEDS[1], 7, i, n) == int(orders[SEEDS[1], 7][i])
    if n >= 16:
        keys = list(orders)
        for a in range(len(keys)):
            for b in range(a + 1, len(keys)):
                assert not np.array_equal(orders[keys[a]], orders[keys[b]]), (n, keys[a], keys[b])


def test_positions_outside_the_range_are_refused():
    with pytest.raises(ValueError):
        ffmodel.shuffle_index(0, 0, 5, 5)
    with pytest.raises(ValueError):
        ffmodel.shuffle_indices(0, 0, 5, first=3, count=3)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_stripe_rule_visits_every_training_sample_once(world):
    """B = 8, five training batches: over one epoch the ids of all ranks' rows are the 40 training samples once each (so nothing of a
    held-out tail behind them), and rank r's rows stay inside rank r's slots of the file's batches."""
    B, nb = 8, 5
    Bl = B // world
    for epoch in (0, 1):
        seen = []
        for k in range(nb):
            for r in range(world):
                for i in range(Bl):
                    p = ffmodel.shuffle_index(9, epoch, k * Bl + i, nb * Bl)
                    g = (p // Bl) * B + r * Bl + p % Bl
                    assert g % B // Bl == r
                    seen.append(g)
        assert sorted(seen) == list(range(nb * B))
        assert np.array_equal(np.array(seen).reshape(nb, world, Bl), SH.epoch_order(9, epoch, nb, B, world).reshape(nb, world, Bl))


# ---- 2. the header's list, the libraries, the bindings ------------------------------------------------------------------------------------
def test_data_header_list_declarations_and_prototypes_agree():
    syms = capi.data_header_symbols()
    assert syms and len(syms) == len(set(syms))
    assert set(syms) == set(capi._SIGS_DATA), set(syms) ^ set(capi._SIGS_DATA)
    body = open(capi.DATA_HEADER_PATH).read().split("#define FFH_DATA_API_LIST")[0]
    declared = set(re.findall(r"^int\s+(ffh_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == set(syms), declared ^ set(syms)
    # include/ff_hip.h: list and ABI version untouched by the extension
    assert not set(syms) & set(capi.header_symbols())
    assert set(capi.header_symbols()) == set(capi._SIGS)
    assert capi.header_abi_version() == 14
    assert capi.data_header_abi_version() == 1
    text = open(capi.DATA_HEADER_PATH).read()
    assert int(re.search(r"#define FFH_GATHER_MAX_SEGMENTS\s+(\d+)", text).group(1)) == capi.GATHER_MAX_SEGMENTS
    assert int(re.search(r"#define FFH_GATHER_LOCAL_ROWS\s+(\d+)", text).group(1)) == capi.GATHER_LOCAL_ROWS
    assert int(re.search(r"#define FFH_GATHER_GLOBAL_ROWS\s+(\d+)", text).group(1)) == capi.GATHER_GLOBAL_ROWS


def test_hip_library_exports_the_extension_and_the_oracle_does_not(oracle):
    exp = _exported(build.build_hip())
    assert set(capi.data_header_symbols()) <= exp
    assert not set(capi.data_header_symbols()) & _exported(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no data extension"):
        capi.data_api(oracle.lib())


def test_c_api_exports_the_order():
    assert {"flexflow_shuffle_index", "flexflow_shuffle_indices"} <= _exported(HOST_LIB)


# ---- 3. flags and refusals --------------------------------------------------------------------------------------------------------------
def test_total_is_refused_on_a_library_without_the_extension():
    for flags in (("--data-randomize", "total"), ("--data-randomize=total",)):
        r = _driver("--synthetic-labels", "logistic", *flags)
        assert r.returncode != 0
        assert "without the data extension" in r.stderr and "include/ff_hip_data.h" in r.stderr and "--data-randomize none" in r.stderr, r.stderr[-2000:]
        assert "THROUGHPUT" not in r.stdout


def test_total_is_refused_on_a_run_that_never_advances_its_batch():
    r = _driver("--data-randomize", "total")
    assert r.returncode != 0
    assert "--data-randomize total: this run never advances its batch" in r.stderr, r.stderr[-2000:]
    assert "--dataset" in r.stderr and "--synthetic-labels logistic" in r.stderr and "--data-randomize none" in r.stderr
    assert "THROUGHPUT" not in r.stdout


@pytest.mark.parametrize("value", ["epoch", "", "TOTAL"])
def test_unknown_value_is_refused(value):
    r = _driver(f"--data-randomize={value}")
    assert r.returncode != 0 and f"--data-randomize {value}: 'none' or 'total'" in r.stderr, r.stderr[-2000:]


def test_default_run_says_file_order_and_is_otherwise_unchanged():
    r = _driver()
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert [l for l in lines if "data order" in l] == ["[DLRM] data order: none (file order, the same every epoch)"]
    assert "THROUGHPUT" in r.stdout
    r2 = _driver("--data-randomize", "none")
    assert r2.returncode == 0, r2.stderr[-2000:]
    strip = lambda s: [l for l in s.splitlines() if "ELAPSED TIME" not in l]
    assert strip(r2.stdout) == strip(r.stdout)
    # the start-up lines of the driver, in order: the one new line sits behind the loss line and nothing else moved
    heads = [l.split(":")[0] for l in lines if l.startswith("[DLRM]")]
    assert heads[:8] == ["[DLRM] batchSize(64) workersPerNodes(0) numNodes(1)", "[DLRM] EmbeddingBagSize(1)", "[DLRM] Embedding Vocab Sizes",
                         "[DLRM] MLP Top", "[DLRM] MLP Bot", "[DLRM] loss", "[DLRM] data order", "[DLRM] Use random dataset..."], heads
