"""Per-table embedding bag sizes without a GPU: the host layer on the CPU oracle -- which has no ragged gather, so a
mixed model gathers once per bag size -- the driver's flag, the HDF5 layout, the refusals, and the surface of include/ff_hip_bags.h."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import bags_helpers as BH
import dlrm_helpers as H

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
TESTS = os.path.dirname(os.path.abspath(__file__))


def test_mixed_model_matches_float64_numpy():
    """3 tables of bag sizes 1, 3, 2 through the FFModel API, 2 steps of plain SGD: predictions and every parameter against the float64
    restatement, at the bound of dlrm_helpers.check_against_golden."""
    m, h = BH.build_mixed_model(H.oracle_backend())
    recs = H.run_steps(m, h, 2)
    exp = BH.numpy_reference(h, 2)
    for step in range(2):
        assert recs[step].keys() == exp[step].keys()
        for k in recs[step]:
            np.testing.assert_allclose(recs[step][k], exp[step][k].reshape(recs[step][k].shape), rtol=1e-5, atol=1e-6, err_msg=f"step {step} {k}")
    assert m.counter("ragged_gather_launches") == 0           # the oracle has no ragged gather: one uniform launch per bag size
    assert m.counter("folded_tables") == 0
    m.close()


_DRIVER = ["-b", "16", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "50-7-300", "--arch-mlp-bot", "13-16-8", "--arch-mlp-top", "32-16-1",
           "--data-size", "64", "--epochs", "2"]


def _transcript(r):
    """What the driver said, without the lines that name the flag's spelling and without the wall-clock line."""
    keep = lambda l: not l.startswith(("[DLRM] EmbeddingBagSize", "[DLRM] embedding gather:", "ELAPSED TIME"))
    return [l for l in r.stdout.splitlines() if keep(l)], r.stderr


def test_list_of_equal_sizes_is_the_uniform_model():
    """--embedding-bag-sizes 2-2-2 == --embedding-bag-size 2: transcript and dumped results, bit for bit."""
    base = [EXE, "--backend", H.oracle_backend()] + _DRIVER
    a = subprocess.run(base + ["--embedding-bag-sizes", "2-2-2"], capture_output=True, text=True, timeout=120)
    b = subprocess.run(base + ["--embedding-bag-size", "2"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert "[DLRM] EmbeddingBagSizes(2-2-2)" in a.stdout and "[DLRM] embedding gather: one bag size" in a.stdout
    assert "[DLRM] EmbeddingBagSize(2)" in b.stdout and "EmbeddingBagSizes" not in b.stdout and "embedding gather" not in b.stdout
    assert _transcript(a) == _transcript(b)
    c = subprocess.run(base + ["--embedding-bag-sizes=2-2-2"], capture_output=True, text=True, timeout=120)
    assert c.returncode == 0 and _transcript(c) == _transcript(a)
    ta = BH.trajectory(H.oracle_backend(), _DRIVER + ["--embedding-bag-sizes", "2-2-2"], 3, trace=False)
    tb = BH.trajectory(H.oracle_backend(), _DRIVER + ["--embedding-bag-size", "2"], 3, trace=False)
    assert ta.keys() == tb.keys()
    for k in ta:
        np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)


def test_mixed_driver_says_how_it_gathers_and_exposes_the_sizes():
    r = subprocess.run([EXE, "--backend", H.oracle_backend()] + _DRIVER + ["--embedding-bag-sizes", "1-3-2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "[DLRM] EmbeddingBagSizes(1-3-2)" in r.stdout and "THROUGHPUT = " in r.stdout
    assert "[DLRM] embedding gather: per bag size, 3 launches (the kernel library has no ragged gather)" in r.stdout
    app = ffmodel.DLRM(["--backend", H.oracle_backend()] + _DRIVER + ["--embedding-bag-sizes", "1-3-2"])
    assert app.bag_sizes == [1, 3, 2]
    assert [app.sparse_input(t).dims[1] for t in range(3)] == [1, 3, 2]
    app.close()


def _mixed_hdf5(tmp_path, bags, rows=(50, 7, 300), n=100, seed=9):
    rng = np.random.default_rng(seed)
    cat = np.concatenate([rng.integers(0, r, (n, L)) for r, L in zip(rows, bags)], 1).astype(np.int32)
    raw = {"X_int": rng.integers(0, 1000, (n, 13)).astype(np.int32), "X_cat": cat, "y": rng.integers(0, 2, n).astype(np.int32)}
    npz, h5 = os.path.join(tmp_path, "mixed.npz"), os.path.join(tmp_path, "mixed.h5")
    np.savez(npz, **raw)
    spec = importlib.util.spec_from_file_location("preprocess_hdf", os.path.join(ROOT, "tools", "preprocess_hdf.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    mod.convert(npz, h5)
    return h5, cat.astype(np.int64)


def test_hdf5_with_a_column_block_per_table(tmp_path):
    """X_cat has sum(L_t) columns, table t's ids in columns [sum_{u<t} L_u, ... + L_t); a wrong column count is refused with the expected sum."""
    bags = (1, 3, 2)
    h5, cat = _mixed_hdf5(str(tmp_path), bags)
    app = ffmodel.DLRM(["--backend", H.oracle_backend()] + H.HDF5_ARGS + ["--dataset", h5, "--embedding-bag-sizes", "1-3-2"])
    assert app.num_samples == 96
    B = 16
    app.warmup()
    for step in range(7):
        app.model.sync()
        k, c0 = step % 6, 0
        for t, L in enumerate(bags):
            assert np.array_equal(app.sparse_input(t).get(np.int64).reshape(B, L), cat[k * B:(k + 1) * B, c0:c0 + L])
            c0 += L
        app.train_steps(1, trace=False)
    assert np.isfinite(app.model.perf_metrics().mse_loss)
    app.close()
    base = [EXE, "--backend", H.oracle_backend()] + H.HDF5_ARGS + ["--dataset", h5]
    r = subprocess.run(base + ["--embedding-bag-sizes", "1-3-3"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "X_cat's second dimension must equal the sum of the tables' bag sizes, 7 (it is 6)" in r.stderr
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "X_cat's second dimension must equal the sum of the tables' bag sizes, 3 (it is 6)" in r.stderr


@pytest.mark.parametrize("flags,message", [
    (["--embedding-bag-sizes", "1-3"], "--embedding-bag-sizes has 2 entries for 3 tables (--arch-embedding-size)"),
    (["--embedding-bag-sizes", "1-0-2"], "--embedding-bag-sizes: entry 1 is 0, a bag size must be >= 1 (--embedding-bag-size has the same rule)"),
    (["--embedding-bag-sizes", "1-3-2", "--embedding-bag-size", "2"], "--embedding-bag-sizes and --embedding-bag-size were both given"),
])
def test_flag_refusals(flags, message):
    r = subprocess.run([EXE, "--backend", H.oracle_backend()] + _DRIVER + flags, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]


_PLACEMENT = r"""
import os, sys
sys.path.insert(0, {tests!r})
import torch.distributed as dist
from dlrm_flexflow_amd.comm import TorchComm
import bags_helpers as BH, dlrm_helpers as H
rank, port = int(sys.argv[1]), int(sys.argv[2])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
comm = TorchComm(on_gpu=False)
BH.build_mixed_model(H.oracle_backend(), extra_argv=[{flag!r}, "6"], comm=comm.struct)
print("COMPILED")
"""


@pytest.mark.parametrize("case,flag,how", [(0, "--row-shard-rows", "row-sharded"), (1, "--column-shard-rows", "column-sharded"),
                                           (2, "--replicate-embedding-rows", "replicated")])
def test_sharded_and_replicated_placements_refuse_mixed_bags(case, flag, how):
    """Two gloo ranks: compile() names the flag to drop (the same flags with one bag size compile: the existing placement tests)."""
    H.oracle_backend()                                       # built once, before the ranks start
    port = 34400 + os.getpid() % 1000 + 1000 * case       # a port of its own per case
    procs = [subprocess.Popen([sys.executable, "-c", _PLACEMENT.format(tests=TESTS, flag=flag), str(r), str(port)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=120))
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate())
    for p, (out, err) in zip(procs, outs):
        assert p.returncode != 0 and "COMPILED" not in out, out
    err = outs[0][1] + outs[1][1]
    assert "different bag sizes (--embedding-bag-sizes) are supported table-wise only" in err, err[-2000:]
    assert f"is {how} here; drop {flag}" in err, err[-2000:]


def test_library_exports_the_bags_extension():
    """libffhip.so exports every symbol of include/ff_hip_bags.h with the header's ABI version (loadable without a GPU); the oracle lacks it."""
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)
    syms = capi.bags_header_symbols()
    assert set(syms) == set(capi._SIGS_BAGS) and "ffh_embedding_fwd_multi_bags" in syms and "ffh_embedding_fwd_multi_bags_bf16" in syms
    for s in syms:
        assert hasattr(lib, s), s
    lib.ffh_bags_abi_version.restype = ctypes.c_int
    assert lib.ffh_bags_abi_version() == capi.bags_header_abi_version() == 1
    assert set(syms).isdisjoint(capi.header_symbols())        # nothing added to ff_hip.h
    oracle = capi.FFHLib(H.oracle_backend())
    with pytest.raises(capi.FFHError, match="no bags extension"):
        capi.bags_api(oracle)
    oracle.close()


def test_kernel_arguments_fit():
    """The ragged gather's kernel-argument struct (64 tables, twin and image pointers, 16-bit bag sizes) stays inside the 4 KB of kernel arguments."""
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)
    lib.ffh_bags_kernarg_bytes.restype = ctypes.c_size_t
    n = lib.ffh_bags_kernarg_bytes()
    assert 64 * 40 < n <= 4096
