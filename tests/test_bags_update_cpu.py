"""The ragged table update (include/ff_hip_bags_update.h) without a GPU: the surface of the extension, its host arithmetic,
and the host layer on the CPU oracle -- which has no ragged update, so a mixed model updates once per bag size."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import bags_helpers as BH
import dlrm_helpers as H

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
_DRIVER = ["-b", "16", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "50-7-300", "--arch-mlp-bot", "13-16-8", "--arch-mlp-top", "32-16-1",
           "--data-size", "64", "--epochs", "2"]


def _lib():
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in capi._SIGS_BAGS_UPDATE.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    lib.ffh_embedding_bwd_workspace_bytes.restype, lib.ffh_embedding_bwd_workspace_bytes.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3 + [ctypes.c_int64]
    return lib


def _bytes(lib, bags, D, batch):
    return lib.ffh_embedding_bwd_bags_workspace_bytes(capi.BagsApi.in_dims(bags), len(bags), D, batch)


def test_library_exports_the_bags_update_extension():
    """libffhip.so exports every symbol of include/ff_hip_bags_update.h with the header's ABI version (loadable without a GPU); the lists of
    ff_hip.h and ff_hip_bags.h are untouched; the oracle lacks the extension."""
    lib = _lib()
    syms = capi.bags_update_header_symbols()
    assert set(syms) == set(capi._SIGS_BAGS_UPDATE) and "ffh_embedding_bwd_fused_multi_bags" in syms and len(syms) == 4
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.ffh_bags_update_abi_version() == capi.bags_update_header_abi_version() == 1
    assert set(syms).isdisjoint(capi.header_symbols()) and set(syms).isdisjoint(capi.bags_header_symbols())
    assert capi.bags_header_abi_version() == 1 and len(capi.bags_header_symbols()) == 4      # ff_hip_bags.h keeps its list
    oracle = capi.FFHLib(H.oracle_backend())
    for s in syms:
        assert not hasattr(oracle.lib, s), s
    with pytest.raises(capi.FFHError, match="no bags-update extension"):
        capi.bags_update_api(oracle)
    oracle.close()


def test_kernel_arguments_fit():
    """64 table descriptors, state pointers and 16-bit bag sizes: the largest argument struct of the ragged kernels stays inside 4 KB."""
    n = _lib().ffh_bags_update_kernarg_bytes()
    assert 64 * (40 + 8 + 8 + 2) < n <= 4096


def test_descriptor_layout():
    """struct ffh_bags_update as the header declares it (LP64): four pointers, two ints, int64, int, float, three pointers."""
    assert ctypes.sizeof(capi.BagsUpdate) == 80
    assert [getattr(capi.BagsUpdate, f).offset for f in ("ntables", "out_dim", "batch", "aggr", "lr", "opt", "lr_block")] == [32, 36, 40, 48, 52, 56, 72]


@pytest.mark.parametrize("nt,L,D,batch", [(3, 7, 16, 500), (1, 1, 8, 64), (26, 1, 128, 8192), (5, 100, 6, 6000)])
def test_workspace_of_equal_bags_is_the_uniform_workspace(nt, L, D, batch):
    lib = _lib()
    assert abs(_bytes(lib, [L] * nt, D, batch) - lib.ffh_embedding_bwd_workspace_bytes(nt, L, D, batch)) <= 256


def test_workspace_grows_with_the_lookups_not_with_the_largest_bag():
    lib = _lib()
    D, batch = 16, 500
    mixed, uniform = _bytes(lib, [1, 100, 1], D, batch), lib.ffh_embedding_bwd_workspace_bytes(3, 100, D, batch)
    one = lib.ffh_embedding_bwd_workspace_bytes(1, 100, D, batch)
    assert mixed < 0.5 * uniform, (mixed, uniform)
    assert one <= mixed <= one + 2 * lib.ffh_embedding_bwd_workspace_bytes(1, 1, D, batch) + 16 * 256      # the heavy table's share and two light ones
    # ... and linearly in the lookups: every table's share again
    assert abs(_bytes(lib, [1, 100, 1, 1, 100, 1], D, batch) - 2 * mixed) <= 0.02 * mixed
    # the order of the tables does not matter to the size
    assert _bytes(lib, [100, 1, 1], D, batch) == mixed == _bytes(lib, [1, 1, 100], D, batch)


# Workspace bytes as commit 8ec5655 ("Update tables of mixed bag sizes in one ragged sort-and-apply call") answers them, before the two layouts
# were given one layout function and one set of tile choices.  Callers size their buffers once and keep them: the sizes do not move.
_UNIFORM_BYTES = [      # ((nt, L, D, batch), bytes)
    ((1, 1, 8, 64), 6656), ((3, 7, 16, 500), 310528), ((26, 1, 128, 8192), 12304896), ((5, 100, 6, 6000), 57210880),
    ((26, 1, 128, 32768), 43946752),
    ((1, 1, 4, 2048), 55296), ((1, 1, 4, 2049), 58368),      # the two sides of the small route's 2048-lookup limit
    ((1, 1, 16, 300000), 6497280),                           # at most 32 sort tiles per table
    ((64, 1, 4, 1), 270080),
]
_MLPERF_BAGS = [3, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 100, 27, 10, 3, 1, 1]      # tools/bags_bench.py
_RAGGED_BYTES = [       # (bag sizes, D, batch, bytes)
    ([1, 100, 1], 128, 8192, 42219776), (_MLPERF_BAGS, 128, 8192, 88619008), ([7] * 3, 128, 8192, 8697600), ([1, 2], 3, 5, 10240),
]


def test_workspace_sizes_are_pinned():
    lib = _lib()
    assert [lib.ffh_embedding_bwd_workspace_bytes(*shape) for shape, _ in _UNIFORM_BYTES] == [n for _, n in _UNIFORM_BYTES]
    assert [_bytes(lib, bags, D, batch) for bags, D, batch, _ in _RAGGED_BYTES] == [n for _, _, _, n in _RAGGED_BYTES]


def test_workspace_of_bad_arguments_is_zero():
    lib = _lib()
    assert _bytes(lib, [1, 0, 3], 8, 64) == 0 and _bytes(lib, [1, capi.BAGS_MAX_IN_DIM + 1], 8, 64) == 0
    assert _bytes(lib, [1, 7], 8, 2**31 // 7 + 1) == 0 and _bytes(lib, [1] * 65, 8, 64) == 0
    assert lib.ffh_embedding_bwd_bags_workspace_bytes(None, 3, 8, 64) == 0 and _bytes(lib, [1, 2], 0, 64) == 0


def test_driver_on_the_oracle_updates_per_bag_size_and_trains():
    for flag in ([], ["--ragged-update"], ["--no-ragged-update"]):
        r = subprocess.run([EXE, "--backend", H.oracle_backend()] + _DRIVER + ["--embedding-bag-sizes", "1-3-2"] + flag, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "[DLRM] embedding update: per bag size, 3 calls per step (the kernel library has no ragged update)" in r.stdout, r.stdout
        assert "[DLRM] embedding gather: per bag size, 3 launches (the kernel library has no ragged gather)" in r.stdout and "THROUGHPUT = " in r.stdout
    # one bag size: no such line, whatever the flag
    r = subprocess.run([EXE, "--backend", H.oracle_backend()] + _DRIVER + ["--embedding-bag-sizes", "2-2-2", "--ragged-update"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "embedding update:" not in r.stdout


def test_the_later_of_the_two_flags_wins():
    """--ragged-update and --no-ragged-update together: the later one holds, as with --early-sort / --no-early-sort (which of them held shows
    on a library that has the extension: tests/test_gpu_bags_update_model.py).  Here: both orders are accepted, the oracle runs no ragged call under
    either, and both train to the same bits."""
    args = _DRIVER + ["--embedding-bag-sizes", "1-3-2"]
    a, ca = BH.trajectory(H.oracle_backend(), args + ["--ragged-update", "--no-ragged-update"], 2, trace=False, counters=("ragged_update_launches",))
    b, cb = BH.trajectory(H.oracle_backend(), args + ["--no-ragged-update", "--ragged-update"], 2, trace=False, counters=("ragged_update_launches",))
    assert ca == cb == {"ragged_update_launches": 0}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_config_setter_and_model_query():
    """FFConfig.set(ragged_update=...) exists and chains like the other settings."""
    c = ffmodel.FFConfig(argv=["-b", "8"], backend=H.oracle_backend())
    assert c.set(ragged_update=True) is c and c.set(ragged_update=False) is c
