"""The ragged table update's two-call form (include/ff_hip_bags_sort.h) without a GPU: the surface of the extension, and
the host layer on the CPU oracle -- which has neither the ragged update nor its pair, so a mixed model given --early-sort sorts in front of its
apply, once per bag size, and trains to the bits of --no-early-sort."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import bags_helpers as BH
import dlrm_helpers as H

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
_DRIVER = ["-b", "16", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "50-7-300", "--arch-mlp-bot", "13-16-8", "--arch-mlp-top", "32-16-1",
           "--data-size", "64", "--epochs", "2", "--embedding-bag-sizes", "1-3-2"]


def test_library_exports_the_bags_sort_extension():
    """libffhip.so exports every symbol of include/ff_hip_bags_sort.h with the header's ABI version (loadable without a GPU); the three
    existing lists keep their lengths and versions and share no symbol with it; the oracle lacks the extension."""
    lib = ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL)
    syms = capi.bags_sort_header_symbols()
    assert set(syms) == set(capi._SIGS_BAGS_SORT) == {"ffh_bags_sort_abi_version", "ffh_embedding_bwd_sort_multi_bags", "ffh_embedding_bwd_apply_multi_bags"}
    assert len(syms) == 3
    for s in syms:
        assert hasattr(lib, s), s
    lib.ffh_bags_sort_abi_version.restype = ctypes.c_int
    assert lib.ffh_bags_sort_abi_version() == capi.bags_sort_header_abi_version() == 1
    base, bags, update = capi.header_symbols(), capi.bags_header_symbols(), capi.bags_update_header_symbols()
    assert set(syms).isdisjoint(base) and set(syms).isdisjoint(bags) and set(syms).isdisjoint(update)
    assert capi.bags_header_abi_version() == 1 and len(bags) == 4                  # ff_hip_bags.h keeps its list
    assert capi.bags_update_header_abi_version() == 1 and len(update) == 4         # ff_hip_bags_update.h too
    lib.ffh_abi_version.restype = ctypes.c_int
    assert lib.ffh_abi_version() == capi.header_abi_version() and len(base) == len(set(base))      # ff_hip.h: as the header says
    oracle = capi.FFHLib(H.oracle_backend())
    for s in syms:
        assert not hasattr(oracle.lib, s), s
    with pytest.raises(capi.FFHError, match="no bags-sort extension"):
        capi.bags_sort_api(oracle)
    oracle.close()


def test_the_pair_takes_the_fused_descriptor():
    """Both entries are declared on struct ffh_bags_update, whose layout include/ff_hip_bags_update.h pins."""
    for name in ("ffh_embedding_bwd_sort_multi_bags", "ffh_embedding_bwd_apply_multi_bags"):
        assert capi._SIGS_BAGS_SORT[name] == capi._SIGS_BAGS_UPDATE["ffh_embedding_bwd_fused_multi_bags"]
    assert ctypes.sizeof(capi.BagsUpdate) == 80


def test_driver_on_the_oracle_takes_early_sort_and_prints_no_suffix():
    """--early-sort is a scheduling wish: on a library without the pair a mixed model is not refused, sorts in front of its apply and says
    nothing about a sort behind the gather."""
    for flag in (["--early-sort"], ["--early-sort", "--ragged-update"], ["--early-sort", "--no-ragged-update"]):
        r = subprocess.run([EXE, "--backend", H.oracle_backend()] + _DRIVER + flag, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "[DLRM] embedding update: per bag size, 3 calls per step (the kernel library has no ragged update)\n" in r.stdout, r.stdout
        assert "sorted behind the gather" not in r.stdout and "THROUGHPUT = " in r.stdout


def test_early_sort_on_the_oracle_trains_to_the_bits_of_no_early_sort():
    cnt = ("early_sorts", "ragged_early_sorts", "ragged_update_launches")
    a, ca = BH.trajectory(H.oracle_backend(), _DRIVER + ["--early-sort"], 3, trace=False, counters=cnt)
    b, cb = BH.trajectory(H.oracle_backend(), _DRIVER + ["--no-early-sort"], 3, trace=False, counters=cnt)
    assert ca == cb == {"early_sorts": 0, "ragged_early_sorts": 0, "ragged_update_launches": 0}
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
