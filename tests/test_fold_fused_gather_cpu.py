"""Host-only checks of the fused-gather extension (include/ffh_fused_gather.h: ffh_fused_gather_linear_fwd and its plan twin) under the rule of
tests/test_extension_loader_cpu.py, through its stub libraries: the entries are in the header's list and in capi's signatures, the fold header is
left as it was, absent is fine, part of the list or another version is refused by both loaders."""
import re

import pytest

from dlrm_flexflow_amd import capi
from test_extension_loader_cpu import _aborted_with, _construct, _driver, stub      # noqa: F401  (stub: the fixture)

EXT = capi.EXTENSIONS["fused_gather"]
NEW = ("ffh_fused_gather_linear_fwd", "ffh_fused_gather_linear_fwd_plan")


def _whole(version):
    return {s: (version if s == "ffh_fused_gather_abi_version" else 0) for s in EXT.header_symbols()}


def test_the_entries_are_in_the_abi_list():
    syms = EXT.header_symbols()
    assert EXT.header == "include/ffh_fused_gather.h" and EXT.header_abi_version() == 1
    assert set(syms) == set(capi._SIGS_FUSED_GATHER) == set(NEW) | {"ffh_fused_gather_abi_version"}
    assert not set(NEW) & set(capi.fold_header_symbols()) and capi.fold_header_abi_version() == 3, "include/ff_hip_fold.h is left as it was"
    entry, plan = (capi._SIGS_FUSED_GATHER[s][1] for s in NEW)
    assert entry[:-1] == plan and len(entry) == len(plan) + 1, "the plan twin takes the entry's arguments without the stream"


def test_the_whole_extension_loads_and_absent_is_fine(stub, oracle):
    r = _construct(stub("fused_fold_gather_whole", _whole(1)))
    assert r.returncode == 0 and "LOADED oracle-cpu" in r.stdout and "FATAL" not in r.stderr, r.stderr[-2000:]
    lib = capi.FFHLib(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match=r"no fused-gather extension \(ffh_\w+ missing; include/ffh_fused_gather.h\)"):
        capi.fused_gather_api(lib)
    lib.close()


@pytest.mark.parametrize("gone", NEW)
def test_part_of_it_is_refused(stub, gone):
    path = stub("fused_fold_gather_without_" + gone, {s: v for s, v in _whole(1).items() if s != gone})
    _aborted_with(_driver(path), "FATAL: %s exports part of include/ffh_fused_gather.h: %s is missing" % (path, gone))
    lib = capi.FFHLib(path)
    with pytest.raises(capi.FFHError, match=r"no fused-gather extension \(%s missing; include/ffh_fused_gather.h\)" % gone):
        capi.fused_gather_api(lib)
    lib.close()


def test_another_version_is_refused(stub):
    path = stub("fused_fold_gather_v2", _whole(2))
    _aborted_with(_driver(path), "FATAL: %s has fused-gather ABI version 2, expected 1" % path)
    lib = capi.FFHLib(path)
    with pytest.raises(capi.FFHError, match=re.escape("fused-gather ABI version 2, include/ffh_fused_gather.h says 1 (rebuild)")):
        capi.fused_gather_api(lib)
    lib.close()
