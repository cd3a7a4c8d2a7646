"""The rule both loaders apply to an optional extension of the kernel C-ABI (host/backend.cc and capi.py), pinned without a GPU:

    absent is fine; present means every symbol of the header's FFH_<X>_API_LIST and ffh_<x>_abi_version() == FFH_<X>_ABI_VERSION;
    anything else fails loudly, naming the library, the header and the symbol.

Every library here is the CPU oracle (which exports no extension) plus stub symbols `int name(void) { return V; }`: a small shared object
linked against the oracle, so that a dlsym on its handle finds the base ABI in the dependency.  The children only LOAD a library (the
model's constructor is where the host layer loads it); nothing ever calls a stub entry."""
import glob
import os
import re
import signal
import subprocess
import sys

import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")

# key (the <x> of capi.<x>_api, capi.<X>_HEADER_PATH, ffh_<x>_abi_version) -> the label of the version message, in load order
LABELS = {"bf16": "bf16", "ctr": "CTR", "lr": "learning-rate", "data": "data", "cross": "cross", "digest": "digest", "adagrad": "Adagrad",
          "rowwise": "row-wise Adagrad", "fold": "fold", "bags": "bags", "bags_update": "bags-update", "bags_sort": "bags-sort", "pad": "pad",
          "pad_mean": "pad-mean", "q8": "q8"}
NO_LABELS = dict(LABELS, bf16="bf16-table")       # the label of capi's "no ... extension" message: one text differs
KEYS = list(LABELS)
FOLD_ABI3 = ("ffh_fold_linear_bwd_dx", "ffh_fold_table_update")      # prefixes of the entries fold ABI 3 added


def _header(x):
    return getattr(capi, x.upper() + "_HEADER_PATH")


def _include(x):
    return "include/" + os.path.basename(_header(x))


def _symbols(x):
    return getattr(capi, x + "_header_symbols")()


def _version(x):
    return getattr(capi, x + "_header_abi_version")()


@pytest.fixture(scope="module")
def stub(oracle, tmp_path_factory):
    """stub(name, {symbol: return value}) -> path of a library that is the oracle plus those symbols."""
    d = tmp_path_factory.mktemp("stubs")
    odir = os.path.dirname(oracle.ORACLE_LIB)

    def make(name, symbols):
        src, out = str(d / (name + ".c")), str(d / ("lib" + name + ".so"))
        with open(src, "w") as f:
            f.write("".join("int %s(void) { return %d; }\n" % (s, v) for s, v in symbols.items()))
        subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", out, src, "-Wl,--no-as-needed", "-L" + odir, "-lffh_oracle", "-Wl,-rpath," + odir])
        return out
    return make


def _whole(x, version):
    return {s: (version if s == "ffh_%s_abi_version" % x else 0) for s in _symbols(x)}


def _driver(path):
    """The dlrm driver on `path`: for the loads that must abort (it dies in the model's constructor, before it builds anything)."""
    return subprocess.run([EXE, "--backend", path, "-b", "8"], capture_output=True, text=True, timeout=120)


def _construct(path):
    """A Python child that constructs the model on `path` and does nothing else: for the loads that must succeed."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dlrm_flexflow_amd import ffmodel\n"
            "m = ffmodel.FFModel(ffmodel.FFConfig(argv=['-b', '8'], backend=%r))\n"
            "print('LOADED', m.backend['name'])\n" % (ROOT, path))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


def _aborted_with(r, line):
    assert r.returncode == -signal.SIGABRT, (r.returncode, r.stderr[-2000:])
    assert line in r.stderr.splitlines(), (line, r.stderr[-2000:])
    assert "THROUGHPUT" not in r.stdout


def test_the_registry_is_the_set_of_extension_headers():
    """(e) every include/ff_hip_*.h with an _API_LIST is an extension capi knows, and the other way round: fifteen of them."""
    known = {n[:-len("_HEADER_PATH")].lower() for n in vars(capi) if n.endswith("_HEADER_PATH")}
    assert known == set(KEYS)
    with_list = {p for p in glob.glob(os.path.join(ROOT, "include", "ff_hip_*.h")) if re.search(r"#define FFH_\w+_API_LIST\(X\)", open(p).read())}
    assert with_list == {os.path.normpath(_header(x)) for x in KEYS} and len(with_list) == 15
    for x in KEYS:
        assert os.path.basename(_header(x)) == "ff_hip_%s.h" % x
        syms = _symbols(x)
        assert "ffh_%s_abi_version" % x in syms and set(syms) == set(getattr(capi, "_SIGS_" + x.upper()))


@pytest.mark.parametrize("x", KEYS)
def test_part_of_an_extension_is_refused(stub, x):
    """(a) the version symbol alone: the host layer names the first entry of the header's list that is missing."""
    rest = [s for s in _symbols(x) if s != "ffh_%s_abi_version" % x]
    if not rest:
        assert x == "rowwise"
        pytest.skip("include/ff_hip_rowwise.h lists the version symbol only: there is no part of it")
    path = stub("part_" + x, {"ffh_%s_abi_version" % x: _version(x)})
    _aborted_with(_driver(path), "FATAL: %s exports part of %s: %s is missing" % (path, _include(x), rest[0]))
    lib = capi.FFHLib(path)
    with pytest.raises(capi.FFHError, match=r"no %s extension \(ffh_\w+ missing; %s\)" % (re.escape(NO_LABELS[x]), re.escape(_include(x)))):
        getattr(capi, x + "_api")(lib)
    lib.close()


@pytest.mark.parametrize("x", KEYS)
def test_another_version_is_refused(stub, x):
    """(b) the whole list with a version symbol that returns the header's version + 1: refused by both loaders, each in its own words."""
    n = _version(x)
    path = stub("version_" + x, _whole(x, n + 1))
    _aborted_with(_driver(path), "FATAL: %s has %s ABI version %d, expected %d" % (path, LABELS[x], n + 1, n))
    lib = capi.FFHLib(path)
    with pytest.raises(capi.FFHError, match=r"%s ABI version %d, %s says %d \(rebuild\)" % (re.escape(LABELS[x]), n + 1, re.escape(_include(x)), n)):
        getattr(capi, x + "_api")(lib)
    lib.close()


def test_a_fold_version_older_than_2_is_refused(stub):
    """(b) fold accepts ABI 2 beside the current one (below) and nothing else."""
    n = _version("fold")
    assert n == 3
    path = stub("version_fold_1", _whole("fold", 1))
    _aborted_with(_driver(path), "FATAL: %s has fold ABI version 1, expected %d" % (path, n))


def test_an_absent_extension_is_fine(oracle):
    """(c) the plain oracle exports none of the fifteen: capi says so one by one, the host layer loads it without a word."""
    lib = capi.FFHLib(oracle.ORACLE_LIB)
    for x in KEYS:
        with pytest.raises(capi.FFHError, match=r"no %s extension \(ffh_\w+ missing; %s\)" % (re.escape(NO_LABELS[x]), re.escape(_include(x)))):
            getattr(capi, x + "_api")(lib)
    lib.close()
    r = _construct(oracle.ORACLE_LIB)
    assert r.returncode == 0 and "LOADED oracle-cpu" in r.stdout and "FATAL" not in r.stderr, r.stderr[-2000:]


def test_a_fold_library_of_abi_2_loads_without_the_abi_3_entries(stub):
    """(d) fold ABI 2 is taken as it is, the entries ABI 3 added left out; an ABI 2 entry may still not be missing."""
    syms = _whole("fold", 2)
    abi2 = {s: v for s, v in syms.items() if not s.startswith(FOLD_ABI3)}
    assert len(syms) - len(abi2) == 4 and len(abi2) == 9
    r = _construct(stub("fold_abi2", abi2))
    assert r.returncode == 0 and "LOADED oracle-cpu" in r.stdout and "FATAL" not in r.stderr, r.stderr[-2000:]
    for gone in ("ffh_fold_product", "ffh_fold_linear_bwd_dw_plan"):
        path = stub("fold_abi2_without_" + gone, {s: v for s, v in abi2.items() if s != gone})
        _aborted_with(_driver(path), "FATAL: %s exports part of include/ff_hip_fold.h: %s is missing" % (path, gone))
    # ... and the entries ABI 3 added may be missing under ABI 2 only
    path = stub("fold_abi3_part", dict(abi2, ffh_fold_abi_version=3))
    _aborted_with(_driver(path), "FATAL: %s exports part of include/ff_hip_fold.h: ffh_fold_linear_bwd_dx is missing" % path)
