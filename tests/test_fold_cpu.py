"""CPU tests of the fold extension's boundary (include/ff_hip_fold.h): the product library exports exactly the header's list and the ctypes prototypes
cover it; the CPU oracle does not export it, and a model on the oracle therefore folds nothing and trains as it did before the route existed."""
import subprocess

import fold_helpers as FH
import dlrm_helpers as H
from dlrm_flexflow_amd import capi


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_fold_header_list_matches_prototypes_and_library():
    from dlrm_flexflow_amd import build
    syms = capi.fold_header_symbols()
    assert len(syms) == len(set(syms)) and set(syms) == set(capi._SIGS_FOLD)
    exp = _exported(build.build_hip())
    assert {s for s in exp if s.startswith("ffh_fold_")} == set(syms)


def test_oracle_does_not_export_the_fold_extension(oracle):
    assert not [s for s in _exported(oracle.ORACLE_LIB) if s.startswith("ffh_fold_")]


def test_model_on_the_oracle_folds_nothing_and_ignores_the_switch():
    """Without the extension the host takes the route of before: no table is folded, and --no-fold-small-tables changes no bit of three steps."""
    runs = [FH.run_model(H.oracle_backend(), flags) for flags in ([], ["--no-fold-small-tables"])]
    for r in runs:
        assert r["folded"] == 0
    assert runs[0]["w1"].keys() == runs[1]["w1"].keys() and len(runs[0]["w1"]) >= 6 + 2 * 5
    for k in runs[0]["w1"]:
        assert runs[0]["w0"][k].tobytes() == runs[1]["w0"][k].tobytes()
        assert runs[0]["w1"][k].tobytes() == runs[1]["w1"][k].tobytes(), k
        assert runs[0]["w1"][k].tobytes() != runs[0]["w0"][k].tobytes() or k.startswith("Embedding"), f"{k}: three steps left it unchanged"
    assert runs[0]["pred"].tobytes() == runs[1]["pred"].tobytes()
