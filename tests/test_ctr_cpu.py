"""CPU tests of the CTR extension (include/ff_hip_ctr.h: binary cross-entropy, held-out evaluation with AUC): the symbol list against
the library and the bindings, the histogram AUC against exact pair counting, and the refusals and flags of the host layer with the CPU
oracle as kernel library (no GPU is opened).  The numbers the kernels and the model compute are tests/test_gpu_ctr.py."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import build, capi, ffmodel
import ctr_helpers as CH

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
C_HEADER = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel_c.h")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "512", "--epochs", "1"]
NEW_C_API = ["flexflow_perf_metrics_get_bce_loss", "flexflow_model_eval_batch", "flexflow_model_reset_eval_metrics",
             "flexflow_model_get_eval_metrics", "flexflow_auc_bins", "flexflow_auc_from_histograms", "flexflow_dlrm_evaluate"]
K = capi.AUC_BINS


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


# ---- 1. the header's list, the library, the bindings ----------------------------------------------------------------------------------
def test_ctr_header_list_declarations_and_prototypes_agree():
    syms = capi.ctr_header_symbols()
    assert syms and len(syms) == len(set(syms))
    assert set(syms) == set(capi._SIGS_CTR), set(syms) ^ set(capi._SIGS_CTR)
    body = open(capi.CTR_HEADER_PATH).read().split("#define FFH_CTR_API_LIST")[0]
    declared = set(re.findall(r"^int\s+(ffh_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == set(syms), declared ^ set(syms)
    # include/ff_hip.h: list and ABI version untouched by the extension
    assert not set(syms) & set(capi.header_symbols())
    assert set(capi.header_symbols()) == set(capi._SIGS)
    assert capi.header_abi_version() == 14
    assert "ctr" not in " ".join(capi.header_symbols()) and "bce" not in " ".join(capi.header_symbols())


def test_hip_library_exports_the_extension_and_the_oracle_does_not():
    path = build.build_hip()
    exp = _exported(path)
    missing = [s for s in capi.ctr_header_symbols() if s not in exp]
    assert not missing, missing
    lib = ctypes.CDLL(path)
    lib.ffh_ctr_abi_version.restype = ctypes.c_int
    assert lib.ffh_ctr_abi_version() == capi.ctr_header_abi_version()
    assert not set(capi.ctr_header_symbols()) & _exported(_oracle())
    with pytest.raises(capi.FFHError, match="no CTR extension"):
        capi.ctr_api(capi.FFHLib(_oracle()))


def test_ctypes_struct_and_constants_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ff_hip_ctr.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d\\n", sizeof(ffh_ctr_eval), offsetof(ffh_ctr_eval, logloss_sum),'
                   ' offsetof(ffh_ctr_eval, hist_pos), offsetof(ffh_ctr_eval, hist_neg), FFH_AUC_BINS, FFH_METRIC_BCE); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-lm"])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    E = capi.CtrEval
    assert got == [ctypes.sizeof(E), E.logloss_sum.offset, E.hist_pos.offset, E.hist_neg.offset, capi.AUC_BINS, capi.METRIC_BCE]
    assert K & (K - 1) == 0                                         # a power of two: p * K is exact in fp32


def test_new_c_api_is_declared_exported_and_bound():
    hdr = open(C_HEADER).read()
    exp = _exported(HOST_LIB)
    L = ffmodel.lib()
    for name in NEW_C_API:
        m = re.search(r"\b" + name + r"\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in ffmodel_c.h"
        assert name in exp, f"{name} is not exported"
        nargs = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, name).argtypes) == nargs, name
    ffh = open(os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel.h")).read()
    for py, cname in ((ffmodel.LOSS_BCE, "LOSS_BINARY_CROSSENTROPY"), (ffmodel.METRICS_BCE, "METRICS_BINARY_CROSSENTROPY"), (ffmodel.METRICS_AUC, "METRICS_AUC")):
        assert py == int(re.search(cname + r" = (\d+)", ffh).group(1))
        assert py == int(re.search(r"#define FLEXFLOW_" + cname + r" (\d+)", hdr).group(1))
    assert L.flexflow_auc_bins() == K


# ---- 2. AUC from histograms against exact pair counting --------------------------------------------------------------------------------
def _scores(case, n=32768, seed=0):
    rng = np.random.default_rng(seed)
    if case == "uniform":
        p = rng.uniform(0, 1, n).astype(np.float32)
        y = (rng.uniform(0, 1, n) < p).astype(np.float32)
    elif case == "ctr_like":                                       # a click model: most predictions small, labels drawn from them
        p = (1.0 / (1.0 + np.exp(-rng.normal(-2.0, 1.0, n)))).astype(np.float32)
        y = (rng.uniform(0, 1, n) < p).astype(np.float32)
    elif case == "few_bins":                                       # everything inside three neighbouring bins
        p = (np.float32(0.5) + rng.uniform(0, 3.0 / K, n).astype(np.float32)).astype(np.float32)
        y = (rng.uniform(0, 1, n) < 0.3 + 0.4 * (p - 0.5) * K / 3).astype(np.float32)
    elif case == "all_ties":
        p = np.full(n, 0.25, np.float32)
        y = (rng.uniform(0, 1, n) < 0.2).astype(np.float32)
    elif case in ("perfect", "inverted"):
        y = (rng.uniform(0, 1, n) < 0.3).astype(np.float32)
        hi, lo = rng.uniform(0.6, 1.0, n), rng.uniform(0.0, 0.4, n)
        p = np.where((y > 0.5) == (case == "perfect"), hi, lo).astype(np.float32)
    elif case == "no_positives":
        p = rng.uniform(0, 1, n).astype(np.float32)
        y = np.zeros(n, np.float32)
    return p, y


@pytest.mark.parametrize("case", ["uniform", "ctr_like", "few_bins", "all_ties", "perfect", "inverted", "no_positives"])
def test_auc_from_histograms_against_pair_counting(case):
    """|AUC_hist - AUC_pairs| <= 0.5 sum_k pos[k] neg[k] / (P N): only pairs inside one bin can be counted differently, each by at most one
    half.  On the main inputs the bound itself is below 1e-3, so a wrong AUC cannot hide inside it."""
    p, y = _scores(case)
    hp, hn = CH.histograms(p, y)
    got = ffmodel.auc_from_histograms(hp, hn)
    if case == "no_positives":
        assert math.isnan(got) and math.isnan(CH.auc_pairs(p, y))
        assert math.isnan(ffmodel.auc_from_histograms(hn, hp))      # ... and no negatives
        return
    exact = CH.auc_pairs(p, y)
    P, N = float(hp.sum()), float(hn.sum())
    bound = 0.5 * float((hp.astype(np.float64) * hn.astype(np.float64)).sum()) / (P * N)
    print(f"{case}: auc_hist {got:.9f} auc_pairs {exact:.9f} diff {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound + 1e-12
    assert abs(got - CH.auc_formula(hp, hn)) <= 1e-12
    if case in ("uniform", "ctr_like"):
        assert bound < 1e-3
        assert 0.6 < got < 0.9
    if case == "all_ties":
        assert got == 0.5 and exact == 0.5
    if case == "perfect":
        assert got == 1.0 and exact == 1.0
    if case == "inverted":
        assert got == 0.0 and exact == 0.0


def test_bins_are_reproduced_on_the_host():
    p = np.array([0.0, 1.0, 0.5, 1.0 / K, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.99999, 1e-30], np.float32)
    assert CH.bins_of(p).tolist() == [0, K - 1, K // 2, 1, K - 1, int(np.float32(0.99999) * np.float32(K)), 0]


# ---- 3. refusals and flags -------------------------------------------------------------------------------------------------------------
def test_driver_refuses_bce_on_a_library_without_the_extension():
    for flags in (("--loss", "bce"), ("--loss=bce",)):
        r = _driver(*flags)
        assert r.returncode != 0
        assert "without the CTR extension" in r.stderr and "include/ff_hip_ctr.h" in r.stderr and "--loss mse" in r.stderr, r.stderr[-2000:]
        assert "THROUGHPUT" not in r.stdout


def test_eval_batches_need_the_extension_too():
    r = _driver("--eval-batches", "2")
    assert r.returncode != 0 and "without the CTR extension" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("value", ["logloss", "", "BCE"])
def test_unknown_loss_value_is_refused(value):
    r = _driver(f"--loss={value}")
    assert r.returncode != 0 and f"--loss {value}: 'mse' or 'bce'" in r.stderr, r.stderr[-2000:]


def test_eval_batches_larger_than_the_data_are_refused():
    r = _driver("--eval-batches", "8")                             # 512 samples / 64 = 8 batches: none would be left to train on
    assert r.returncode != 0 and "--eval-batches 8: only 8 batches were loaded" in r.stderr, r.stderr[-2000:]
    r = _driver("--eval-only")
    assert r.returncode != 0 and "--eval-only needs --eval-batches" in r.stderr, r.stderr[-2000:]


def test_default_run_is_unchanged_apart_from_the_loss_line():
    r = _driver()
    assert r.returncode == 0, r.stderr[-2000:]
    assert "EVAL" not in r.stdout and "THROUGHPUT" in r.stdout
    assert "[DLRM] loss: mse" in r.stdout
    assert "binary_crossentropy" not in r.stderr and "mean_squared_error" in r.stderr
    m = re.search(r"Num\. iterations/epoch = (\d+)", r.stdout)
    assert m and int(m.group(1)) == 8
    r2 = _driver("--loss", "mse")
    assert r2.returncode == 0
    strip = lambda s: [l for l in s.splitlines() if "ELAPSED TIME" not in l]
    assert strip(r2.stdout) == strip(r.stdout)


_REFUSAL = r"""
import sys
sys.path.insert(0, {tests!r})
import dlrm_helpers as H
from dlrm_flexflow_amd import capi, ffmodel
case = {case!r}
cfg = ffmodel.FFConfig(argv=["-b", "16"], backend=H.oracle_backend())
m = ffmodel.FFModel(cfg)
x = m.create_tensor([16, 8], ffmodel.DT_FLOAT)
h = m.dense(x, 4, capi.AC_MODE_RELU)
if case == "no_sigmoid":
    m.dense(h, 1, capi.AC_MODE_NONE)
elif case == "two_columns":
    m.dense(h, 2, capi.AC_MODE_SIGMOID)
else:
    m.dense(h, 1, capi.AC_MODE_SIGMOID)
m.set_sgd_optimizer(lr=0.01)
if case == "auc_on_a_library_without_the_extension":
    m.compile(ffmodel.LOSS_MSE_AVG, (ffmodel.METRICS_ACCURACY, ffmodel.METRICS_AUC))
else:
    m.compile(ffmodel.LOSS_BCE, (ffmodel.METRICS_ACCURACY, ffmodel.METRICS_BCE))
print("COMPILED")
"""


@pytest.mark.parametrize("case,message", [("no_sigmoid", "--sigmoid-top"), ("two_columns", "--sigmoid-top"),
                                          ("library", "without the CTR extension"), ("auc_on_a_library_without_the_extension", "without the CTR extension")])
def test_compile_refusals(case, message):
    """compile() dies with the reason before anything is allocated; the shape of the final layer is checked before the library, so the
    oracle (which lacks the extension) still shows which refusal came first.  (The refusals that come after the library check need a
    library with the extension: tests/test_gpu_ctr.py::test_compile_refusals_behind_the_library_check.)"""
    src = _REFUSAL.format(tests=os.path.join(ROOT, "tests"), case=case)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "COMPILED" not in r.stdout
    assert message in r.stderr, r.stderr[-2000:]
    if message == "--sigmoid-top":
        assert "without the CTR extension" not in r.stderr
