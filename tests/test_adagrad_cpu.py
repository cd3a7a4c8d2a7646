"""CPU tests of Adagrad (--optimizer adagrad; include/ff_hip_adagrad.h): the numpy restatement of the rule against
torch.optim.Adagrad in float64, the property that lets the fused table update stand in for the dense sweep (an element without gradient keeps
its bits), the symbol list against the libraries and the bindings, and the flags and refusals of the driver with the CPU oracle as kernel
library (no GPU is opened).  What the kernels and the model do is tests/test_gpu_adagrad.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from dlrm_flexflow_amd import build, capi, ffmodel

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "512", "--epochs", "1"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def _driver(*extra):
    import dlrm_helpers as H
    return subprocess.run([EXE, "--backend", H.oracle_backend(), *SMALL, *extra], capture_output=True, text=True, timeout=300)


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("A", [0.0, 0.1])
def test_restatement_equals_torch_adagrad_in_float64(wd, A):
    """5 steps on 257 elements: adagrad_reference in float64 against torch.optim.Adagrad (CPU, float64).  The two differ in operation order only
    (torch: addcdiv of -lr; here lr * (gt / d)): a few float64 ulps on O(1) values, bound 1e-12 relative."""
    rng = np.random.default_rng(7)
    lr, eps = 0.05, 1e-10
    w0 = rng.standard_normal(257)
    grads = [rng.standard_normal(257) for _ in range(5)]
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adagrad([p], lr=lr, lr_decay=0, weight_decay=wd, initial_accumulator_value=A, eps=eps)
    w, S = w0.copy(), np.full(257, A)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, S = ffmodel.adagrad_reference(w, g, S, lr, eps, wd)
        assert w.dtype == np.float64 and S.dtype == np.float64
        want = p.detach().numpy()
        err = np.max(np.abs(w - want) / np.maximum(np.abs(want), 1.0))
        assert err <= 1e-12, err
        err_s = np.max(np.abs(S - opt.state[p]["sum"].numpy()) / np.maximum(S, 1.0))
        assert err_s <= 1e-12, err_s


def test_restatement_rounds_every_operation_in_float32():
    """One numpy operation per rounded operation: the float32 result is the chain of float32 roundings, not a rounding of the float64 result."""
    rng = np.random.default_rng(3)
    w, g = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    S = np.abs(rng.standard_normal(4096)).astype(np.float32)
    lr, eps, wd = np.float32(0.05), np.float32(1e-10), np.float32(1e-3)
    got_w, got_s = ffmodel.adagrad_reference(w, g, S, lr, eps, wd)
    assert got_w.dtype == np.float32 and got_s.dtype == np.float32
    gt = g + wd * w
    s1 = S + gt * gt
    want = w - lr * (gt / (np.sqrt(s1) + eps))
    assert got_w.tobytes() == want.tobytes() and got_s.tobytes() == s1.tobytes()
    w64, _ = ffmodel.adagrad_reference(w.astype(np.float64), g.astype(np.float64), S.astype(np.float64), float(lr), float(eps), float(wd))
    assert np.count_nonzero(w64.astype(np.float32) != got_w) > 0      # (the once-rounded result differs somewhere: the chain is what is specified)
    assert ffmodel.adagrad_reference(w, g, S, lr, eps, 0.0)[1].tobytes() == (S + g * g).tobytes()      # no weight decay: gt is g itself


# ---- 2. lazy equals dense ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [0.0, 0.1])
def test_elements_without_gradient_keep_their_bits(A):
    """weight_decay == 0: where g == 0, w and S come back bit for bit (-0.0, denormals, huge and tiny values included) -- so updating only the
    rows a batch touched is the dense sweep."""
    rng = np.random.default_rng(11)
    w = rng.standard_normal(1000).astype(np.float32)
    w[:8] = np.array([0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x3F800001], dtype=np.uint32).view(np.float32)
    S = np.full(1000, A, np.float32)
    S[500:] += np.abs(rng.standard_normal(500)).astype(np.float32) + np.float32(1e-3)      # rows an earlier step touched
    g = rng.standard_normal(1000).astype(np.float32)
    idle = np.arange(1000) % 3 != 1
    idle[:8] = True
    g[idle] = 0.0
    w1, S1 = ffmodel.adagrad_reference(w, g, S, 0.05, 1e-10, 0.0)
    assert w1[idle].tobytes() == w[idle].tobytes() and S1[idle].tobytes() == S[idle].tobytes()
    assert np.all(w1[~idle] != w[~idle]) and np.all(S1[~idle] > S[~idle])


# ---- 3. the driver on a library without the extension ----------------------------------------------------------------------------------------
def test_driver_on_the_oracle_is_refused_naming_the_extension_and_backend():
    r = _driver("--optimizer", "adagrad")
    assert r.returncode != 0
    assert "without the Adagrad extension" in r.stderr and "include/ff_hip_adagrad.h" in r.stderr and "--backend" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout


def test_zero_eps_with_zero_accumulator_is_refused_naming_both_flags():
    r = _driver("--optimizer", "adagrad", "--adagrad-eps", "0")
    assert r.returncode != 0
    assert "--adagrad-eps" in r.stderr and "--adagrad-initial-accumulator" in r.stderr and "0 / 0" in r.stderr, r.stderr[-2000:]
    # a positive accumulator makes eps 0 well defined: the next refusal is the library's
    r = _driver("--optimizer", "adagrad", "--adagrad-eps", "0", "--adagrad-initial-accumulator", "0.1")
    assert r.returncode != 0 and "without the Adagrad extension" in r.stderr and "0 / 0" not in r.stderr, r.stderr[-2000:]


def test_flags_parse_in_the_equals_form():
    r = _driver("--optimizer=adagrad", "--adagrad-eps=1e-8", "--adagrad-initial-accumulator=0.5")
    assert r.returncode != 0
    assert "without the Adagrad extension" in r.stderr, r.stderr[-2000:]      # (--optimizer=adagrad was read: a run with the default SGD would have trained)
    assert "THROUGHPUT" not in r.stdout
    r = _driver("--optimizer", "adagrid")
    assert r.returncode != 0 and "'adagrad'" in r.stderr


# ---- 4. the header's list, the libraries, the bindings ------------------------------------------------------------------------------------
def test_header_list_declarations_and_prototypes_agree():
    syms = capi.adagrad_header_symbols()
    assert syms == ["ffh_adagrad_abi_version", "ffh_adagrad_update", "ffh_adagrad_update_lr"]
    assert set(syms) == set(capi._SIGS_ADAGRAD)
    text = open(capi.ADAGRAD_HEADER_PATH).read()
    body = text.split("#define FFH_ADAGRAD_API_LIST")[0]
    declared = set(re.findall(r"^int\s+(ffh_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == set(syms), declared ^ set(syms)
    assert capi.adagrad_header_abi_version() == 1
    assert int(re.search(r"#define FFH_SPARSE_OPT_ADAGRAD\s+(\d+)", text).group(1)) == capi.SPARSE_OPT_ADAGRAD == 3
    # include/ff_hip.h: list and ABI version untouched by the extension
    assert not set(syms) & set(capi.header_symbols())
    assert set(capi.header_symbols()) == set(capi._SIGS)
    assert capi.header_abi_version() == 14
    for name in ("ffh_adagrad_update", "ffh_adagrad_update_lr"):
        params = re.search(rf"^int\s+{name}\s*\((.*?)\);", body, re.M | re.S).group(1)
        assert len(params.split(",")) == len(capi._SIGS_ADAGRAD[name][1]), name


def test_hip_library_exports_the_extension_and_the_oracle_does_not(oracle):
    exp = _exported(build.build_hip())
    assert set(capi.adagrad_header_symbols()) <= exp
    assert {s for s in exp if "adagrad" in s} == set(capi.adagrad_header_symbols())
    assert not set(capi.adagrad_header_symbols()) & _exported(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no Adagrad extension"):
        capi.adagrad_api(oracle.lib())


def test_c_api_and_python_face_export_the_optimizer():
    assert {"flexflow_adagrad_optimizer_create", "flexflow_model_set_adagrad_optimizer", "flexflow_config_set_adagrad"} <= _exported(HOST_LIB)
    assert callable(ffmodel.AdagradOptimizer) and callable(ffmodel.FFModel.set_adagrad_optimizer) and callable(ffmodel.adagrad_reference)
