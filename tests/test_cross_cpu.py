"""CPU tests of the DCNv2 low-rank cross interaction (--arch-interaction-op dcn; include/ff_hip_cross.h): the float32
numpy restatement of the combine against torch float64 autograd, the symbol list against the libraries and the bindings, and the flags,
the start-up line and the refusals of the driver with the CPU oracle as kernel library (no GPU is opened).  What the kernels and the
model do is tests/test_gpu_cross.py."""
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
# concat width 8 + 3 x 8 = 32
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--data-size", "512", "--epochs", "1"]
TOP_OK = ["--arch-mlp-top", "32-16-1"]


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


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def _operands(shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-2, 2, shape).astype(np.float32) for _ in range(4)]


# A float32 product and a float32 sum, each rounded once: against exact arithmetic on the same float32 inputs (float64 holds the product of two
# float32 exactly and rounds the sum at 2^-53) the error is at most half an ulp of each result, 2^-24 (|a b| + |a b + c|) <= 2^-23 (|a b| + |c|).
def _bound(prod, add):
    return 2.0 ** -23 * (np.abs(prod) + np.abs(add)) + 1e-300


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (64, 67)])
def test_cross_reference_forward_and_backward_equal_torch_float64_autograd(shape, aliased):
    x0, v, xl, dy = _operands(shape, 7)
    t0 = torch.tensor(x0.astype(np.float64), requires_grad=True)
    tv = torch.tensor(v.astype(np.float64), requires_grad=True)
    tl = t0 if aliased else torch.tensor(xl.astype(np.float64), requires_grad=True)
    y = t0 * tv + tl
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    got = ffmodel.cross_reference(x0, v, x0 if aliased else xl)
    assert got.dtype == np.float32 and got.shape == shape
    base = x0 if aliased else xl
    assert np.all(np.abs(got.astype(np.float64) - y.detach().numpy()) <= _bound(x0.astype(np.float64) * v, base))
    dv, g0, gl = ffmodel.cross_reference_backward(dy, x0, v, aliased=aliased)
    assert dv.dtype == np.float32 and g0.dtype == np.float32
    assert np.all(np.abs(dv.astype(np.float64) - tv.grad.numpy()) <= _bound(dy.astype(np.float64) * x0, 0.0))
    if aliased:
        assert gl is None
        assert np.all(np.abs(g0.astype(np.float64) - t0.grad.numpy()) <= _bound(dy.astype(np.float64) * v, dy))
    else:
        assert np.all(np.abs(g0.astype(np.float64) - t0.grad.numpy()) <= _bound(dy.astype(np.float64) * v, 0.0))
        assert gl.tobytes() == dy.tobytes() and np.array_equal(tl.grad.numpy(), dy.astype(np.float64))


def test_cross_reference_rounds_twice():
    """a * b + c with the product rounded to float32 first: 2^-12 squared is lost beside 1 only when the product is rounded on its own."""
    a = np.float32(1 + 2.0 ** -12)
    exact = float(a) * float(a) - 1.0                        # 2^-11 + 2^-24
    got = ffmodel.cross_reference(np.array([a]), np.array([a]), np.array([-1.0], np.float32))[0]
    assert got == np.float32(2.0 ** -11) and float(got) != exact        # an fma would return 2^-11 + 2^-24


# ---- 2. the header's list, the libraries, the bindings ---------------------------------------------------------------------------------
def test_cross_header_list_declarations_and_prototypes_agree():
    syms = capi.cross_header_symbols()
    assert syms == ["ffh_cross_abi_version", "ffh_cross_fwd", "ffh_cross_bwd"]
    assert set(syms) == set(capi._SIGS_CROSS)
    text = open(capi.CROSS_HEADER_PATH).read()
    body = text.split("#define FFH_CROSS_API_LIST")[0]
    declared = set(re.findall(r"^int\s+(ffh_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == set(syms), declared ^ set(syms)
    assert capi.cross_header_abi_version() == 1
    for name, val in (("SKIP", capi.CROSS_SKIP), ("STORE", capi.CROSS_STORE), ("ADD", capi.CROSS_ADD)):
        assert int(re.search(rf"#define FFH_CROSS_{name}\s+(\d+)", text).group(1)) == val
    # include/ff_hip.h: list and ABI version untouched by the extension
    assert not set(syms) & set(capi.header_symbols())
    assert set(capi.header_symbols()) == set(capi._SIGS)
    assert capi.header_abi_version() == 14
    # argument counts of the prototypes: ctx + the header's parameters
    for name in ("ffh_cross_fwd", "ffh_cross_bwd"):
        params = re.search(rf"^int\s+{name}\s*\((.*?)\);", body, re.M | re.S).group(1)
        assert len(params.split(",")) == len(capi._SIGS_CROSS[name][1]), name


def test_hip_library_exports_the_extension_and_the_oracle_does_not(oracle):
    exp = _exported(build.build_hip())
    assert set(capi.cross_header_symbols()) <= exp
    assert not set(capi.cross_header_symbols()) & _exported(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no cross extension"):
        capi.cross_api(oracle.lib())


def test_c_api_and_python_face_export_the_operators():
    assert {"flexflow_model_add_cross_combine", "flexflow_model_add_cross_net"} <= _exported(HOST_LIB)
    assert callable(ffmodel.FFModel.cross_combine) and callable(ffmodel.FFModel.cross_net)


# ---- 3. flags, the start-up line, refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,L,R", [
    (("--arch-interaction-op", "dcn"), 3, 512),                                                    # the defaults
    (("--arch-interaction-op", "dcn", "--dcn-num-layers", "2", "--dcn-low-rank-dim", "4"), 2, 4),
    (("--arch-interaction-op=dcn", "--dcn-num-layers=5", "--dcn-low-rank-dim=16"), 5, 16),
    (("--dcn-low-rank-dim=7", "--arch-interaction-op", "dcn", "--dcn-num-layers", "1"), 1, 7),
])
def test_flags_start_up_line_and_refusal_on_a_library_without_the_extension(flags, L, R):
    """The flags in both forms reach the driver (its start-up line says what it will build); the CPU oracle has no cross extension, so
    compile() refuses the model before anything runs, naming the flag to change."""
    r = _driver(*TOP_OK, *flags)
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("[DLRM] interaction")] == [f"[DLRM] interaction: dcn layers {L} rank {R}"], r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode != 0
    assert "without the cross extension" in r.stderr and "include/ff_hip_cross.h" in r.stderr and "--arch-interaction-op" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout
    # the new line sits behind the MLP lines; nothing else moved
    heads = [l.split(":")[0] for l in lines if l.startswith("[DLRM]")]
    assert heads[:6] == ["[DLRM] batchSize(64) workersPerNodes(0) numNodes(1)", "[DLRM] EmbeddingBagSize(1)", "[DLRM] Embedding Vocab Sizes",
                         "[DLRM] MLP Top", "[DLRM] MLP Bot", "[DLRM] interaction"], heads


@pytest.mark.parametrize("top", ["33-16-1", "8-16-1"])
def test_top_mlp_width_mismatch_is_refused(top):
    r = _driver("--arch-mlp-top", top, "--arch-interaction-op", "dcn", "--dcn-low-rank-dim", "4")
    assert r.returncode != 0
    assert "--arch-mlp-top must start with the interaction's width 32" in r.stderr and f"not {top.split('-')[0]}" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout


@pytest.mark.parametrize("flags,msg", [(("--dcn-num-layers", "0"), "--dcn-num-layers 0: must be >= 1"),
                                       (("--dcn-low-rank-dim=0",), "--dcn-low-rank-dim 0: must be >= 1")])
def test_non_positive_sizes_are_refused(flags, msg):
    r = _driver(*TOP_OK, "--arch-interaction-op", "dcn", *flags)
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-2000:]


def test_other_interactions_say_nothing_new_and_unknown_ones_name_dcn():
    r = _driver(*TOP_OK)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "interaction" not in r.stdout and "THROUGHPUT" in r.stdout
    # the dcn sizes are inert without the interaction
    r2 = _driver(*TOP_OK, "--dcn-num-layers", "9", "--dcn-low-rank-dim=3")
    strip = lambda s: [l for l in s.splitlines() if "ELAPSED TIME" not in l]
    assert r2.returncode == 0 and strip(r2.stdout) == strip(r.stdout)
    r3 = _driver(*TOP_OK, "--arch-interaction-op", "dcnv3")
    assert r3.returncode != 0 and "'dcn'" in r3.stderr
