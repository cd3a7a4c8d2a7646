"""CPU tests of row-wise Adagrad (--optimizer adagrad --adagrad-rowwise; include/ff_hip_rowwise.h): the numpy restatement of the
rule and its TREE sum order, the property that lets the fused table update stand in for a sweep (a row without gradient keeps its bits), the
symbol list against the libraries and the bindings, and the flag and the refusals of the driver with the CPU oracle as kernel library (no GPU is
opened).  What the kernels and the model do is tests/test_gpu_rowwise.py and tests/test_gpu_rowwise_model.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import build, capi, ffmodel

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "512", "--epochs", "1"]
ROWWISE = ["--optimizer", "adagrad", "--adagrad-rowwise"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def _driver(*extra):
    import dlrm_helpers as H
    return subprocess.run([EXE, "--backend", H.oracle_backend(), *SMALL, *extra], capture_output=True, text=True, timeout=300)


# ---- 1. the reference function ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_width_one_equals_the_element_wise_restatement_bit_for_bit(wd):
    rng = np.random.default_rng(5)
    w, g = rng.standard_normal((4096, 1)).astype(np.float32), rng.standard_normal((4096, 1)).astype(np.float32)
    S = np.abs(rng.standard_normal(4096)).astype(np.float32)
    S[::7] = 0.0
    for _ in range(3):
        w1, S1 = ffmodel.rowwise_adagrad_reference(w, g, S, 0.05, 1e-10, wd)
        w2, S2 = ffmodel.adagrad_reference(w, g, S[:, None], 0.05, 1e-10, wd)
        assert w1.dtype == np.float32 and S1.dtype == np.float32 and S1.shape == (4096,)
        assert w1.tobytes() == w2.tobytes() and S1.tobytes() == S2.tobytes()
        w, S, g = w1, S1, rng.standard_normal((4096, 1)).astype(np.float32)


def _float64_rule(w, g, S, lr, eps, wd):
    """the same rule written in float64, with numpy's own (pairwise) sum: the order matters only at float64 rounding"""
    w, g, S = w.astype(np.float64), g.astype(np.float64), S.astype(np.float64)
    gt = g + wd * w
    S = S + (gt * gt).sum(axis=1) / w.shape[1]
    return w - lr * (gt / (np.sqrt(S) + eps)[:, None]), S


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("D", [3, 13, 48, 64, 320])
def test_float32_restatement_agrees_with_the_rule_in_float64(D, wd):
    """rtol 1e-6 on w and S, no atol.  S and the step lr * q are fewer than log2(P) + 6 rounded float32 operations on positive terms (the
    tree's log2(P) <= 9 levels; the square, the division by D, the addition to S, the square root, the sum with eps, the quotient; the
    product with lr), each within 2^-24 relative: under 15 * 6e-8 = 9e-7.  w - step rounds once more and can cancel, so the inputs keep
    |step| <= |w| / 2 (|w| in [0.5, 1.5]; S >= 0.05 and |g| < 5.5 give |step| <= 0.01 * 5.5 / sqrt(0.05) < 0.25): the step's error is then
    at most the same fraction of w - step."""
    rng = np.random.default_rng(D)
    w = (rng.uniform(0.5, 1.5, (257, D)) * rng.choice([-1.0, 1.0], (257, D))).astype(np.float32)
    g = np.clip(rng.standard_normal((257, D)), -5.5, 5.5).astype(np.float32)
    S = rng.uniform(0.05, 0.15, 257).astype(np.float32)
    w1, S1 = ffmodel.rowwise_adagrad_reference(w, g, S, 0.01, 1e-10, wd)
    w2, S2 = _float64_rule(w, g, S, 0.01, 1e-10, wd)
    assert w1.dtype == np.float32 and S1.dtype == np.float32
    np.testing.assert_allclose(S1, S2, rtol=1e-6, atol=0)
    np.testing.assert_allclose(w1, w2, rtol=1e-6, atol=0)
    assert np.abs(w2 - w).max() <= 0.25 and np.abs(w2 - w).max() > 1e-3
    # the float64 form of the restatement itself (the same statements in the dtype of w)
    w3, S3 = ffmodel.rowwise_adagrad_reference(w.astype(np.float64), g.astype(np.float64), S.astype(np.float64), 0.01, 1e-10, wd)
    assert w3.dtype == np.float64
    np.testing.assert_allclose(w3, w2, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(S3, S2, rtol=1e-12, atol=0)


@pytest.mark.parametrize("A", [0.0, 0.1])
def test_rows_without_gradient_keep_their_bits(A):
    """weight_decay == 0: a row whose gradient is all +0 gets w and S back bit for bit (-0.0, denormals, huge and tiny values included) -- so
    updating only the rows a batch touched is the sweep over the table."""
    rng = np.random.default_rng(11)
    w = rng.standard_normal((300, 13)).astype(np.float32)
    w[:, :8] = np.array([0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x3F800001], dtype=np.uint32).view(np.float32)
    S = np.full(300, A, np.float32)
    S[150:] += np.abs(rng.standard_normal(150)).astype(np.float32) + np.float32(1e-3)      # rows an earlier step touched
    g = rng.standard_normal((300, 13)).astype(np.float32)
    idle = np.arange(300) % 3 != 1
    g[idle] = 0.0
    w1, S1 = ffmodel.rowwise_adagrad_reference(w, g, S, 0.05, 1e-10, 0.0)
    assert w1[idle].tobytes() == w[idle].tobytes() and S1[idle].tobytes() == S[idle].tobytes()
    assert np.all(S1[~idle] > S[~idle]) and np.all(w1[~idle][:, 8:] != w[~idle][:, 8:])


@pytest.mark.parametrize("D", [1, 3, 13, 48, 64, 70, 320])
def test_tree_of_a_row_equals_tree_of_the_zero_padded_row(D):
    rng = np.random.default_rng(D + 100)
    t = np.square(rng.standard_normal((64, D)).astype(np.float32))
    P = 1 << (D - 1).bit_length()
    padded = np.concatenate([t, np.zeros((64, P - D), np.float32)], axis=1)
    twice = np.concatenate([t, np.zeros((64, 2 * P - D), np.float32)], axis=1)
    got = ffmodel.rowwise_tree_sum(t)
    assert got.dtype == np.float32 and got.shape == (64,)
    assert got.tobytes() == ffmodel.rowwise_tree_sum(padded).tobytes() == ffmodel.rowwise_tree_sum(twice).tobytes()
    # the order written out: level k adds the elements whose indices differ in bit k
    x = padded.copy()
    stride = 1
    while stride < P:
        x[:, 0::2 * stride] = x[:, 0::2 * stride] + x[:, stride::2 * stride]
        stride *= 2
    assert got.tobytes() == x[:, 0].tobytes()
    if D >= 48:      # (it is an order of its own: the left-to-right sum differs somewhere)
        seq = np.zeros(64, np.float32)
        for j in range(D):
            seq = seq + t[:, j]
        assert np.count_nonzero(seq != got) > 0


# ---- 2. header and symbols -----------------------------------------------------------------------------------------------------------------
def test_header_list_declarations_and_bindings_agree():
    syms = capi.rowwise_header_symbols()
    assert syms == ["ffh_rowwise_abi_version"]
    assert set(syms) == set(capi._SIGS_ROWWISE)
    text = open(capi.ROWWISE_HEADER_PATH).read()
    body = text.split("#define FFH_ROWWISE_API_LIST")[0]
    declared = set(re.findall(r"^int\s+(ffh_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == set(syms), declared ^ set(syms)
    assert re.search(r"^int\s+ffh_rowwise_abi_version\s*\(void\);", body, re.M) and capi._SIGS_ROWWISE["ffh_rowwise_abi_version"][1] == []
    assert capi.rowwise_header_abi_version() == 1
    assert int(re.search(r"#define FFH_SPARSE_OPT_ROWWISE_ADAGRAD\s+(\d+)", text).group(1)) == capi.SPARSE_OPT_ROWWISE_ADAGRAD == 8
    # include/ff_hip.h and include/ff_hip_adagrad.h: lists and ABI versions untouched by the extension
    assert capi.header_abi_version() == 14 and set(capi.header_symbols()) == set(capi._SIGS)
    assert capi.adagrad_header_abi_version() == 1
    assert capi.adagrad_header_symbols() == ["ffh_adagrad_abi_version", "ffh_adagrad_update", "ffh_adagrad_update_lr"]
    assert not set(syms) & (set(capi.header_symbols()) | set(capi.adagrad_header_symbols()))
    assert capi.SPARSE_OPT_ADAGRAD == 3


def test_hip_library_exports_the_extension_and_the_oracle_does_not(oracle):
    exp = _exported(build.build_hip())
    assert {s for s in exp if "rowwise" in s} == set(capi.rowwise_header_symbols())
    assert not {s for s in _exported(oracle.ORACLE_LIB) if "rowwise" in s}
    with pytest.raises(capi.FFHError, match="no row-wise Adagrad extension"):
        capi.rowwise_api(oracle.lib())


def test_c_api_and_python_face_export_the_switch():
    assert {"flexflow_config_set_adagrad_rowwise", "flexflow_adagrad_optimizer_set_rowwise"} <= _exported(HOST_LIB)
    hdr = open(os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel_c.h")).read()
    L = ffmodel.lib()
    for name in ("flexflow_config_set_adagrad_rowwise", "flexflow_adagrad_optimizer_set_rowwise"):
        m = re.search(r"\b" + name + r"\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == len(getattr(L, name).argtypes) == 2, name
    assert re.search(r"flexflow_adagrad_optimizer_create\(flexflow_model_t, double lr, double weight_decay, double epsilon, double initial_accumulator\);", hdr)
    assert callable(ffmodel.rowwise_adagrad_reference) and callable(capi.rowwise_api)
    import inspect
    assert inspect.signature(ffmodel.AdagradOptimizer.__init__).parameters["rowwise"].default is False
    assert "adagrad_rowwise" in inspect.signature(ffmodel.FFConfig.set).parameters


# ---- 3. the driver on the oracle backend: every refusal names the flag to change ------------------------------------------------------------
def test_flag_without_adagrad_is_refused():
    for opt in ([], ["--optimizer", "adam"]):
        r = _driver("--adagrad-rowwise", *opt)
        assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
        assert "--adagrad-rowwise" in r.stderr and "--optimizer adagrad" in r.stderr, r.stderr[-2000:]


def test_flag_with_the_dense_table_update_is_refused():
    r = _driver(*ROWWISE, "--dense-embedding-update")
    assert r.returncode != 0
    assert "--adagrad-rowwise" in r.stderr and "--dense-embedding-update" in r.stderr, r.stderr[-2000:]
    assert "extension" not in r.stderr      # (before the library checks)


def test_both_forms_of_the_flag_reach_the_library_check():
    """--adagrad-rowwise and --adagrad-rowwise=1 parse; with every other refusal passed the oracle is refused for want of the extensions, in the
    wording of the Adagrad refusal (the element-wise one comes first: the dense slab needs it)."""
    for form in (["--adagrad-rowwise"], ["--adagrad-rowwise=1"]):
        r = _driver("--optimizer=adagrad", *form)
        assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
        assert "without the Adagrad extension" in r.stderr and "--backend" in r.stderr, r.stderr[-2000:]
    r = _driver("--adagrad-rowwise=0")      # the switch off: plain SGD trains
    assert r.returncode == 0 and "THROUGHPUT" in r.stdout, r.stderr[-2000:]
    r = _driver("--adagrad-rowwise=1")
    assert r.returncode != 0 and "--optimizer adagrad" in r.stderr


_REFUSAL = r"""
import sys
sys.path.insert(0, {tests!r})
import os
import dlrm_helpers as H
import adagrad_helpers as AH
from conftest import golden
case = {case!r}
comm, argv, hp = None, [], dict(lr=0.05, rowwise=True)
if case == "row_sharded":
    import torch.distributed as dist
    from dlrm_flexflow_amd.comm import TorchComm
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % (33400 + os.getpid() % 1000), rank=0, world_size=1)
    comm = TorchComm(on_gpu=False).struct
    argv = ["--force-exchange", "--row-shard-rows", "1"]
if case == "weight_decay":
    hp["weight_decay"] = 1e-3
if case == "weight_decay_sparse":
    hp["weight_decay"] = 1e-3
    argv = ["--sparse-embedding-optimizer"]
if case == "config_switch":
    hp.pop("rowwise")
    argv = ["--adagrad-rowwise"]
AH.build_dlrm(H.oracle_backend(), golden("dlrm_step_torch"), hp, argv=argv, comm=comm, dense_update=case in ("dense_update", "config_switch"))
print("COMPILED")
"""


@pytest.mark.parametrize("case,words", [
    ("row_sharded", ["is row-sharded", "--row-shard-rows", "--adagrad-rowwise"]),
    ("dense_update", ["--dense-embedding-update", "--adagrad-rowwise"]),
    ("config_switch", ["--dense-embedding-update", "--adagrad-rowwise"]),
    ("weight_decay", ["weight decay", "--sparse-embedding-optimizer", "--adagrad-rowwise"]),
])
def test_compile_refuses_what_the_row_rule_does_not_cover(case, words):
    """Through the FFModel API (AdagradOptimizer(rowwise=True), or the config's switch): each case dies in compile() with its reason and the flags
    to change, before the library checks (the oracle would otherwise be refused first for want of the extension)."""
    src = _REFUSAL.format(tests=os.path.join(ROOT, "tests"), case=case)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "COMPILED" not in r.stdout
    for word in words:
        assert word in r.stderr, (word, r.stderr[-2000:])
    assert "extension" not in r.stderr


def test_weight_decay_with_the_sparse_flag_passes_the_optimizer_checks():
    src = _REFUSAL.format(tests=os.path.join(ROOT, "tests"), case="weight_decay_sparse")
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "without the Adagrad extension" in r.stderr and "--sparse-embedding-optimizer" not in r.stderr, r.stderr[-2000:]


def test_sharded_and_replicated_tables_are_refused_in_a_two_rank_job(tmp_path):
    """--column-shard-rows and --replicate-embedding-rows place tables that way only with more than one rank: two driver ranks on the oracle
    (gloo), each refusal naming its flag."""
    import dlrm_helpers as H
    launcher = os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py")
    for flag, value, word in (("--column-shard-rows", "150", "is column-sharded"), ("--replicate-embedding-rows", "60", "is replicated"),
                              ("--row-shard-rows", "150", "is row-sharded")):
        r = subprocess.run([sys.executable, launcher, "-ll:gpu", "2", "--backend", H.oracle_backend(), *SMALL, *ROWWISE, flag, value],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
        assert word in r.stderr and flag in r.stderr and "--adagrad-rowwise" in r.stderr, (flag, r.stderr[-2000:])
        assert "extension" not in r.stderr
