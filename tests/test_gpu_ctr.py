"""GPU tests (-m gpu) of the CTR extension (include/ff_hip_ctr.h): the kernels through the C-ABI against numpy / torch on the CPU, the
model with binary cross-entropy against torch, and evaluation between training steps."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import ctr_helpers as CH
import dlrm_helpers as H

pytestmark = pytest.mark.gpu

HIP = capi.HIP_LIB_PATH
DEV = "cuda"
K = capi.AUC_BINS
MATH_SPLIT_ALL = 3      # FFH_MATH_FP32_SPLIT_BF16X3_ALL (include/ff_hip.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def ctr(hip):
    return capi.ctr_api(hip)


def _probabilities(rng, n, nc=1):
    p = rng.uniform(0.001, 0.999, (n, nc)).astype(np.float32)
    y = (rng.uniform(0, 1, (n, nc)) > 0.5).astype(np.float32)
    soft = rng.uniform(0, 1, (n, nc)) < 0.2
    y[soft] = rng.uniform(0, 1, int(soft.sum())).astype(np.float32)
    k = min(n, 8)                                                   # exact 0 and 1 against labels 0, 1 and soft labels
    p.ravel()[:k] = np.array([0, 0, 0, 1, 1, 1, 0, 1], np.float32)[:k]
    y.ravel()[:k] = np.array([0, 1, 0.25, 0, 1, 0.75, 0.5, 0.5], np.float32)[:k]
    return p, y


# ---- 4. kernels through the C-ABI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,NC", [(1, 1), (37, 1), (4099, 1), (32768, 1), (777, 3)])
def test_bce_bwd_metrics_gradient_and_logloss(hip, ctr, B, NC):
    """dz bit-identical to fp32 numpy (p - y) * scale; the log-loss sum against float64 (and torch's binary_cross_entropy on the CPU)
    within 1e-5 relative, the bound of the MSE-sum tests; the other sums and counts as ffh_metrics_update leaves them."""
    rng = np.random.default_rng(B + NC)
    p, y = _probabilities(rng, B, NC)
    scale = np.float32(1.0 / B)
    mf = capi.METRIC_ACCURACY | capi.METRIC_MSE | capi.METRIC_BCE
    dz = torch.full((B, NC), 9.0, dtype=torch.float32, device=DEV)
    perf = torch.zeros(8, dtype=torch.int32, device=DEV)
    perf2 = torch.zeros(8, dtype=torch.int32, device=DEV)
    bsum = torch.zeros(1, dtype=torch.float32, device=DEV)
    ctr.call("ffh_bce_bwd_metrics", dz, dev(p), dev(y), perf, bsum, B, NC, float(scale), mf, None)
    hip.call("ffh_metrics_update", dev(p), dev(y), perf2, B, NC, capi.METRIC_ACCURACY | capi.METRIC_MSE, None)
    assert bits_equal(host(dz), ((p - y) * scale).astype(np.float32))
    want = float(CH.bce_f64(p, y).sum())
    tor = float(torch.nn.functional.binary_cross_entropy(torch.from_numpy(p), torch.from_numpy(y), reduction="sum").double())
    got = float(host(bsum)[0])
    print(f"B={B} NC={NC}: logloss sum gpu {got:.6f} float64 {want:.6f} torch {tor:.6f}")
    assert abs(tor - want) <= 1e-5 * want
    assert abs(got - want) <= 1e-5 * want
    a, b = host(perf), host(perf2)
    assert a[:2].tolist() == b[:2].tolist()
    if NC == 1:
        assert a[:2].tolist() == [2 * B, B]                         # train_all double count (1 class + accuracy)
    np.testing.assert_allclose(a[4:5].view(np.float32), b[4:5].view(np.float32), rtol=1e-5)


@pytest.mark.parametrize("mode", [0, MATH_SPLIT_ALL], ids=["fp32", "split"])
@pytest.mark.parametrize("B,IN,OUT", [(2048, 256, 1), (100, 64, 3), (777, 1024, 4), (8192, 256, 1)])
def test_linear_bwd_bce_equals_the_two_calls(hip, ctr, mode, B, IN, OUT):
    """ffh_linear_bwd_bce against ffh_bce_bwd_metrics followed by ffh_linear_bwd_ex(FFH_LINEAR_DY_PREMASKED), at the relation
    test_gpu_parity.py::test_linear_bwd_mse_equals_the_two_calls asserts for the MSE form: dy and dX bit-exact, dW / db / the sums within 1e-5
    (atomics); in the exact and in the split math mode; unsupported forms return FFH_ERR_UNSUPPORTED with the output buffers untouched."""
    act = capi.AC_MODE_SIGMOID
    rng = np.random.default_rng(B + OUT)
    x = rng.uniform(-1, 1, (B, IN)).astype(np.float32)
    w = rng.uniform(-1, 1, (OUT, IN)).astype(np.float32)
    y = rng.uniform(0.05, 0.95, (B, OUT)).astype(np.float32)
    label = (rng.uniform(0, 1, (B, OUT)) > 0.5).astype(np.float32)
    flags = capi.LINEAR_DX_OVERWRITE | capi.LINEAR_DX_MASK_BY_X
    mf = capi.METRIC_ACCURACY | capi.METRIC_MSE | capi.METRIC_BCE
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, mode) == 0
    try:
        res = []
        for fused in (True, False):
            dx = torch.full((B, IN), 3.0, dtype=torch.float32, device=DEV)
            dy = torch.full((B, OUT), 9.0, dtype=torch.float32, device=DEV)
            dw, db = torch.zeros(OUT, IN, device=DEV), torch.zeros(OUT, device=DEV)
            perf = torch.zeros(8, dtype=torch.int32, device=DEV)
            bsum = torch.zeros(1, dtype=torch.float32, device=DEV)
            if fused:
                ctr.call("ffh_linear_bwd_bce", dev(x), IN, dx, IN, dev(y), OUT, dy, OUT, dev(w), dw, db, IN, OUT, B, act, flags,
                         dev(label), 1.0 / B, perf, bsum, mf, None)
            else:
                ctr.call("ffh_bce_bwd_metrics", dy, dev(y), dev(label), perf, bsum, B, OUT, 1.0 / B, mf, None)
                hip.call("ffh_linear_bwd_ex", dev(x), IN, dx, IN, dev(y), OUT, dy, OUT, dev(w), dw, db, IN, OUT, B, act,
                         flags | capi.LINEAR_DY_PREMASKED, None, None)
            res.append([host(t) for t in (dx, dy, dw, db, perf, bsum)])
        f, t = res
        assert bits_equal(f[0], t[0]) and bits_equal(f[1], t[1])
        np.testing.assert_allclose(f[2], t[2], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(f[3], t[3], rtol=1e-5, atol=1e-6)
        assert f[4][:2].tolist() == t[4][:2].tolist()
        np.testing.assert_allclose(f[4][4:5].view(np.float32), t[4][4:5].view(np.float32), rtol=1e-5)
        np.testing.assert_allclose(f[5], t[5], rtol=1e-5)
        # against numpy: dz = (p - label) / B, no sigmoid derivative; db its column sums; dW = dz^T x
        dz = ((y - label) * np.float32(1.0 / B)).astype(np.float32)
        assert bits_equal(f[1], dz)
        np.testing.assert_allclose(f[3], dz.astype(np.float64).sum(0), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(f[2], dz.astype(np.float64).T @ x.astype(np.float64), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(f[5][0], CH.bce_f64(y, label).sum(), rtol=1e-5)
        # what the launch does not serve: FFH_ERR_UNSUPPORTED, nothing launched, the caller makes the two calls
        dx = torch.full((B, IN), 3.0, dtype=torch.float32, device=DEV)
        dy = torch.full((B, OUT), 9.0, dtype=torch.float32, device=DEV)
        dw, db = torch.full((OUT, IN), 5.0, device=DEV), torch.full((OUT,), 6.0, device=DEV)
        perf = torch.zeros(8, dtype=torch.int32, device=DEV)
        bsum = torch.zeros(1, dtype=torch.float32, device=DEV)
        for bad_flags in (capi.LINEAR_ONLY_DX, capi.LINEAR_ONLY_DW, capi.LINEAR_DY_PREMASKED):
            rc = ctr.rc("ffh_linear_bwd_bce", dev(x), IN, dx, IN, dev(y), OUT, dy, OUT, dev(w), dw, db, IN, OUT, B, act, bad_flags,
                        dev(label), 1.0 / B, perf, bsum, mf, None)
            assert rc == capi.FFH_ERR_UNSUPPORTED
        assert (host(dx) == 3).all() and (host(dy) == 9).all() and (host(dw) == 5).all() and (host(db) == 6).all()
        assert not host(perf).any() and host(bsum)[0] == 0
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0


def test_linear_bwd_bce_refuses_shapes_the_launch_does_not_serve(hip, ctr):
    B = 64
    for IN, OUT in ((256, 5), (2048, 1), (250, 1)):                 # more than 4 outputs; in_dim above 1024; in_dim not a multiple of 4
        x, w = torch.zeros(B, IN, device=DEV), torch.zeros(OUT, IN, device=DEV)
        y, label = torch.full((B, OUT), 0.5, device=DEV), torch.zeros(B, OUT, device=DEV)
        dx, dy = torch.full((B, IN), 3.0, device=DEV), torch.full((B, OUT), 9.0, device=DEV)
        dw, db = torch.full((OUT, IN), 5.0, device=DEV), torch.full((OUT,), 6.0, device=DEV)
        perf = torch.zeros(8, dtype=torch.int32, device=DEV)
        bsum = torch.zeros(1, dtype=torch.float32, device=DEV)
        rc = ctr.rc("ffh_linear_bwd_bce", x, IN, dx, IN, y, OUT, dy, OUT, w, dw, db, IN, OUT, B, capi.AC_MODE_SIGMOID, 0, label, 1.0 / B,
                    perf, bsum, capi.METRIC_BCE, None)
        assert rc == capi.FFH_ERR_UNSUPPORTED, (IN, OUT)
        assert (host(dx) == 3).all() and (host(dy) == 9).all() and (host(dw) == 5).all() and (host(db) == 6).all() and host(bsum)[0] == 0
    rc = ctr.rc("ffh_linear_bwd_bce", x, IN, dx, IN, y, OUT, dy, OUT, w, dw, db, IN, OUT, B, capi.AC_MODE_RELU, 0, label, 1.0 / B, perf, bsum, 0, None)
    assert rc == capi.FFH_ERR_BAD_ARG                               # the loss is defined on a sigmoid output


def _eval_buffer():
    return torch.zeros(ctypes.sizeof(capi.CtrEval) // 8, dtype=torch.int64, device=DEV)


def _read_eval(buf):
    raw = host(buf).tobytes()
    return capi.CtrEval.from_buffer_copy(raw)


@pytest.mark.parametrize("B", [1, 37, 2048, 32768])
def test_ctr_eval_update_counts_and_histograms_are_exact(hip, ctr, B):
    """Histograms, counts and the NaN count equal to numpy exactly, accumulated over several calls, and equal between two different batch
    splits of the same data (integer atomics only)."""
    rng = np.random.default_rng(B)
    calls = 3
    n = B * calls
    p = (1.0 / (1.0 + np.exp(-rng.normal(-1.5, 1.5, n)))).astype(np.float32)      # CTR-like: many samples in a few hundred bins
    y = (rng.uniform(0, 1, n) < p).astype(np.float32)
    y[rng.uniform(0, 1, n) < 0.1] = 0.5                                           # soft labels on the threshold: positives
    special = np.array([0.0, 1.0, np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0 / K, np.nan], np.float32)
    idx = rng.choice(n, size=min(n, len(special)), replace=False)
    p[idx] = special[:len(idx)]
    dp, dy_ = dev(p), dev(y)
    bufs = []
    for split in (B, max(1, (B * 2) // 3 + 1)):
        buf = _eval_buffer()
        for i in range(0, n, split):
            m = min(split, n - i)
            ctr.call("ffh_ctr_eval_update", dp[i:i + m], dy_[i:i + m], buf, m, None)
        bufs.append(_read_eval(buf))
    e, e2 = bufs
    ok = ~np.isnan(p)
    hp, hn = CH.histograms(p, y)
    assert e.samples == int(ok.sum()) and e.nan_predictions == int((~ok).sum())
    assert e.positives == int((y[ok] >= 0.5).sum())
    assert e.correct == int(((p[ok] >= 0.5) == (y[ok] >= 0.5)).sum())
    assert np.array_equal(np.ctypeslib.as_array(e.hist_pos), hp) and np.array_equal(np.ctypeslib.as_array(e.hist_neg), hn)
    want = float(CH.bce_f64(p[ok], y[ok]).sum())
    assert abs(e.logloss_sum - want) <= 1e-5 * want
    for f in ("samples", "positives", "correct", "nan_predictions"):
        assert getattr(e, f) == getattr(e2, f)
    assert bytes(e.hist_pos) == bytes(e2.hist_pos) and bytes(e.hist_neg) == bytes(e2.hist_neg)
    assert abs(e2.logloss_sum - want) <= 1e-5 * want
    if e.positives and e.positives != e.samples:
        assert ffmodel.auc_from_histograms(hp, hn) == CH.auc_formula(hp, hn) or abs(ffmodel.auc_from_histograms(hp, hn) - CH.auc_formula(hp, hn)) < 1e-12


# ---- 5. the model against torch on the CPU ---------------------------------------------------------------------------------------------
def _records_close(a, b, keys=None):
    for step in range(len(a)):
        for k in (keys or a[step]):
            if k == "bce_sum":
                continue
            np.testing.assert_allclose(a[step][k], b[step][k], rtol=1e-5, atol=1e-6, err_msg=f"step {step} {k}")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replayed"])
def test_bce_model_matches_torch(hip, graph):
    """The golden DLRM with LOSS_BCE, four SGD steps, against torch on the CPU at the tolerance of the MSE torch step (1e-5 / 1e-6); the fused
    loss + last layer launch and --no-fused-loss agree at the relation of the kernel test (predictions and parameters within 1e-5)."""
    steps = 4
    recs = {}
    for name, extra in (("fused", []), ("unfused", ["--no-fused-loss"])):
        m, h = CH.build_bce_dlrm(HIP, enable_graph=graph, extra_argv=extra)
        recs[name] = H.run_steps(m, h, steps, trace=graph)
        assert m.uses_graph == graph
        # the route: the fused leg really took ffh_linear_bwd_bce (every eager backward; a replayed step calls it once, at the capture)
        calls = m.counter("fused_loss_calls")
        assert calls == (0 if extra else (1 if graph else steps)), (name, calls)
        exp = CH.torch_bce_sgd_reference(h["g"], steps)
        _records_close(recs[name], exp, keys=list(recs[name][0]))
        pm = m.perf_metrics()
        want = sum(e["bce_sum"] for e in exp)
        got = m.bce_loss()
        print(f"{name} graph={graph}: bce sum {got:.6f} torch {want:.6f}")
        assert abs(got - want) <= 1e-5 * want and pm.train_all == 2 * steps * int(h["g"]["B"])
        m.close()
    _records_close(recs["fused"], recs["unfused"])
    # the loss moves the model away from the MSE trajectory (the golden file's): the two losses are not the same step
    g = h["g"]
    assert not np.allclose(recs["fused"][1]["top.0.weight"], g["step1/top.0.weight"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("flags,exact", [(["--profiling"], True), (["--fp32-split-bf16x3"], True), (["--allow-tensor-op-math-conversion"], False),
                                         (["--embedding-dtype", "bf16"], False), (["--embedding-dtype", "bf16", "--no-fused-loss"], False)])
def test_bce_model_in_the_other_modes(hip, flags, exact):
    """--loss bce with --profiling, the two bf16-pipe math modes and bf16 tables (training, not --deterministic): four steps against torch.
    The fp32-accurate forms at the 1e-5 / 1e-6 of the plain run; the forms that round to bf16 (operands: 2^-9 relative each, include/ff_hip.h;
    table rows: 2^-9 of a row after every update) at 2e-2 absolute on the probabilities, with a log-loss that falls."""
    steps = 4
    m, h = CH.build_bce_dlrm(HIP, extra_argv=flags)
    sums = []
    recs = []
    for _ in range(steps):
        m.reset_metrics()
        recs += H.run_steps(m, h, 1)
        sums.append(m.bce_loss())
    exp = CH.torch_bce_sgd_reference(h["g"], steps)
    if exact:
        _records_close(recs, exp, keys=list(recs[0]))
    else:
        for step in range(steps):
            assert np.isfinite(recs[step]["pred"]).all()
            np.testing.assert_allclose(recs[step]["pred"], exp[step]["pred"], rtol=0, atol=2e-2, err_msg=f"step {step}")
    print(f"{flags}: log-loss sums {sums} torch {[e['bce_sum'] for e in exp]}")
    assert all(b < a for a, b in zip(sums, sums[1:]))
    if "--profiling" not in flags and "--no-fused-loss" not in flags:
        assert m.counter("fused_loss_calls") == steps
    m.close()


_REFUSAL = r"""
import sys
sys.path.insert(0, {tests!r})
from dlrm_flexflow_amd import capi, ffmodel
case = {case!r}
cfg = ffmodel.FFConfig(argv=["-b", "16"], backend=capi.HIP_LIB_PATH)
m = ffmodel.FFModel(cfg)
x = m.create_tensor([16, 8], ffmodel.DT_FLOAT)
m.dense(m.dense(x, 4, capi.AC_MODE_RELU), 1, capi.AC_MODE_SIGMOID)
m.set_sgd_optimizer(lr=0.01)
if case == "auc_without_eval":
    m.compile(ffmodel.LOSS_BCE, (ffmodel.METRICS_ACCURACY, ffmodel.METRICS_BCE, ffmodel.METRICS_AUC))
elif case == "bce_metric_with_mse":
    m.compile(ffmodel.LOSS_MSE_AVG, (ffmodel.METRICS_ACCURACY, ffmodel.METRICS_BCE))
elif case == "auc_in_inference":
    m.compile(ffmodel.LOSS_BCE, (ffmodel.METRICS_AUC,), ffmodel.COMP_MODE_INFERENCE)
print("COMPILED")
"""


@pytest.mark.parametrize("case,message", [("auc_without_eval", "METRICS_AUC in a training compile() needs held-out data to evaluate: set --eval-batches"),
                                          ("bce_metric_with_mse", "METRICS_BINARY_CROSSENTROPY is accumulated by the loss step of --loss bce"),
                                          ("auc_in_inference", None)])
def test_compile_refusals_behind_the_library_check(hip, case, message):
    """On a library WITH the extension: METRICS_AUC in a training compile() without --eval-batches and METRICS_BINARY_CROSSENTROPY without
    the loss die naming what to change; METRICS_AUC in an inference compile() is accepted."""
    import sys
    src = _REFUSAL.format(tests=os.path.join(ROOT, "tests"), case=case)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300, cwd=ROOT)
    if message is None:
        assert r.returncode == 0 and "COMPILED" in r.stdout, r.stderr[-2000:]
    else:
        assert r.returncode != 0 and "COMPILED" not in r.stdout
        assert message in r.stderr, r.stderr[-2000:]


# ---- 6. evaluation does not disturb training -------------------------------------------------------------------------------------------
def _params(m, h):
    out = {}
    for k, li in h["names"].items():
        out[f"{k}.weight"] = m.parameter(li, 0).get_weights()
        if not k.startswith("emb"):
            out[f"{k}.bias"] = m.parameter(li, 1).get_weights()
    return out


def _set_inputs(m, g, dense, label, sparse_ids, rng=None):
    """golden inputs, or (rng given) another batch of the same shapes"""
    B = int(g["B"])
    d, lab = g["dense"], g["label"]
    ids = [g[f"sparse{t}"] for t in range(len(sparse_ids))]
    if rng is not None:
        d = rng.uniform(0, 1, d.shape).astype(np.float32)
        lab = (rng.uniform(0, 1, lab.shape) > 0.5).astype(np.float32)
        ids = [rng.integers(0, int(r), i.shape).astype(np.int64) for r, i in zip(g["rows"], ids)]
    dense.set(d); label.set(lab)
    for s, i in zip(sparse_ids, ids):
        s.set(i)
    return B


def _build_with_inputs(extra, graph):
    """build_golden_dlrm keeps its input tensors to itself: they are the model's first tensors, so they are rebuilt here through the same
    calls in the same order and found again as the tensors H wrote (the label tensor is public)."""
    created = []
    orig = ffmodel.FFModel.create_tensor

    def spy(self, *a, **k):
        t = orig(self, *a, **k)
        created.append(t)
        return t
    ffmodel.FFModel.create_tensor = spy
    try:
        m, h = CH.build_bce_dlrm(HIP, enable_graph=graph, extra_argv=["--deterministic"] + extra)
    finally:
        ffmodel.FFModel.create_tensor = orig
    n = len(h["g"]["rows"])
    return m, h, created[:n], created[n]


@pytest.mark.parametrize("variant,extra,graph", [("eager", [], False), ("early_sort", ["--early-sort"], False), ("replayed", [], True),
                                                  ("bf16_tables", ["--embedding-dtype", "bf16"], False)])
def test_eval_batches_between_steps_leave_training_bit_identical(hip, variant, extra, graph):
    """--deterministic: run A trains 6 steps; run B trains the same 6 steps with two eval_batch() calls on other inputs after steps 2 and 4.
    All parameters and table rows -- and with bf16 tables and stochastic rounding the update counter -- are bit-identical; parameters are
    bit-unchanged across an eval_batch()."""
    final = {}
    for run in ("A", "B"):
        m, h, sparse, dense = _build_with_inputs(extra, graph)
        g = h["g"]
        rng = np.random.default_rng(11)
        for step in range(6):
            if graph:
                m.begin_trace(7)
            m.forward(); m.zero_gradients(); m.backward(); m.update()
            if graph:
                m.end_trace(7)
            if run == "B" and step in (1, 3):
                m.sync()
                before = _params(m, h)
                _set_inputs(m, g, dense, m.label_tensor, sparse, rng)
                m.eval_batch()
                m.sync()
                after = _params(m, h)
                for k in before:
                    assert bits_equal(before[k], after[k]), k
                _set_inputs(m, g, dense, m.label_tensor, sparse)
        m.sync()
        final[run] = _params(m, h)
        final[run + "_counter"] = m.counter("bf16_updates")
        if run == "B":
            e = m.eval_metrics(histograms=True)
            assert e["samples"] == 2 * int(g["B"]) and e["nan_predictions"] == 0
            assert int(e["hist_pos"].sum() + e["hist_neg"].sum()) == e["samples"] and int(e["hist_pos"].sum()) == e["positives"]
            assert e["auc"] == ffmodel.auc_from_histograms(e["hist_pos"], e["hist_neg"])
            m.reset_eval_metrics()
            assert m.eval_metrics()["samples"] == 0
        m.close()
    for k in final["A"]:
        assert bits_equal(final["A"][k], final["B"][k]), f"{variant}: {k}"
    assert final["A_counter"] == final["B_counter"]
    if variant == "bf16_tables":
        assert final["A_counter"] == 6


# ---- 9. the driver ---------------------------------------------------------------------------------------------------------------------
DRIVER = ["-ll:gpu", "1", "-b", "128", "--arch-sparse-feature-size", "16", "--arch-embedding-size", "-".join(["1000"] * 8),
          "--arch-mlp-bot", "13-64-16", "--arch-mlp-top", "144-64-1", "--data-size", "1536", "--loss", "bce", "--eval-batches", "4", "--deterministic"]
EVAL_LINE = re.compile(r"^EVAL epoch (\d+): samples (\d+) logloss ([\d.]+) accuracy ([\d.]+) auc ([\d.]+|nan) time [\d.]+s$", re.M)


def test_driver_prints_eval_lines_equal_to_python(hip):
    exe = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
    r = subprocess.run([exe, *DRIVER, "--epochs", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = EVAL_LINE.findall(r.stdout)
    assert [l[0] for l in lines] == ["1", "2"] and all(l[1] == "512" for l in lines), r.stdout[-2000:]
    assert "[DLRM] loss: bce" in r.stdout and "THROUGHPUT" in r.stdout and "binary_crossentropy" in r.stderr
    assert "Num. iterations/epoch = 8" in r.stdout
    # the same two epochs through Python, step for step as DLRMApp::run_epochs issues them (--deterministic: the same bits run to run)
    app = ffmodel.DLRM(DRIVER + ["--epochs", "2"])
    app.warmup()
    app.model.set_trace_mode(0)
    for epoch in range(2):
        app.model.reset_metrics()
        app.train_steps(8, trace=epoch > 0)
        e = app.evaluate(epoch + 1)
        assert lines[epoch][1:] == (str(e["samples"]), f"{e['logloss']:.4f}", f"{e['accuracy']:.4f}", f"{e['auc']:.4f}"), (epoch, lines[epoch], e)
    app.close()
    assert lines[0][2:] != lines[1][2:]                             # training between the two evaluations moved the figures
    r = subprocess.run([exe, *DRIVER, "--eval-only"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = EVAL_LINE.findall(r.stdout)
    assert len(lines) == 1 and lines[0][0] == "0"
    # the same evaluation through Python: the same seeded model, no training
    app = ffmodel.DLRM(DRIVER + ["--eval-only"])
    e = app.evaluate(0)
    app.close()
    assert int(lines[0][1]) == e["samples"] == 512
    assert lines[0][2] == f"{e['logloss']:.4f}" and lines[0][3] == f"{e['accuracy']:.4f}" and lines[0][4] == f"{e['auc']:.4f}"


# ---- 8. learning ---------------------------------------------------------------------------------------------------------------------
LEARN_STEPS, LEARN_BATCH, LEARN_TRAIN_BATCHES, LEARN_EVAL_BATCHES = 300, 2048, 50, 8
# Held-out AUC (8 batches, 16384 samples) before / after LEARN_STEPS steps of --loss bce on the Kaggle shape with --synthetic-labels
# logistic, seeds 1, 2, 3, measured on one MI355X: 0.4911 -> 0.5192, 0.4909 -> 0.5531, 0.4992 -> 0.5287 (log-loss 0.78 -> 0.693,
# 0.96 -> 0.691, 0.74 -> 0.692).  The smallest gain is 0.0281; the test asserts half of it.  (The standard error of an AUC near 0.5 on 16384
# samples is about sqrt((1 / P + 1 / N) / 12) = 0.0045.)
LEARN_MIN_GAIN = 0.014


def _learning_run(seed):
    args = H.KAGGLE_ARGS(LEARN_BATCH)
    args[args.index("--data-size") + 1] = str(LEARN_BATCH * (LEARN_TRAIN_BATCHES + LEARN_EVAL_BATCHES))
    app = ffmodel.DLRM(args + ["--device", "0", "--loss", "bce", "--synthetic-labels", "logistic", "--eval-batches", str(LEARN_EVAL_BATCHES),
                               "--seed", str(seed)])
    before = app.evaluate(0)
    app.warmup()
    app.train_steps(LEARN_STEPS, trace=False)
    after = app.evaluate(1)
    app.close()
    return before, after


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bce_training_raises_the_held_out_auc(hip, seed):
    before, after = _learning_run(seed)
    print(f"LEARN seed {seed}: auc before {before['auc']:.4f} after {after['auc']:.4f} gain {after['auc'] - before['auc']:.4f} "
          f"logloss before {before['logloss']:.4f} after {after['logloss']:.4f}")
    assert before["samples"] == after["samples"] == LEARN_BATCH * LEARN_EVAL_BATCHES
    assert after["auc"] - before["auc"] >= LEARN_MIN_GAIN
    assert after["logloss"] < before["logloss"]
