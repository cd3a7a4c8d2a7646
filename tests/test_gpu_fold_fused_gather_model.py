"""GPU tests (-m gpu) of the fold's forward with the gather-add inside the first top GEMM's epilogue ("The gather in the epilogue")
against the three launches of before (--no-fold-fused-gather): the same arithmetic in the same order, so under --deterministic every parameter and the
predictions agree to the bit, and without it -- where the weight gradients meet by float atomics -- within rtol 2e-5, atol 2e-6.

The model is the `cat` DLRM of tests/fold_dw_helpers.py (seven tables of which three are folded, top 1024-256-64-1).  The smallest model of
tests/fold_helpers.py (batch 512, top 224-128-64-1) folds its tables on the plain MFMA kernel, four output tiles, and never reaches the persistent
kernel whose epilogue this is; the batch here is the smallest at which the first top layer's forward is one whole round of 128 x 128 tiles."""
import functools

import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import fold_dw_helpers as DH
import fold_helpers as FH

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
STEPS = 3
OFF = "--no-fold-fused-gather"


def model_batch(compute_units):
    """The smallest multiple of 128 at which the 2 column tiles of the first top layer's output fill whole rounds of one workgroup per CU (at least one
    round, the last one 80 % full): the rule ffh_fold_linear_fwd_plan restates from the persistent kernel's plan."""
    g = compute_units & ~7
    b = 128
    while True:
        tiles = (DH.MODEL_OUT // 128) * (b // 128)
        if tiles >= g and tiles * 100 >= -(-tiles // g) * g * 80:
            return b
        b += 128


@functools.lru_cache(maxsize=None)
def _run(cu, flags, trace=False):
    app = ffmodel.DLRM(["--backend", HIP, "--lr", str(DH.LR)] + DH.model_args(model_batch(cu), list(flags)))
    m = app.model
    rec = {"folded": m.counter("folded_tables")}
    app.warmup()
    m.sync()
    rec["fused_warm"] = m.counter("fold_fused_gather_steps")
    app.train_steps(STEPS, trace=trace)
    m.sync()
    rec["fused"] = m.counter("fold_fused_gather_steps") - rec["fused_warm"]
    rec["replays"] = m.counter("graph_replays")
    rec["w"] = FH.weights_of(m)
    rec["pred"] = m.layer_output(m.num_layers - 1).get()
    app.close()
    for a in list(rec["w"].values()) + [rec["pred"]]:
        a.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def cu(hip):
    return hip.device_info().compute_units


def test_deterministic_runs_agree_to_the_bit(cu):
    on, off = _run(cu, ("--deterministic", "--no-trace")), _run(cu, ("--deterministic", "--no-trace", OFF))
    assert on["folded"] > 0 and off["folded"] == on["folded"]
    assert on["fused_warm"] >= 1 and on["fused"] == STEPS and off["fused_warm"] == 0 and off["fused"] == 0
    for k in on["w"]:
        assert on["w"][k].tobytes() == off["w"][k].tobytes(), f"{k} differs"
    assert on["pred"].tobytes() == off["pred"].tobytes()


def _close(a, b):
    worst = 0.0
    for k in a["w"]:
        x, y = a["w"][k].astype(np.float64), b["w"][k].astype(np.float64)
        worst = max(worst, float((np.abs(x - y) / (2e-6 + 2e-5 * np.abs(y))).max()))
    print(f"worst |difference| / tolerance over the parameters: {worst:.4f}")
    for k in a["w"]:
        np.testing.assert_allclose(a["w"][k], b["w"][k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(a["pred"], b["pred"], rtol=2e-5, atol=2e-6)


def test_default_runs_agree_within_the_tolerance(cu):
    on, off = _run(cu, ("--no-trace",)), _run(cu, ("--no-trace", OFF))
    assert on["folded"] > 0 and on["fused"] == STEPS and off["fused"] == 0 and off["fused_warm"] == 0
    _close(on, off)


def test_replayed_steps_agree(cu):
    on, off = _run(cu, ("--always-replay",), True), _run(cu, ("--always-replay", OFF), True)
    assert on["replays"] >= 2 and off["replays"] >= 2
    assert on["fused_warm"] >= 1 and off["fused_warm"] == 0 and off["fused"] == 0
    _close(on, off)
    _close(on, _run(cu, ("--no-trace",)))
