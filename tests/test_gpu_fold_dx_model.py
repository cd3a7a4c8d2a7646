"""GPU tests (-m gpu) of the data-gradient fold in the host model: the `cat` DLRM of tests/fold_dw_helpers.py (D = 128, seven tables
of which three are folded, top 1024-256-64-1) at the smallest batch at which the kept data gradient is served (tests/fold_dx_helpers.py::model_batch).
The route on against --no-fold-dx -- the forward and weight-gradient folds on in both, so the first iteration's forward and dy are the same bits -- on
the weight deltas under the rule of tests/test_gpu_fold_dw_model.py (_delta_check, _compare: imported, not restated): after the warm-up iteration alone
no element excused, after three more steps at most 1 % of a tensor excused by a relu' flip.  The folded tables' deltas are the ones the route computes
another way (E -= lr G W_t instead of the sparse update of dx's columns); everything else must not notice.  The counters; the route off under
--deterministic, --no-overlap, momentum and bf16 tables; a replayed step against an eager one."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import fold_dw_helpers as DH
import fold_dx_helpers as XH
from test_gpu_fold_dw_model import _compare

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH


@pytest.fixture(scope="module")
def batch(hip):
    return XH.model_batch(hip.device_info().compute_units)


def test_route_on_against_no_fold_dx(hip, batch):
    on = XH.run_model(HIP, batch, [], snapshots=True)
    off = XH.run_model(HIP, batch, ["--no-fold-dx"], snapshots=True)
    assert on["counters"] == (3, 3, 3) and off["counters"] == (3, 3, 0)
    for k in on["w0"]:
        assert on["w0"][k].tobytes() == off["w0"][k].tobytes(), f"{k}: the two runs start from different weights"
    for nm, a in on["dy_warm"].items():
        assert a.tobytes() == off["dy_warm"][nm].tobytes(), f"{nm}: dy of the first iteration differs"
    # the warm-up iteration alone: the same forward and dy in both runs, so no relu' flip yet and no element excused
    worst = {}
    on_w = dict(on, masks=on["masks"][:1]); off_w = dict(off, masks=off["masks"][:1])
    _compare(on_w, off_w, batch, "w0", "w_warm", "_warm", 1, 0, worst)
    assert all(v[0] == 0 for v in worst.values()), f"warm-up iteration: elements beyond the bound: {worst}"
    print("warm-up iteration, per tensor (beyond the bound, unexplained, worst error / bound):", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:6]})
    # the kept columns of the data gradient are the plain call's bits, so after one iteration only the folded tables may differ at all
    folded = [f"{nm}/0" for t, nm in enumerate(n for n in on["names"] if n.startswith("Embedding")) if DH.MODEL_ROWS[t] <= 7420]
    assert len(folded) == 3
    for k in on["w_warm"]:
        if k not in folded and not k.startswith("Dense"):
            assert on["w_warm"][k].tobytes() == off["w_warm"][k].tobytes(), f"{k}: a table that is not folded differs after one iteration"
    for k in folded:
        assert np.abs(on["w_warm"][k].astype(np.float64) - on["w0"][k]).max() > 0, f"{k}: the folded table did not move"
    # three more steps, relu' flips from the two runs' own activations
    worst = {}
    _compare(on, off, batch, "w_warm", "w1", "", 3, 1, worst)
    np.testing.assert_allclose(on["pred"], off["pred"], rtol=2e-5, atol=2e-6)
    print("three steps, per tensor (beyond the bound, unexplained, worst error / bound):", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:6]})


@pytest.mark.parametrize("flags, expect", [(["--deterministic", "--no-trace"], (3, 0, 0)), (["--no-overlap"], (3, 3, 0)), (["--optimizer", "sgd-momentum"], (3, 3, 0)),
                                           (["--embedding-dtype", "bf16"], (0, 0, 0)), (["--no-fold-dw"], (3, 0, 0)), (["--no-fold-small-tables"], (0, 0, 0))],
                         ids=["deterministic", "no-overlap", "momentum", "bf16-tables", "no-fold-dw", "no-fold-small-tables"])
def test_route_off(hip, batch, flags, expect):
    assert XH.route_counters(HIP, batch, flags) == expect


def test_a_replayed_step_agrees_with_an_eager_one(hip, batch):
    eager = XH.run_model(HIP, batch, ["--no-trace"], snapshots=True)
    replay = XH.run_model(HIP, batch, ["--always-replay"], trace=True, snapshots=True)
    assert eager["counters"] == (3, 3, 3) and replay["counters"] == (3, 3, 3)
    assert replay["replays"] >= 2 and eager["replays"] == 0
    worst = {}
    _compare(replay, eager, batch, "w0", "w1", "", 4, 0, worst)
    np.testing.assert_allclose(replay["pred"], eager["pred"], rtol=2e-5, atol=2e-6)
