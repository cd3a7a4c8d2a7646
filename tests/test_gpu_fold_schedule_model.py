"""GPU tests (-m gpu) of the order in which the fold's backward is issued ("The schedule"): the kept-tile weight-gradient GEMM on the
compute stream behind the backward of the layers below instead of behind the segmented sum and the products (--fold-dw-behind-sum restores that), and the sparse
update of the tables that are not dx-folded started at "gradients ready" instead of behind the products (--fold-update-behind-products restores that).
No arithmetic changes, so every comparison is between two orders of the same launches on the `cat` DLRM of tests/fold_dw_helpers.py (seven tables of
which three are folded, top 1024-256-64-1) at tests/fold_dx_helpers.py::model_batch, under the rules of tests/test_gpu_fold_dw_model.py::_compare
(imported): the tables bit for bit after the warm-up iteration (G in the canonical order, the dense update one fixed chain, the kept dx the plain call's
bits), the dense tensors -- whose weight gradients meet by float atomics -- within 1e-5 of the term mass with no element excused after one iteration and
at most 1 % excused by a relu' flip after three more.  A missing edge shows here only if the race shows at this size; the table of edges in DESIGN is the
other half."""
import functools

import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import fold_dw_helpers as DH
import fold_dx_helpers as XH
from test_gpu_fold_dw_model import _compare

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
OLD = ["--fold-dw-behind-sum", "--fold-update-behind-products"]


@pytest.fixture(scope="module")
def batch(hip):
    return XH.model_batch(hip.device_info().compute_units)


@functools.lru_cache(maxsize=None)
def _run(batch, flags):
    """One run per (batch, flags) for the whole module; the arrays are read-only so that no test changes what another one compares against."""
    rec = XH.run_model(HIP, batch, list(flags), snapshots=True)
    for v in rec.values():
        for a in (v.values() if isinstance(v, dict) else v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return rec


def _tables(rec):
    return [f"{n}/0" for n in rec["names"] if n.startswith("Embedding")]


def _same_order_rule(a, b, batch, tables_exact=True):
    """`a` and `b` run the same launches in two orders."""
    for k in a["w0"]:
        assert a["w0"][k].tobytes() == b["w0"][k].tobytes(), f"{k}: the two runs start from different weights"
    for nm, g in a["dy_warm"].items():
        assert g.tobytes() == b["dy_warm"][nm].tobytes(), f"{nm}: dy of the first iteration differs"
    if tables_exact:
        assert len(_tables(a)) == len(DH.MODEL_ROWS)
        for k in _tables(a):
            assert a["w_warm"][k].tobytes() == b["w_warm"][k].tobytes(), f"{k}: the table differs after one iteration"
            assert np.abs(a["w_warm"][k].astype(np.float64) - a["w0"][k]).max() > 0, f"{k}: the table did not move"
    worst = {}
    a_w = dict(a, masks=a["masks"][:1]); b_w = dict(b, masks=b["masks"][:1])
    _compare(a_w, b_w, batch, "w0", "w_warm", "_warm", 1, 0, worst)
    assert all(v[0] == 0 for v in worst.values()), f"warm-up iteration: elements beyond the bound: {worst}"
    print("warm-up iteration, per tensor (beyond the bound, unexplained, worst error / bound):", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:6]})
    worst = {}
    _compare(a, b, batch, "w_warm", "w1", "", 3, 1, worst)
    np.testing.assert_allclose(a["pred"], b["pred"], rtol=2e-5, atol=2e-6)
    print("three steps, per tensor (beyond the bound, unexplained, worst error / bound):", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:6]})


def test_new_order_against_the_order_of_before(hip, batch):
    new, old = _run(batch, ()), _run(batch, tuple(OLD))
    assert new["counters"] == (3, 3, 3) and old["counters"] == (3, 3, 3)
    _same_order_rule(new, old, batch)


@pytest.mark.parametrize("flag", OLD, ids=["dw-behind-sum", "update-behind-products"])
def test_each_switch_alone_against_both(hip, batch, flag):
    one, old = _run(batch, (flag,)), _run(batch, tuple(OLD))
    assert one["counters"] == (3, 3, 3)
    _same_order_rule(one, old, batch)


def test_a_replayed_step_agrees_with_an_eager_one_in_the_new_order(hip, batch):
    eager = _run(batch, ("--no-trace",))
    replay = XH.run_model(HIP, batch, ["--always-replay"], trace=True, snapshots=True)
    assert eager["counters"] == (3, 3, 3) and replay["counters"] == (3, 3, 3)
    assert replay["replays"] >= 2 and eager["replays"] == 0
    worst = {}
    _compare(replay, eager, batch, "w0", "w1", "", 4, 0, worst)
    np.testing.assert_allclose(replay["pred"], eager["pred"], rtol=2e-5, atol=2e-6)


def test_without_the_dx_fold_the_update_still_waits_for_the_products(hip, batch):
    """--no-fold-dx: the sparse update covers the folded tables, whose rows the products read -- it must stay behind ev_fold_e_read; only the GEMM moves."""
    new, old = _run(batch, ("--no-fold-dx",)), _run(batch, ("--no-fold-dx", "--fold-dw-behind-sum"))
    assert new["counters"] == (3, 3, 0) and old["counters"] == (3, 3, 0)
    _same_order_rule(new, old, batch)


@pytest.mark.parametrize("flags, expect", [(("--serial-dw",), (3, 3, 3)), (("--no-overlap",), (3, 3, 0)), (("--deterministic", "--no-trace"), (3, 0, 0))],
                         ids=["serial-dw", "no-overlap", "deterministic"])
def test_configurations_that_keep_their_launches(hip, batch, flags, expect):
    """Outside the route (weight gradient forked, table update on the side stream) the switches change nothing."""
    a, b = _run(batch, flags), _run(batch, flags + tuple(OLD))
    assert a["counters"] == expect and b["counters"] == expect
    if "--deterministic" in flags:
        for k in a["w1"]:
            assert a["w1"][k].tobytes() == b["w1"][k].tobytes(), f"{k}: --deterministic differs with the switches set"
        assert a["pred"].tobytes() == b["pred"].tobytes()
    else:
        _same_order_rule(a, b, batch)


@pytest.mark.parametrize("flags, expect", [((), (True, True)), (("--fold-dw-behind-sum",), (False, True)), (("--fold-update-behind-products",), (True, False)),
                                           (tuple(OLD), (False, False)), (("--no-fold-dx",), (True, False)), (("--serial-dw",), (False, False)),
                                           (("--no-overlap",), (False, False)), (("--deterministic", "--no-trace"), (False, False))],
                         ids=["default", "dw-behind-sum", "update-behind-products", "both", "no-fold-dx", "serial-dw", "no-overlap", "deterministic"])
def test_the_switches_move_the_launches(hip, batch, flags, expect):
    """The results cannot tell the two orders apart, so the model counts the steps it issued each way: one iteration of every configuration."""
    from dlrm_flexflow_amd import ffmodel
    app = ffmodel.DLRM(["--backend", HIP, "--lr", str(DH.LR)] + DH.model_args(batch, list(flags)))
    app.warmup()
    app.model.sync()
    got = (app.model.counter("fold_dw_on_compute_steps") > 0, app.model.counter("fold_update_early_steps") > 0)
    app.close()
    assert got == expect
