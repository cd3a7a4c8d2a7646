"""GPU tests (-m gpu) of the fold route in the host model: a `cat` DLRM with 6 tables of 3-5000-1-40-70000-300 rows, D = 32, bottom
13-64-32, top 224-128-64-1, batch 512.  Four of the tables are folded out of the first top layer's forward GEMM (5000 and 70000 rows lie above the
threshold).  The route on against --no-fold-small-tables on the weight DELTAS of the warm-up iteration + three steps, at the bound
tests/test_gpu_round4.py::_delta_check applies between the HIP kernels and the oracle (re-stated below); eager against hipGraph replay and run
against run, bit for bit under --deterministic."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import fold_helpers as FH

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
LR, STEPS = 0.01, 4        # the driver's warm-up iteration + three steps


def _delta_check(name, da, db, tol_mass, tol_ulp, worst, explained=None, extra_tol=0.0):
    """tests/test_gpu_round4.py::_delta_check: |delta_a - delta_b| <= 1e-5 of the update's term mass (+ the rounding of w itself); an element beyond
    that must lie where a relu' flip between the two runs -- derived from their own activations, step by step -- reaches (the rows of the flipped
    units, the table rows the flipped samples hit), and stays within 5e-2 of the mass there."""
    err = np.abs(da - db)
    tol = tol_mass + tol_ulp + extra_tol
    bad = err > tol
    if explained is None:
        explained = np.zeros(err.shape, bool)
    explained = np.broadcast_to(explained, err.shape)
    unexplained = bad & ~explained
    worst[name] = (int(bad.sum()), int(unexplained.sum()), float((err / tol).max()))
    at = int(np.where(unexplained, err / tol, 0).argmax())
    msg = (f"{name}: {int(unexplained.sum())} of {err.size} deltas beyond 1e-5 of the term mass that no relu' flip explains ({int(bad.sum())} beyond it in all); "
           f"worst unexplained at flat index {at}: off by {err.flat[at]:.3e}, bound {tol.flat[at]:.3e} (delta on {da.flat[at]:.3e} off {db.flat[at]:.3e})")
    assert not unexplained.any(), msg
    assert np.all(err <= 5000 * tol_mass + tol_ulp), msg


def test_three_steps_with_the_route_on_against_off(hip):
    on = FH.run_model(HIP, [], snapshots=True)
    off = FH.run_model(HIP, ["--no-fold-small-tables"], snapshots=True)
    assert on["folded"] == 4 and off["folded"] == 0
    assert on["w0"].keys() == off["w0"].keys()
    for k in on["w0"]:
        assert on["w0"][k].tobytes() == off["w0"][k].tobytes(), f"{k}: the two runs start from different weights"
    names, B, D = off["names"], FH.MODEL_B, FH.MODEL_D
    f64 = lambda a: np.abs(a).astype(np.float64)
    # relu' flips between the two runs, from their own activations: per layer the units and the samples whose y > 0 differs in any step
    concat = [n for n in names if n.startswith("Concat")][0]
    flip_units, flip_rows, flip_samples, nflips = {}, {}, np.zeros(B, bool), {}
    for nm in on["masks"][0]:
        f = np.zeros((B, on["masks"][0][nm].shape[-1]), bool)
        for ma, mb in zip(on["masks"], off["masks"]):
            f |= (ma[nm] ^ mb[nm]).reshape(B, -1)
        flip_units[nm], flip_rows[nm], nflips[nm] = f.any(0), f.any(1), int(f.sum())
        if names.index(nm) > names.index(concat):
            flip_samples |= f.any(1)
    print("relu' flips between the two runs over the steps, per layer:", nflips)
    worst = {}
    first_top = names[names.index(concat) + 1]
    for nm in [n for n in names if n.startswith("Dense")]:
        li = names.index(nm)
        x = off["x0"] if li == 0 else off["out"][names[li - 1]]
        dy = off["dy"][nm]
        mass_w, mass_b = f64(dy).T @ f64(x), f64(dy).sum(0)
        for wi, mass in ((0, mass_w), (1, mass_b)):
            k = f"{nm}/{wi}"
            da = on["w1"][k].astype(np.float64) - on["w0"][k].astype(np.float64)
            db = off["w1"][k].astype(np.float64) - off["w0"][k].astype(np.float64)
            fu = flip_units.get(nm, np.zeros(da.shape[0], bool))
            above = np.zeros(B, bool)
            for n2, fr in flip_rows.items():
                if names.index(n2) > li:
                    above |= fr
            extra = 4.0 * LR * STEPS * (f64(dy[above]).T @ f64(x[above]) if wi == 0 else f64(dy[above]).sum(0)) if above.any() else 0.0
            _delta_check(k, da, db, 1e-5 * LR * STEPS * mass.reshape(da.shape), STEPS * 2 * np.spacing(np.abs(off["w0"][k]).astype(np.float32)).astype(np.float64), worst,
                         explained=fu[:, None] if da.ndim == 2 else fu, extra_tol=extra)
            assert np.abs(db).max() > 0
    # tables: a row's update is lr * the sum of its hits' rows of dZ = dy1 W1[:, the table's columns]
    dzmass = f64(off["dy"][first_top]) @ f64(off["w0"][f"{first_top}/0"])
    t = 0
    for nm in names:
        if not nm.startswith("Embedding"):
            continue
        k = f"{nm}/0"
        ids = off["ids"][t].reshape(B, -1)
        R = on["w0"][k].shape[0]
        rowmass = np.zeros((R, D))
        for l in range(ids.shape[1]):
            np.add.at(rowmass, ids[:, l], dzmass[:, D * (t + 1):D * (t + 2)])
        da = on["w1"][k].astype(np.float64) - on["w0"][k].astype(np.float64)
        db = off["w1"][k].astype(np.float64) - off["w0"][k].astype(np.float64)
        hit = np.zeros(R, bool); hit[ids[flip_samples].reshape(-1)] = True
        _delta_check(k, da, db, 1e-5 * LR * STEPS * rowmass, STEPS * 2 * np.spacing(np.abs(off["w0"][k]).astype(np.float32)).astype(np.float64), worst, explained=hit[:, None])
        untouched = np.ones(R, bool); untouched[ids.reshape(-1)] = False
        assert not da[untouched].any() and not db[untouched].any()
        t += 1
    assert t == len(FH.MODEL_ROWS)
    np.testing.assert_allclose(on["pred"], off["pred"], rtol=2e-5, atol=2e-6)
    print("per tensor: elements beyond 1e-5 of the mass, of those unexplained, worst error / bound:", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:8]})


def _same_bits(a, b, what):
    assert a["w1"].keys() == b["w1"].keys()
    for k in a["w1"]:
        assert a["w1"][k].tobytes() == b["w1"][k].tobytes(), f"{k}: {what}"
    assert a["pred"].tobytes() == b["pred"].tobytes(), f"predictions: {what}"


def test_route_on_eager_equals_graph_replay_and_itself_bit_for_bit(hip):
    """--deterministic (no floating-point atomics anywhere in the step: same kernels => same bits).  The replayed run captures its first traced step
    and replays the next two: the products, the gather-add and their two events are nodes of that graph."""
    eager = FH.run_model(HIP, ["--deterministic", "--no-trace"])
    again = FH.run_model(HIP, ["--deterministic", "--no-trace"])
    replay = FH.run_model(HIP, ["--deterministic", "--always-replay"], trace=True)
    serial = FH.run_model(HIP, ["--deterministic", "--no-trace", "--no-overlap", "--no-early-sort", "--serial-dw"])
    for r in (eager, again, replay, serial):
        assert r["folded"] == 4
    assert replay["replays"] >= 2 and eager["replays"] == 0
    _same_bits(eager, again, "two eager runs with the route on differ")
    _same_bits(eager, replay, "the replayed step differs from the eager one")
    _same_bits(eager, serial, "the sum computed on the side stream differs from the one computed on the compute stream")
    assert any(eager["w1"][k].tobytes() != eager["w0"][k].tobytes() for k in eager["w1"])
