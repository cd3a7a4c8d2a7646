"""GPU tests (-m gpu) of the weight-gradient fold in the host model: a `cat` DLRM with D = 128, bottom 13-64-128, seven tables of
3-300-70000-40-80000-90000-100000 rows (three folded, four kept: five kept 128-column tiles of dW with the bottom block), top 1024-256-64-1, at the
smallest batch at which the stream-K weight gradient takes the kept tiles (about 13,000).  The route on against --no-fold-dw -- both with the forward
fold on, so the first iteration's forward and dy are the same bits -- on the weight deltas: after the warm-up iteration alone with no element excused,
after three more steps by the rule of tests/test_gpu_fold_model.py::_delta_check (re-stated) with at most 1 % of a tensor's elements excused by a relu'
flip; the counter; the deterministic mode (route off, the bits of --no-fold-dw); a replayed step against the eager one."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import fold_dw_helpers as DH

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
LR = DH.LR
MAX_EXCUSED = 0.01


def f64(a):
    return np.abs(a).astype(np.float64)


def _delta_check(name, da, db, tol_mass, tol_ulp, worst, explained=None, extra_tol=0.0):
    """tests/test_gpu_fold_model.py::_delta_check: |delta_a - delta_b| <= 1e-5 of the update's term mass (+ the rounding of w itself); an element beyond that
    must lie where a relu' flip between the two runs reaches and stay within 5e-2 of the mass there -- and here at most 1 % of the tensor may be so excused."""
    err = np.abs(da - db)
    tol = tol_mass + tol_ulp + extra_tol
    bad = err > tol
    if explained is None:
        explained = np.zeros(err.shape, bool)
    explained = np.broadcast_to(explained, err.shape)
    unexplained = bad & ~explained
    excused = bad & explained
    worst[name] = (int(bad.sum()), int(unexplained.sum()), float((err / tol).max()))
    at = int(np.where(unexplained, err / tol, 0).argmax())
    msg = (f"{name}: {int(unexplained.sum())} of {err.size} deltas beyond 1e-5 of the term mass that no relu' flip explains ({int(bad.sum())} beyond it in all); "
           f"worst unexplained at flat index {at}: off by {err.flat[at]:.3e}, bound {tol.flat[at]:.3e} (delta on {da.flat[at]:.3e} off {db.flat[at]:.3e})")
    assert not unexplained.any(), msg
    assert np.all(err <= 5000 * tol_mass + tol_ulp), msg
    assert excused.sum() <= MAX_EXCUSED * err.size, f"{name}: {int(excused.sum())} of {err.size} deltas excused by a relu' flip, more than 1 %"


def _compare(on, off, B, w_from, w_to, tag, steps, masks_from, worst):
    """The deltas w_to - w_from of both runs, the masses from the route-off run's activations of the snapshot `tag`; relu' flips over masks[masks_from:]."""
    names, D = off["names"], DH.MODEL_D
    concat = [n for n in names if n.startswith("Concat")][0]
    flip_units, flip_rows, flip_samples = {}, {}, np.zeros(B, bool)
    for nm in on["masks"][0]:
        f = np.zeros((B, on["masks"][0][nm].shape[-1]), bool)
        for ma, mb in zip(on["masks"][masks_from:], off["masks"][masks_from:]):
            f |= (ma[nm] ^ mb[nm]).reshape(B, -1)
        flip_units[nm], flip_rows[nm] = f.any(0), f.any(1)
        if names.index(nm) > names.index(concat):
            flip_samples |= f.any(1)
    first_top = names[names.index(concat) + 1]
    out, dyo = off["out" + tag], off["dy" + tag]
    for nm in [n for n in names if n.startswith("Dense")]:
        li = names.index(nm)
        x = off["x0" + tag] if li == 0 else out[names[li - 1]]
        dy = dyo[nm]
        mass_w, mass_b = f64(dy).T @ f64(x), f64(dy).sum(0)
        for wi, mass in ((0, mass_w), (1, mass_b)):
            k = f"{nm}/{wi}"
            da = on[w_to][k].astype(np.float64) - on[w_from][k].astype(np.float64)
            db = off[w_to][k].astype(np.float64) - off[w_from][k].astype(np.float64)
            fu = flip_units.get(nm, np.zeros(da.shape[0], bool))
            above = np.zeros(B, bool)
            for n2, fr in flip_rows.items():
                if names.index(n2) > li:
                    above |= fr
            extra = 4.0 * LR * steps * (f64(dy[above]).T @ f64(x[above]) if wi == 0 else f64(dy[above]).sum(0)) if above.any() else 0.0
            _delta_check(k, da, db, 1e-5 * LR * steps * mass.reshape(da.shape), steps * 2 * np.spacing(np.abs(off[w_from][k]).astype(np.float32)).astype(np.float64), worst,
                         explained=fu[:, None] if da.ndim == 2 else fu, extra_tol=extra)
            assert np.abs(db).max() > 0
    dzmass = f64(dyo[first_top]) @ f64(off[w_from][f"{first_top}/0"])
    t = 0
    for nm in names:
        if not nm.startswith("Embedding"):
            continue
        k = f"{nm}/0"
        ids = off["ids" + tag][t].reshape(B, -1)
        R = on["w0"][k].shape[0]
        rowmass = np.zeros((R, D))
        for l in range(ids.shape[1]):
            np.add.at(rowmass, ids[:, l], dzmass[:, D * (t + 1):D * (t + 2)])
        da = on[w_to][k].astype(np.float64) - on[w_from][k].astype(np.float64)
        db = off[w_to][k].astype(np.float64) - off[w_from][k].astype(np.float64)
        hit = np.zeros(R, bool); hit[ids[flip_samples].reshape(-1)] = True
        _delta_check(k, da, db, 1e-5 * LR * steps * rowmass, steps * 2 * np.spacing(np.abs(off[w_from][k]).astype(np.float32)).astype(np.float64), worst, explained=hit[:, None])
        t += 1
    assert t == len(DH.MODEL_ROWS)


@pytest.fixture(scope="module")
def batch(hip):
    return DH.model_batch(hip.device_info().compute_units)


def test_route_on_against_no_fold_dw(hip, batch):
    on = DH.run_model(HIP, batch, [], snapshots=True)
    off = DH.run_model(HIP, batch, ["--no-fold-dw"], snapshots=True)
    assert on["folded"] == 3 and off["folded"] == 3
    assert on["folded_dw"] == 3 and off["folded_dw"] == 0
    for k in on["w0"]:
        assert on["w0"][k].tobytes() == off["w0"][k].tobytes(), f"{k}: the two runs start from different weights"
    # the warm-up iteration alone: the same forward and dy in both runs, so no relu' flip yet and no element excused
    for nm, a in on["dy_warm"].items():
        assert a.tobytes() == off["dy_warm"][nm].tobytes(), f"{nm}: dy of the first iteration differs"
    worst = {}
    on_w = dict(on, masks=on["masks"][:1]); off_w = dict(off, masks=off["masks"][:1])
    _compare(on_w, off_w, batch, "w0", "w_warm", "_warm", 1, 0, worst)
    assert all(v[0] == 0 for v in worst.values()), f"warm-up iteration: elements beyond the bound: {worst}"
    print("warm-up iteration, per tensor (beyond the bound, unexplained, worst error / bound):", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:6]})
    # three more steps, relu' flips from the two runs' own activations
    worst = {}
    _compare(on, off, batch, "w_warm", "w1", "", 3, 1, worst)
    np.testing.assert_allclose(on["pred"], off["pred"], rtol=2e-5, atol=2e-6)
    print("three steps, per tensor (beyond the bound, unexplained, worst error / bound):", {k: (v[0], v[1], round(v[2], 3)) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][2])[:6]})


def test_deterministic_mode_keeps_the_gemm_and_a_replayed_step_agrees(hip, batch):
    det = DH.run_model(HIP, batch, ["--deterministic", "--no-trace"])
    det_off = DH.run_model(HIP, batch, ["--deterministic", "--no-trace", "--no-fold-dw"])
    assert det["folded_dw"] == 0 and det_off["folded_dw"] == 0 and det["folded"] == 3
    for k in det["w1"]:
        assert det["w1"][k].tobytes() == det_off["w1"][k].tobytes(), f"{k}: --deterministic differs from --deterministic --no-fold-dw"
    assert det["pred"].tobytes() == det_off["pred"].tobytes()
    eager = DH.run_model(HIP, batch, ["--no-trace"], snapshots=True)
    replay = DH.run_model(HIP, batch, ["--always-replay"], trace=True, snapshots=True)
    assert eager["folded_dw"] == 3 and replay["folded_dw"] == 3
    assert replay["replays"] >= 2 and eager["replays"] == 0
    worst = {}
    _compare(replay, eager, batch, "w0", "w1", "", 4, 0, worst)
    np.testing.assert_allclose(replay["pred"], eager["pred"], rtol=2e-5, atol=2e-6)
