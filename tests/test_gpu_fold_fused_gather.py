"""GPU tests (-m gpu) of ffh_fused_gather_linear_fwd (include/ffh_fused_gather.h): the persistent forward kernel over the kept k-tiles whose epilogue
gathers the folded tables' share itself.  The contract is the BITS of the two-call form, ffh_fold_gather_add + ffh_fold_linear_fwd(addend = S), on the
same inputs; the float64 bound |error| <= 1e-5 * mass + 1e-6 of the unfolded formula follows from it and is checked so that the file stands alone.

The entry takes the products P_t as given, so the tables here ARE their products (random [rows][out]) and x carries NaN in every folded k-tile.
Shapes: the persistent form needs one round of 128 x 128 tiles, one per workgroup (G = the CUs rounded down to 8): batch = 128 G at out = 128 is the
smallest, 32768 rows x 128 columns; every case asks ffh_fold_linear_fwd_plan and skips where it does not answer 2 -- the three cases that cannot be
whole tiles (ragged batch, out = 64, out = 192) out of eighteen."""
import functools

import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import fold_helpers as FH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KT = 64      # depth of a k-tile of the persistent kernel


@pytest.fixture(scope="module")
def fold(hip):
    return capi.fold_api(hip)


@pytest.fixture(scope="module")
def fg(hip):
    return capi.fused_gather_api(hip)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# name: (batch in units of G rows (a pair: multiplier, offset), out, rows per table, bag, bias, act, kept k-tiles as a 0/1 string, ids)
CASES = {
    "one-table":            ((128, 0), 128, [5], 1, True, FH.RELU, "100", "random"),
    "two-tables":           ((128, 0), 128, [5, 300], 1, True, FH.RELU, "100", "random"),
    "thirteen-tables":      ((128, 0), 128, [3, 1, 40, 7420, 300, 17, 2208, 64, 5, 1000, 2, 33, 500], 1, True, FH.RELU, "100", "random"),
    "a-table-of-one-row":   ((128, 0), 128, [1], 1, True, FH.RELU, "100", "random"),
    "first-and-last-row":   ((128, 0), 128, [300, 7], 1, True, FH.RELU, "100", "ends"),
    "bag-3":                ((128, 0), 128, [5, 300], 3, True, FH.RELU, "100", "random"),
    "bag-4-eight-tables":   ((128, 0), 128, [5, 300, 1, 17, 64, 2, 40, 9], 4, True, FH.NONE, "100", "random"),
    "sixteen-tables-bag-2": ((128, 0), 128, [5, 300, 1, 17, 64, 2, 40, 9, 3, 11, 100, 6, 33, 77, 8, 250], 2, True, FH.RELU, "100", "random"),
    "no-bias":              ((128, 0), 128, [5, 300, 40], 1, False, FH.RELU, "100", "random"),
    "no-activation":        ((128, 0), 128, [5, 300, 40], 1, True, FH.NONE, "100", "random"),
    "tile-0-folded":        ((128, 0), 128, [5, 300, 40], 1, True, FH.RELU, "011", "random"),
    "kept-tiles-apart":     ((128, 0), 128, [5, 300, 40], 1, True, FH.RELU, "10101", "random"),
    "out-256":              ((64, 0), 256, [5, 300, 40], 1, True, FH.RELU, "100", "random"),
    "seven-quarter-rounds": ((224, 0), 128, [5, 300, 40], 1, True, FH.RELU, "100", "random"),      # 1.75 G tiles: a workgroup walks two tiles, a quarter of them one
    "two-rounds":           ((256, 0), 128, [5, 300, 40], 1, True, FH.RELU, "10", "random"),
    "ragged-batch":         ((128, 72), 128, [5, 300], 1, True, FH.RELU, "100", "random"),         # a partial last row tile: not whole tiles
    "out-64":               ((256, 0), 64, [5, 300], 1, True, FH.RELU, "100", "random"),           # half a column tile
    "out-192":              ((128, 0), 192, [5, 300], 1, True, FH.RELU, "100", "random"),          # a partial last column tile
}


@functools.lru_cache(maxsize=None)
def _inputs(name, G):
    (mul, off), out, rows, bag, has_bias, act, kept, kind = CASES[name]
    batch, IN = mul * G + off, KT * len(kept)
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.uniform(-1, 1, (batch, IN)).astype(np.float32)
    w = (rng.uniform(-1, 1, (out, IN)) / np.sqrt(IN)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, out).astype(np.float32) if has_bias else None
    P = [rng.uniform(-1, 1, (r, out)).astype(np.float32) for r in rows]
    if kind == "ends":
        ids = [np.where(rng.integers(0, 2, (batch, bag)) == 0, 0, r - 1).astype(np.int64) for r in rows]
    else:
        ids = [FH.make_ids(rng, "random", batch, bag, r) for r in rows]
    keep = [(KT * k, KT) for k, c in enumerate(kept) if c == "1"]
    cols = np.concatenate([np.arange(k0, k0 + n) for k0, n in keep])
    return batch, IN, out, bag, act, x, w, b, P, ids, keep, cols


def _on_device(name, G):
    batch, IN, out, bag, act, x, w, b, P, ids, keep, cols = _inputs(name, G)
    xn = x.copy()
    folded = np.setdiff1d(np.arange(IN), cols)
    xn[:, folded] = np.nan      # the kernel must not read a folded k-tile: a NaN there would reach y
    d = {"x": dev(xn), "w": dev(w), "b": dev(b) if b is not None else None, "P": [dev(p) for p in P], "ids": [dev(i) for i in ids]}
    d["tabs"] = [(d["ids"][t], d["P"][t], None, P[t].shape[0], 0) for t in range(len(P))]
    return d


def _plan(fold, name, G, d, y):
    batch, IN, out, bag, act, x, w, b, P, ids, keep, cols = _inputs(name, G)
    rc = fold.rc("ffh_fold_linear_fwd_plan", d["x"], IN, y, out, d["w"], d["b"], IN, out, batch, fold.segs(keep), len(keep), y, out)
    if rc != 2:
        pytest.skip(f"ffh_fold_linear_fwd_plan answers {rc} for batch {batch}, out {out}: the persistent kernel does not serve the layer")


def _gather(hip, fg, fold, name, G, d, y, stream=None):
    batch, IN, out, bag, act, x, w, b, P, ids, keep, cols = _inputs(name, G)
    tabs = hip.emb_tables(d["tabs"])
    assert fg.rc("ffh_fused_gather_linear_fwd_plan", tabs, len(P), bag, FH.AGGR_SUM, d["x"], IN, y, out, d["w"], d["b"], IN, out, batch, act, fold.segs(keep), len(keep)) == 1
    fg.call("ffh_fused_gather_linear_fwd", tabs, len(P), bag, FH.AGGR_SUM, d["x"], IN, y, out, d["w"], d["b"], IN, out, batch, act, fold.segs(keep), len(keep), stream)
    return hip.lib.ffh_linear_last_route(hip.ctx).decode()


@pytest.mark.parametrize("name", list(CASES))
def test_the_bits_of_the_two_call_form(hip, fold, fg, name):
    G = hip.device_info().compute_units & ~7
    batch, IN, out, bag, act, x, w, b, P, ids, keep, cols = _inputs(name, G)
    d = _on_device(name, G)
    y2 = torch.full((batch + 1, out), -7.0, device=DEV)
    _plan(fold, name, G, d, y2)
    S = torch.zeros(batch, out, device=DEV)
    tabs = hip.emb_tables(d["tabs"])
    fold.call("ffh_fold_gather_add", tabs, len(P), bag, out, batch, FH.AGGR_SUM, S, out, None)
    fold.call("ffh_fold_linear_fwd", d["x"], IN, y2, out, d["w"], d["b"], IN, out, batch, act, fold.segs(keep), len(keep), S, out, None)
    route2 = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    assert f"sk_128x128x64|kept={len(keep)}/{IN // KT}|addend" in route2, route2
    y1 = torch.full((batch + 1, out), -7.0, device=DEV)
    route1 = _gather(hip, fg, fold, name, G, d, y1)
    assert f"fold_linear_fwd_gather gemm|sk_128x128x64|kept={len(keep)}/{IN // KT}|gather={len(P)}x{bag}" in route1, route1
    torch.cuda.synchronize()
    got, two = y1.cpu().numpy(), y2.cpu().numpy()
    assert np.all(got[batch] == -7.0), "written behind the last row"
    diff = int((got.view(np.uint32) != two.view(np.uint32)).sum())
    print(f"{name}: {diff} of {got.size} words differ from the two-call form")
    assert got.tobytes() == two.tobytes()
    # float64, the unfolded formula: the kept columns of x, and the rows of the products in place of the folded ones
    f = np.float64
    ref = x[:, cols].astype(f) @ w[:, cols].astype(f).T
    mass = np.abs(x[:, cols]).astype(f) @ np.abs(w[:, cols]).astype(f).T
    for t in range(len(P)):
        ref += P[t].astype(f)[ids[t]].sum(1)
        mass += np.abs(P[t]).astype(f)[ids[t]].sum(1)
    if b is not None:
        ref += b.astype(f); mass += np.abs(b).astype(f)
    if act == FH.RELU:
        ref = np.maximum(ref, 0)
    FH.assert_within(got[:batch], ref, mass, name)
    # a second call, and a call on another stream: the same bytes
    y3 = torch.full((batch + 1, out), -7.0, device=DEV)
    _gather(hip, fg, fold, name, G, d, y3)
    s2 = torch.cuda.Stream()
    y4 = torch.full((batch + 1, out), -7.0, device=DEV)
    torch.cuda.synchronize()
    _gather(hip, fg, fold, name, G, d, y4, s2.cuda_stream)
    torch.cuda.synchronize()
    assert y3.cpu().numpy().tobytes() == got.tobytes() and y4.cpu().numpy().tobytes() == got.tobytes()


def test_refusals_launch_nothing(hip, fold, fg):
    G = hip.device_info().compute_units & ~7
    name = "two-tables"
    batch, IN, out, bag, act, x, w, b, P, ids, keep, cols = _inputs(name, G)
    d = _on_device(name, G)
    y = torch.full((batch, out), -7.0, device=DEV)
    _plan(fold, name, G, d, y)
    segs = fold.segs(keep)

    def both(tabs, ntab, bag_, aggr, batch_):
        tabs = hip.emb_tables(tabs)
        a = fg.rc("ffh_fused_gather_linear_fwd_plan", tabs, ntab, bag_, aggr, d["x"], IN, y, out, d["w"], d["b"], IN, out, batch_, act, segs, len(keep))
        b_ = fg.rc("ffh_fused_gather_linear_fwd", tabs, ntab, bag_, aggr, d["x"], IN, y, out, d["w"], d["b"], IN, out, batch_, act, segs, len(keep), None)
        return a, b_
    no = (FH.UNSUPPORTED, FH.UNSUPPORTED)
    assert both(d["tabs"], 2, bag, FH.AGGR_AVG, batch) == no, "mean aggregation"
    assert both([d["tabs"][0]] * 17, 17, 1, FH.AGGR_SUM, batch) == no, "more tables than the argument block holds"
    assert both(d["tabs"], 2, 5, FH.AGGR_SUM, batch) == no, "a larger bag than the argument block holds"
    assert both([d["tabs"][0]] * 9, 9, 4, FH.AGGR_SUM, batch) == no, "more ids per sample than the LDS images hold"
    assert both(d["tabs"], 2, bag, FH.AGGR_SUM, 256) == no, "two row tiles: the persistent kernel does not serve the layer"
    assert both(d["tabs"], 2, bag, FH.AGGR_SUM, batch - 56) == no, "a partial row tile"
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
