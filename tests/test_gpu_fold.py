"""GPU tests (-m gpu) of the fold extension's kernels through the C ABI (include/ff_hip_fold.h): the grouped product P_t = E_t W_t^T, the gather-add
S = sum_t P_t[ids_t], and ffh_linear_fwd over kept reduction-depth segments with S as the epilogue's addend -- each against a float64 numpy
computation of the UNFOLDED formula at |error| <= 1e-5 * sum_k |a_k b_k| + 1e-6, the term mass over the full-width sum.  D = 32 and 128, out = 128
and 256 throughout; the shapes are the smallest that reach every path: one-row and ragged groups, a ragged last block of the gather, bags of 1 and 3,
the plain MFMA kernel (everything small) and the persistent kernel with its kept-k-tile stream (16384 rows: one full round of 128 x 128 tiles)."""
import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import fold_helpers as FH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = [(32, 128), (32, 256), (128, 128), (128, 256)]


@pytest.fixture(scope="module")
def fold(hip):
    return capi.fold_api(hip)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(a):
    return a.astype(np.float64)


@pytest.mark.parametrize("D,OUT", DIMS)
def test_grouped_product_one_launch(hip, fold, D, OUT):
    """Tables of 1, 3, 17, 200 and 2208 rows in one launch; W_t is a column block of a wider weight.  Rows behind a group's last stay untouched."""
    rng = np.random.default_rng(D * 1000 + OUT)
    rows = [1, 3, 17, 200, 2208]
    ldw = D * (len(rows) + 1)
    w = (rng.uniform(-1, 1, (OUT, ldw)) / np.sqrt(D)).astype(np.float32)
    E = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    wd, Ed = dev(w), [dev(e) for e in E]
    P = torch.full((sum(rows) + 1, OUT), -7.0, device=DEV)
    groups, r0 = [], 0
    for t, r in enumerate(rows):
        groups.append((Ed[t], D, D * (t + 1), P[r0:], r))
        r0 += r
    fold.call("ffh_fold_product", fold.groups(groups), len(rows), wd, ldw, D, OUT, None)
    torch.cuda.synchronize()
    got = P.cpu().numpy()
    assert np.all(got[-1] == -7.0), "the row behind the last group was written"
    r0 = 0
    for t, r in enumerate(rows):
        wt = w[:, D * (t + 1):D * (t + 2)]
        FH.assert_within(got[r0:r0 + r], f64(E[t]) @ f64(wt).T, np.abs(f64(E[t])) @ np.abs(f64(wt)).T, f"product of the {r}-row table")
        r0 += r


ID_SETS = [("random", "random", "random"), ("equal", "random", "equal"), ("last", "last", "last")]


@pytest.mark.parametrize("D,OUT", DIMS)
@pytest.mark.parametrize("batch", [384, 500])
@pytest.mark.parametrize("bag", [1, 3])
def test_gather_add(hip, fold, D, OUT, batch, bag):
    """S[b] = sum over tables, then bag positions, of rows of the products: random ids, all ids equal, ids on the last row; batch 500 leaves the
    last workgroup ragged.  The reference adds the same fp32 rows in float64 (D plays no part here: the rows are OUT wide)."""
    rng = np.random.default_rng(batch * 10 + bag + D + OUT)
    rows = [3, 17, 200]
    P = [rng.uniform(-1, 1, (r, OUT)).astype(np.float32) for r in rows]
    Pd = [dev(p) for p in P]
    for kinds in ID_SETS:
        ids = [FH.make_ids(rng, k, batch, bag, r) for k, r in zip(kinds, rows)]
        idd = [dev(i) for i in ids]
        S = torch.full((batch + 1, OUT + 4), -7.0, device=DEV)
        tabs = hip.emb_tables([(idd[t], Pd[t], None, rows[t], 0) for t in range(len(rows))])
        fold.call("ffh_fold_gather_add", tabs, len(rows), bag, OUT, batch, FH.AGGR_SUM, S, OUT + 4, None)
        torch.cuda.synchronize()
        got = S.cpu().numpy()
        assert np.all(got[batch] == -7.0) and np.all(got[:, OUT:] == -7.0), "written outside [batch][out]"
        ref = sum(f64(P[t])[ids[t]].sum(1) for t in range(len(rows)))
        mass = sum(np.abs(f64(P[t]))[ids[t]].sum(1) for t in range(len(rows)))
        FH.assert_within(got[:batch, :OUT], ref, mass, f"gather-add {kinds}")
    assert fold.rc("ffh_fold_gather_add", tabs, len(rows), bag, OUT, batch, FH.AGGR_AVG, S, OUT + 4, None) == FH.UNSUPPORTED


def _layer(rng, D, OUT, batch, bag, folded, ntab=6, rows=(3, 2208, 17, 200, 64, 1)):
    """A first top layer over [bottom | 6 tables] of width D each: the tables, ids, x as the gather leaves it, w, bias, and the kept segments."""
    IN = D * (ntab + 1)
    E = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    ids = [FH.make_ids(rng, "last" if t == 3 else ("equal" if t == 5 else "random"), batch, bag, rows[t]) for t in range(ntab)]
    x = np.empty((batch, IN), np.float32)
    x[:, :D] = np.maximum(rng.uniform(-1, 1, (batch, D)), 0)
    for t in range(ntab):
        x[:, D * (t + 1):D * (t + 2)] = E[t][ids[t]].sum(1, dtype=np.float32) if bag == 1 else f64(E[t])[ids[t]].sum(1).astype(np.float32)
    w = (rng.uniform(-1, 1, (OUT, IN)) / np.sqrt(IN)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, OUT).astype(np.float32)
    keep, k0 = [], 0
    for t in sorted(folded):
        if D * (t + 1) > k0:
            keep.append((k0, D * (t + 1) - k0))
        k0 = D * (t + 2)
    if IN > k0:
        keep.append((k0, IN - k0))
    return IN, E, ids, x, w, b, keep


def _folded_forward(hip, fold, D, OUT, batch, bag, folded, act, rows):
    """products -> gather-add -> ffh_fold_linear_fwd; returns (got, ref, mass, route).  With bags of 3 the gathered x is a rounded sum of three rows, so
    the reference is stated on the TABLE rows (the unfolded formula in float64: sum over the bag of E[id] . w), not on the rounded x."""
    rng = np.random.default_rng(D + OUT + batch + bag + 17 * len(folded))
    IN, E, ids, x, w, b, keep = _layer(rng, D, OUT, batch, bag, folded, rows=rows)
    xd, wd, bd = dev(x), dev(w), dev(b)
    for t in folded:
        xd[:, D * (t + 1):D * (t + 2)] = float("nan")      # the kernel must not read the folded columns: a NaN there would reach y
    y = torch.full((batch, OUT), -7.0, device=DEV)
    S = None
    if folded:
        Ed = {t: dev(E[t]) for t in folded}
        idd = {t: dev(ids[t]) for t in folded}
        P = torch.zeros(sum(rows[t] for t in folded), OUT, device=DEV)
        groups, tabs, r0 = [], [], 0
        for t in sorted(folded):
            groups.append((Ed[t], D, D * (t + 1), P[r0:], rows[t]))
            tabs.append((idd[t], P[r0:], None, rows[t], 0))
            r0 += rows[t]
        S = torch.zeros(batch, OUT, device=DEV)
        fold.call("ffh_fold_product", fold.groups(groups), len(groups), wd, IN, D, OUT, None)
        fold.call("ffh_fold_gather_add", hip.emb_tables(tabs), len(tabs), bag, OUT, batch, FH.AGGR_SUM, S, OUT, None)
    fold.call("ffh_fold_linear_fwd", xd, IN, y, OUT, wd, bd, IN, OUT, batch, act, fold.segs(keep), len(keep), S, OUT, None)
    route = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    torch.cuda.synchronize()
    x64 = f64(x)
    for t in folded:
        x64[:, D * (t + 1):D * (t + 2)] = f64(E[t])[ids[t]].sum(1)
    ref = x64 @ f64(w).T + f64(b)
    mass = np.abs(x64) @ np.abs(f64(w)).T + np.abs(f64(b))
    if act == FH.RELU:
        ref = np.maximum(ref, 0)
    return y.cpu().numpy(), ref, mass, route


ROWS = (3, 2208, 17, 200, 64, 1)


@pytest.mark.parametrize("D,OUT", DIMS)
@pytest.mark.parametrize("batch", [256, 128 * 5])
@pytest.mark.parametrize("folded", [(0, 2, 5), (0, 1, 2, 3, 4, 5)], ids=["tables-0-2-5", "bottom-block-only"])
def test_forward_with_segment_list_and_addend(hip, fold, D, OUT, batch, folded):
    """In = D + 6 D with tables 0, 2 and 5 folded (the list of folded tables starts with the first table and ends with the last), and with every
    table folded (only the bottom block is left to the GEMM); bags of 1 and 3; ReLU and none."""
    for bag, act in ((1, FH.RELU), (3, FH.NONE)):
        got, ref, mass, route = _folded_forward(hip, fold, D, OUT, batch, bag, folded, act, ROWS)
        assert "fold_linear_fwd gemm" in route, route
        FH.assert_within(got, ref, mass, f"forward, tables {folded} folded, bag {bag}: route {route}")


@pytest.mark.parametrize("D,OUT", DIMS)
@pytest.mark.parametrize("batch", [256, 128 * 5])
def test_forward_with_the_empty_list_is_ffh_linear_fwd(hip, fold, D, OUT, batch):
    """No list and no addend: the same launches, the same bytes."""
    rng = np.random.default_rng(D + OUT + batch)
    IN, E, ids, x, w, b, keep = _layer(rng, D, OUT, batch, 1, (), rows=ROWS)
    assert keep == [(0, IN)]
    xd, wd, bd = dev(x), dev(w), dev(b)
    ya, yb = torch.zeros(batch, OUT, device=DEV), torch.zeros(batch, OUT, device=DEV)
    hip.call("ffh_linear_fwd", xd, IN, ya, OUT, wd, bd, IN, OUT, batch, FH.RELU, None)
    ra = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    fold.call("ffh_fold_linear_fwd", xd, IN, yb, OUT, wd, bd, IN, OUT, batch, FH.RELU, fold.segs([]), 0, None, 0, None)
    rb = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    torch.cuda.synchronize()
    assert ra == rb and ya.cpu().numpy().tobytes() == yb.cpu().numpy().tobytes()
    # ... and the whole depth as ONE kept segment goes through the fold kernels: within the bound of the same formula
    yc = torch.zeros(batch, OUT, device=DEV)
    fold.call("ffh_fold_linear_fwd", xd, IN, yc, OUT, wd, bd, IN, OUT, batch, FH.RELU, fold.segs(keep), 1, None, 0, None)
    torch.cuda.synchronize()
    FH.assert_within(yc.cpu().numpy(), np.maximum(f64(x) @ f64(w).T + f64(b), 0), np.abs(f64(x)) @ np.abs(f64(w)).T + np.abs(f64(b)), "one segment, no addend")


@pytest.mark.parametrize("folded", [(0, 2, 5), (0, 1, 2, 3, 4, 5), ()], ids=["tables-0-2-5", "bottom-block-only", "nothing-folded"])
def test_forward_on_the_persistent_kernel(hip, fold, folded):
    """16384 rows, D = 128, out = 256: 256 tiles of 128 x 128, one round of the persistent forward kernel, which here walks the KEPT k-tiles only
    (3 of 14 folded out; 12 of 14: two k-tiles per output tile; none) and reads the addend in its epilogue.  The plan query names the same kernel."""
    assert hip.device_info().compute_units >= 256, "one round of 256 tiles needs the full chip"
    D, OUT, batch = 128, 256, 16384
    got, ref, mass, route = _folded_forward(hip, fold, D, OUT, batch, 1, folded, FH.RELU, ROWS)
    nk = 14 - 2 * len(folded)
    assert f"sk_128x128x64|kept={nk}/14" in route and ("addend" in route) == bool(folded), route
    FH.assert_within(got, ref, mass, f"persistent forward, tables {folded} folded")
    x = torch.zeros(batch, 7 * D, device=DEV); y = torch.zeros(batch, OUT, device=DEV); w = torch.zeros(OUT, 7 * D, device=DEV)
    keep = [(0, D)] if len(folded) == 6 else [(0, 7 * D)]
    assert fold.rc("ffh_fold_linear_fwd_plan", x, 7 * D, y, OUT, w, None, 7 * D, OUT, batch, fold.segs(keep), 1, y, OUT) == 2
    assert fold.rc("ffh_fold_linear_fwd_plan", x, 7 * D, y, OUT, w, None, 7 * D, OUT, 256, fold.segs(keep), 1, y, OUT) == 1


def test_refusals_launch_nothing(hip, fold):
    D, OUT, batch = 32, 128, 64
    x = torch.zeros(batch, 7 * D, device=DEV); w = torch.zeros(OUT, 7 * D, device=DEV); y = torch.full((batch, OUT), -7.0, device=DEV)
    bad = [[(8, 16)], [(0, 24)], [(32, 32), (0, 32)], [(0, 8 * D)]]
    codes = [fold.rc("ffh_fold_linear_fwd", x, 7 * D, y, OUT, w, None, 7 * D, OUT, batch, FH.NONE, fold.segs(k), len(k), None, 0, None) for k in bad]
    assert codes == [FH.UNSUPPORTED, FH.UNSUPPORTED, -1, -1], codes
    assert fold.rc("ffh_fold_linear_fwd", x, 7 * D, y, OUT - 28, w, None, 7 * D, OUT - 28, batch, FH.NONE, fold.segs([(0, D)]), 1, None, 0, None) == FH.UNSUPPORTED
    e = torch.zeros(4, D, device=DEV); p = torch.zeros(4, OUT, device=DEV)
    assert fold.rc("ffh_fold_product", fold.groups([(e, D, 8, p, 4)]), 1, w, 7 * D, D, OUT, None) == FH.UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
