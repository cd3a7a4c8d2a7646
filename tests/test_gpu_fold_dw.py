"""GPU tests (-m gpu) of the weight-gradient half of the fold extension through the C ABI (include/ff_hip_fold.h, ABI 2): the segmented sum
G_t = sum of dy over the hits of a table's rows, the products dW[:, cols_t] += G_t^T E_t, the stream-K weight gradient over kept 128-column tiles, and
the three together against the unfolded dy^T x -- each against float64 numpy at |error| <= 1e-5 * sum_k |a_k b_k| + 1e-6, the term mass over the full
unfolded sum.  Shapes: tables of 1, 3, 300 and 5000 rows in one call (one row, fewer rows than an MFMA tile, a ragged chunk, twenty chunks), width 256,
batch 512, bags of 1 and 2; the GEMM at out = 256, in = 640 and the smallest batch at which the stream-K form takes the kept tiles."""
import ctypes as C

import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import fold_helpers as FH
import fold_dw_helpers as DH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT, IN, NT = 256, 640, 5      # the GEMM tests: five 128-column blocks
SENT = -7.0


@pytest.fixture(scope="module")
def fold(hip):
    return capi.fold_api(hip)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(a):
    return a.astype(np.float64)


def tiles(lst):
    return (C.c_int32 * len(lst))(*lst)


def attach_workspace(hip, ntables, bag, width, batch):
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(ntables, bag, width, batch) + 256
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(ws, n)


def segment_sum(hip, fold, idd, dyd, lddy, rows, bag, width, batch, stream=None):
    """G of all tables in one call, pre-filled with a sentinel, one spare row behind the last table."""
    G = torch.full((sum(rows) + 1, width), SENT, device=DEV)
    tabs, r0 = [], 0
    for t, r in enumerate(rows):
        tabs.append((idd[t], G[r0:], dyd, r, lddy))
        r0 += r
    fold.call("ffh_fold_segment_sum", hip.emb_tables(tabs), len(rows), bag, width, batch, stream)
    torch.cuda.synchronize()
    return G


@pytest.mark.parametrize("bag", [1, 2])
def test_segment_sum(hip, fold, bag):
    attach_workspace(hip, len(DH.ROWS), bag, DH.WIDTH, DH.BATCH)
    side = torch.cuda.Stream()
    for kind in DH.KINDS:
        dy, ids, _ = DH.segment_inputs(bag, kind)
        dyd, idd = dev(dy), [dev(i) for i in ids]
        G = segment_sum(hip, fold, idd, dyd, DH.WIDTH, DH.ROWS, bag, DH.WIDTH, DH.BATCH)
        got = G.cpu().numpy()
        assert np.all(got[-1] == SENT), "the row behind the last table was written"
        r0 = 0
        for t, r in enumerate(DH.ROWS):
            ref, mass = DH.segment_sum_f64(ids[t], dy, r)
            FH.assert_within(got[r0:r0 + r], ref, mass, f"segment sum, {r} rows, bag {bag}, ids {kind}")
            hit = np.zeros(r, bool); hit[ids[t].reshape(-1)] = True
            assert not got[r0:r0 + r][~hit].any(), "a row that was not hit is not exactly 0"
            r0 += r
        again = segment_sum(hip, fold, idd, dyd, DH.WIDTH, DH.ROWS, bag, DH.WIDTH, DH.BATCH)
        assert again.cpu().numpy().tobytes() == got.tobytes(), "two calls differ"
        other = segment_sum(hip, fold, idd, dyd, DH.WIDTH, DH.ROWS, bag, DH.WIDTH, DH.BATCH, stream=side.cuda_stream)
        assert other.cpu().numpy().tobytes() == got.tobytes(), "a call on another stream differs"


@pytest.mark.parametrize("bag", [1, 2])
def test_products_add_into_their_columns_only(hip, fold, bag):
    """dW [256][640]: column block 0 belongs to nobody, block t + 1 to table t.  dW holds a known pattern before the call."""
    for kind in DH.KINDS:
        dy, ids, E = DH.segment_inputs(bag, kind)
        G = [DH.segment_sum_f64(ids[t], dy, r)[0].astype(np.float32) for t, r in enumerate(DH.ROWS)]
        rng = np.random.default_rng(5)
        pat = rng.uniform(-1, 1, (DH.WIDTH, IN)).astype(np.float32)
        dw = dev(pat)
        Gd, Ed = [dev(g) for g in G], [dev(e) for e in E]
        groups = [(Ed[t], DH.D, DH.D * (t + 1), Gd[t], r) for t, r in enumerate(DH.ROWS)]
        fold.call("ffh_fold_dw_product", fold.groups(groups), len(groups), dw, IN, DH.D, DH.WIDTH, None)
        torch.cuda.synchronize()
        got = dw.cpu().numpy()
        assert got[:, :DH.D].tobytes() == pat[:, :DH.D].tobytes(), "a column outside every table's block changed"
        for t, r in enumerate(DH.ROWS):
            c0 = DH.D * (t + 1)
            ref = f64(pat[:, c0:c0 + DH.D]) + f64(G[t]).T @ f64(E[t])
            mass = np.abs(f64(pat[:, c0:c0 + DH.D])) + np.abs(f64(G[t])).T @ np.abs(f64(E[t]))
            FH.assert_within(got[:, c0:c0 + DH.D], ref, mass, f"pattern + G^T E, {r} rows, bag {bag}, ids {kind}")
    e = torch.zeros(4, DH.D, device=DEV); g = torch.zeros(4, DH.WIDTH, device=DEV)
    assert fold.rc("ffh_fold_dw_product", fold.groups([(e, DH.D, 0, g, 4)]), 1, dw, IN, 32, DH.WIDTH, None) == FH.UNSUPPORTED
    torch.cuda.synchronize()
    assert dw.cpu().numpy().tobytes() == got.tobytes()


# ---- the GEMM over kept column tiles -------------------------------------------------------------------------------------------------------------
def plan_batch(hip, nkept):
    """The smallest multiple of 64 the plan accepts: 8 k-tiles of 64 samples per workgroup over nkept x (OUT / 128) tiles."""
    g = hip.device_info().compute_units & ~7
    return -(-8 * g // (nkept * (OUT // 128))) * 64


@pytest.fixture(scope="module")
def gemm_data(hip):
    """x [B][640], dy [B][256] at the largest batch the tests need; x's blocks 1 and 3 are gathered rows of two tables (300 and 5000 rows), as a
    Concat leaves them.  The float64 references are computed once per batch and kept."""
    B = plan_batch(hip, 3)
    rng = np.random.default_rng(77)
    rows = {1: 300, 3: 5000}
    E = {t: rng.uniform(-1, 1, (r, DH.D)).astype(np.float32) for t, r in rows.items()}
    ids = {t: rng.integers(0, r, (B, 1)).astype(np.int64) for t, r in rows.items()}
    x = rng.uniform(-1, 1, (B, IN)).astype(np.float32)
    for t in rows:
        x[:, DH.D * t:DH.D * (t + 1)] = E[t][ids[t][:, 0]]
    dy = (rng.uniform(-1, 1, (B, OUT)) / 64).astype(np.float32)
    data = {"B": B, "x": x, "dy": dy, "E": E, "ids": ids, "rows": rows, "xd": dev(x), "dyd": dev(dy), "ref": {}}

    def ref(batch):
        if batch not in data["ref"]:
            a, b = f64(dy[:batch]), f64(x[:batch])
            data["ref"][batch] = (a.T @ b, np.abs(a).T @ np.abs(b), a.sum(0), np.abs(a).sum(0))
        return data["ref"][batch]
    data["ref_of"] = ref
    return data


def run_kept(hip, fold, data, batch, kept, with_db=True):
    dw = torch.full((OUT, IN), SENT, device=DEV)
    db = torch.full((OUT,), SENT, device=DEV)
    rc = fold.rc("ffh_fold_linear_bwd_dw", data["xd"], IN, data["dyd"], OUT, dw, db if with_db else None, IN, OUT, batch, tiles(kept), len(kept), None)
    route = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    torch.cuda.synchronize()
    return rc, route, dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize("kept", [[0, 2, 4], [0, 1, 2], [0, 1, 2, 3, 4]], ids=["tiles-0-2-4", "trailing-folded", "nothing-folded"])
def test_kept_tile_weight_gradient(hip, fold, gemm_data, kept):
    batch = plan_batch(hip, len(kept))
    args = (gemm_data["xd"], IN, gemm_data["dyd"], OUT, torch.zeros(OUT, IN, device=DEV), None, IN, OUT)
    assert fold.rc("ffh_fold_linear_bwd_dw_plan", *args, batch, tiles(kept), len(kept)) == 1
    assert fold.rc("ffh_fold_linear_bwd_dw_plan", *args, batch - 64, tiles(kept), len(kept)) == 0, "not the smallest batch the plan accepts"
    rc, route, dw, db = run_kept(hip, fold, gemm_data, batch, kept)
    assert rc == 0 and f"|kept={len(kept)}/{NT}" in route and "fold_linear_bwd_dw gemm|sk_128x128x64" in route, (rc, route)
    ref, mass, rdb, mdb = gemm_data["ref_of"](batch)
    for t in range(NT):
        cols = slice(128 * t, 128 * (t + 1))
        if t in kept:
            FH.assert_within(dw[:, cols], SENT + ref[:, cols], mass[:, cols] + abs(SENT), f"kept tile {t} of {kept}")
        else:
            assert np.all(dw[:, cols] == SENT), f"folded tile {t} was written"
    FH.assert_within(db, SENT + rdb, mdb + abs(SENT), f"bias gradient, kept {kept}")
    if len(kept) == NT:      # nothing folded: the weight gradient of ffh_linear_bwd_ex, within the bound of the same formula
        dw2 = torch.zeros(OUT, IN, device=DEV); db2 = torch.zeros(OUT, device=DEV)
        w = torch.zeros(OUT, IN, device=DEV); y = torch.zeros(batch, OUT, device=DEV)
        hip.call("ffh_linear_bwd_ex", gemm_data["xd"], IN, None, IN, y, OUT, gemm_data["dyd"], OUT, w, dw2, db2, IN, OUT, batch, FH.NONE,
                 capi.LINEAR_ONLY_DW | capi.LINEAR_DY_PREMASKED, None, None)
        torch.cuda.synchronize()
        FH.assert_within(dw2.cpu().numpy(), ref, mass, "ffh_linear_bwd_ex ONLY_DW")
        FH.assert_within(dw - SENT, f64(dw2.cpu().numpy()), 2 * mass + abs(SENT), "kept = all against ffh_linear_bwd_ex ONLY_DW")


def test_refusals_write_nothing(hip, fold, gemm_data):
    rc, route, dw, db = run_kept(hip, fold, gemm_data, 512, [0, 2, 4])
    assert rc == FH.UNSUPPORTED and np.all(dw == SENT) and np.all(db == SENT), (rc, route)
    batch = plan_batch(hip, 3)
    rc, route, dw, db = run_kept(hip, fold, gemm_data, batch, [1, 2, 4])
    assert rc == FH.UNSUPPORTED and np.all(dw == SENT) and np.all(db == SENT), (rc, route)
    rc, route, dw, db = run_kept(hip, fold, gemm_data, batch, [1, 2, 4], with_db=False)      # (without a bias gradient the first tile is free)
    assert rc == 0 and np.all(dw[:, :128] == SENT) and not np.any(dw[:, 128:384] == SENT), (rc, route)
    assert fold.rc("ffh_fold_linear_bwd_dw", gemm_data["xd"], IN, gemm_data["dyd"], OUT, torch.zeros(OUT, IN, device=DEV), None, IN, OUT, batch, tiles([2, 1]), 2, None) == -1


def test_sum_gemm_and_products_compose_to_the_unfolded_weight_gradient(hip, fold, gemm_data):
    """Tables behind blocks 1 and 3 folded, tiles {0, 2, 4} kept: dW = dy^T x over all 640 columns.  21 K lookups per table: the radix-sort form of the
    segmented sum (the tests above run its one-launch form)."""
    d, batch, kept = gemm_data, plan_batch(hip, 3), [0, 2, 4]
    attach_workspace(hip, 2, 1, OUT, batch)
    ts = sorted(d["rows"])
    rows = [d["rows"][t] for t in ts]
    idd = [dev(d["ids"][t][:batch]) for t in ts]
    G = segment_sum(hip, fold, idd, d["dyd"], OUT, rows, 1, OUT, batch)
    dw = torch.zeros(OUT, IN, device=DEV)
    fold.call("ffh_fold_linear_bwd_dw", d["xd"], IN, d["dyd"], OUT, dw, None, IN, OUT, batch, tiles(kept), len(kept), None)
    groups, r0 = [], 0
    for t, r in zip(ts, rows):
        groups.append((dev(d["E"][t]), DH.D, DH.D * t, G[r0:], r))
        r0 += r
    fold.call("ffh_fold_dw_product", fold.groups(groups), len(groups), dw, IN, DH.D, OUT, None)
    torch.cuda.synchronize()
    ref, mass, _, _ = d["ref_of"](batch)
    FH.assert_within(dw.cpu().numpy(), ref, mass, "segment sum + kept-tile GEMM + products against dy^T x")
