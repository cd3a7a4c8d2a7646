"""GPU tests (-m gpu) of the data-gradient half of the fold extension through the C ABI (include/ff_hip_fold.h, ABI 3).

ffh_fold_linear_bwd_dx: in = 640 (five 128-column tiles, tiles 0, 2, 4 kept), out = 128, at the smallest batch its plan accepts -- the kept columns bit
for bit those of ffh_linear_bwd_ex(ONLY_DX) of the whole layer (store and add, with and without mask-by-x), the skipped columns untouched, the column sums
bit-equal to the plain call's on columns 0..127 (compared on exactly representable data: the sums meet by float atomics, whose order is free), and the
refusals, which launch nothing.

ffh_fold_table_update: tables of 1, 3, 63 and 1543 rows, batch 4096, D 128, out 256 and 1024, bags of 1 and 2, from the G of ffh_fold_segment_sum --
against float64 of the UNFOLDED formula at 1e-5 lr (term mass) + 2 ulp(w); the same bits on two runs and two streams; the _lr twin equal to the float form."""
import ctypes as C

import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import fold_helpers as FH
import fold_dx_helpers as XH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN, OUT, NT, KEPT = 640, 128, 5, [0, 2, 4]
SENT = -7.0
OVERWRITE, MASK = capi.LINEAR_DX_OVERWRITE, capi.LINEAR_DX_MASK_BY_X


@pytest.fixture(scope="module")
def fold(hip):
    return capi.fold_api(hip)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tiles(lst):
    return (C.c_int32 * len(lst))(*lst)


# ---- the data gradient over kept column tiles ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dx_data(hip, fold):
    """The smallest multiple of 128 the plan accepts (searched through the plan itself) and the layer's operands at that batch."""
    bmax = 128 * 512
    big = torch.zeros(bmax, IN, device=DEV)
    dyb = torch.zeros(bmax, OUT, device=DEV)
    wz = torch.zeros(OUT, IN, device=DEV)
    B = None
    for nby in range(1, 513):
        if fold.rc("ffh_fold_linear_bwd_dx_plan", big, IN, big, IN, dyb, OUT, wz, IN, OUT, 128 * nby, OVERWRITE | MASK, tiles(KEPT), len(KEPT), None) == 1:
            B = 128 * nby
            break
    assert B is not None, "no batch up to 65536 is served"
    del big, dyb
    rng = np.random.default_rng(31)
    x = rng.uniform(-1, 1, (B, IN)).astype(np.float32)            # the mask: about half of dx is cleared
    dy = (rng.uniform(-1, 1, (B, OUT)) / 16).astype(np.float32)
    w = rng.uniform(-1, 1, (OUT, IN)).astype(np.float32)
    old = rng.uniform(-1, 1, (B, IN)).astype(np.float32)          # what dx holds before an accumulating call
    return {"B": B, "xd": dev(x), "dyd": dev(dy), "wd": dev(w), "old": old}


def plain_dx(hip, d, flags, start, colsum=None):
    dx = dev(start)
    y = torch.zeros(1, device=DEV)      # (never read: dy is final)
    dw = torch.zeros(1, device=DEV)
    if colsum is not None:
        hip.call("ffh_linear_bwd_set_dx_colsum", colsum, IN)
    hip.call("ffh_linear_bwd_ex", d["xd"], IN, dx, IN, y, OUT, d["dyd"], OUT, d["wd"], dw, None, IN, OUT, d["B"], FH.NONE,
             flags | capi.LINEAR_ONLY_DX | capi.LINEAR_DY_PREMASKED, None, None)
    route = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    torch.cuda.synchronize()
    assert "linear_bwd dx gemm|sk_128x128x64" in route and "streamk" not in route, route
    return dx.cpu().numpy(), route


def kept_dx(hip, fold, d, flags, start, kept=KEPT, colsum=None, batch=None):
    dx = dev(start)
    rc = fold.rc("ffh_fold_linear_bwd_dx", d["xd"], IN, dx, IN, d["dyd"], OUT, d["wd"], IN, OUT, d["B"] if batch is None else batch, flags,
                 tiles(kept), len(kept), colsum, None, None)
    route = hip.lib.ffh_linear_last_route(hip.ctx).decode()
    torch.cuda.synchronize()
    return rc, route, dx.cpu().numpy()


@pytest.mark.parametrize("mask", [0, MASK], ids=["plain", "mask-by-x"])
@pytest.mark.parametrize("store", [OVERWRITE, 0], ids=["store", "add"])
def test_kept_columns_are_the_plain_calls_bits(hip, fold, dx_data, store, mask):
    d = dx_data
    args = (d["xd"], IN, d["xd"], IN, d["dyd"], OUT, d["wd"], IN, OUT)
    assert fold.rc("ffh_fold_linear_bwd_dx_plan", *args, d["B"], store | mask, tiles(KEPT), len(KEPT), None) == 1
    assert fold.rc("ffh_fold_linear_bwd_dx_plan", *args, d["B"] - 128, store | mask, tiles(KEPT), len(KEPT), None) == 0, "not the smallest batch the plan accepts"
    start = np.full((d["B"], IN), SENT, np.float32) if store else d["old"]
    ref, _ = plain_dx(hip, d, store | mask, start)
    rc, route, got = kept_dx(hip, fold, d, store | mask, start)
    assert rc == 0 and f"fold_linear_bwd_dx gemm|sk_128x128x64|kept={len(KEPT)}/{NT}" in route, (rc, route)
    for t in range(NT):
        cols = slice(128 * t, 128 * (t + 1))
        if t in KEPT:
            assert got[:, cols].tobytes() == ref[:, cols].tobytes(), f"kept tile {t}: not the plain call's bits"
            assert np.any(got[:, cols] != start[:, cols])
        else:
            assert got[:, cols].tobytes() == start[:, cols].tobytes(), f"skipped tile {t} was written"


def test_colsum_is_the_plain_calls(hip, fold, dx_data):
    """The column sums meet by float atomics in an order nobody fixes, so two runs of ONE call agree bit for bit only where every partial sum is exact:
    dy in {-1/2, 0, 1/2} and w in {-1, 0, 1} make every dx a multiple of 1/2 of at most 64, and every partial sum of at most 2^16 of them a multiple of
    1/2 below 2^23: exact in fp32.  On such data the kept call's sums over columns 0..127 are the plain call's bits; the skipped columns keep what
    colsum held."""
    d = dict(dx_data)
    rng = np.random.default_rng(32)
    d["dyd"] = dev((rng.integers(-1, 2, (d["B"], OUT)) / 2).astype(np.float32))
    d["wd"] = dev(rng.integers(-1, 2, (OUT, IN)).astype(np.float32))
    assert d["B"] <= 1 << 16
    start = np.full((d["B"], IN), SENT, np.float32)
    for mask in (0, MASK):
        cs_ref = torch.full((IN,), 3.0, device=DEV)
        ref, route = plain_dx(hip, d, OVERWRITE | mask, start, colsum=cs_ref)
        assert "colsum" in route and hip.lib.ffh_linear_dx_colsum_used(hip.ctx) == 1, route
        cs = torch.full((IN,), 3.0, device=DEV)
        rc, route, got = kept_dx(hip, fold, d, OVERWRITE | mask, start, colsum=cs)
        assert rc == 0 and "|colsum" in route, (rc, route)
        a, b = cs.cpu().numpy(), cs_ref.cpu().numpy()
        assert a[:128].tobytes() == b[:128].tobytes(), "column sums of tile 0 differ from the plain call's"
        for t in range(NT):
            cols = slice(128 * t, 128 * (t + 1))
            if t in KEPT:
                assert a[cols].tobytes() == b[cols].tobytes() and got[:, cols].tobytes() == ref[:, cols].tobytes()
                np.testing.assert_array_equal(a[cols], 3.0 + got[:, cols].astype(np.float64).sum(0))
            else:
                assert np.all(a[cols] == 3.0), f"column sums of skipped tile {t} were written"
    # the kept call neither reads nor clears what the ctx has armed for the next ffh_linear_bwd_ex
    armed = torch.zeros(IN, device=DEV)
    hip.call("ffh_linear_bwd_set_dx_colsum", armed, IN)
    rc, route, got = kept_dx(hip, fold, d, OVERWRITE, start)
    assert rc == 0 and "colsum" not in route and not armed.cpu().numpy().any()
    ref, route = plain_dx(hip, d, OVERWRITE, start)
    assert "colsum" in route and armed.cpu().numpy().any(), "the armed column sums were consumed by the kept call"


def test_refusals_launch_nothing(hip, fold, dx_data):
    d = dx_data
    start = np.full((d["B"], IN), SENT, np.float32)

    def refused(rc, got, cs=None):
        assert rc == FH.UNSUPPORTED, rc
        assert np.all(got == SENT), "a refused call wrote dx"
        if cs is not None:
            assert np.all(cs.cpu().numpy() == 3.0), "a refused call wrote the column sums"
    cs = torch.full((IN,), 3.0, device=DEV)
    rc, _, got = kept_dx(hip, fold, d, OVERWRITE, start, kept=[1, 2, 4], colsum=cs)                 # column sums without tile 0
    refused(rc, got, cs)
    rc, _, got = kept_dx(hip, fold, d, OVERWRITE, start, kept=[1, 2, 4])                            # (without them the first tile is free)
    assert rc == 0 and np.all(got[:, :128] == SENT) and not np.any(got[:, 128:384] == SENT)
    rc, _, got = kept_dx(hip, fold, d, 0, start, colsum=cs)                                         # column sums of an accumulating call
    refused(rc, got, cs)
    hip.call("ffh_ctx_set_deterministic", 1)
    try:
        rc, _, got = kept_dx(hip, fold, d, OVERWRITE, start)
        assert fold.rc("ffh_fold_linear_bwd_dx_plan", d["xd"], IN, d["xd"], IN, d["dyd"], OUT, d["wd"], IN, OUT, d["B"], OVERWRITE, tiles(KEPT), len(KEPT), None) == 0
    finally:
        hip.call("ffh_ctx_set_deterministic", 0)
    refused(rc, got)
    rc, _, got = kept_dx(hip, fold, d, OVERWRITE, start, batch=d["B"] - 128)                        # a batch below the plan
    refused(rc, got)
    assert kept_dx(hip, fold, d, OVERWRITE, start, kept=[2, 1])[0] == -1                            # (bad arguments are not "unsupported")


# ---- the dense update of the folded tables ------------------------------------------------------------------------------------------------------------
LDE = XH.D + 4      # floats between rows of a table: the pad must stay as it is


def table_buffers(E):
    """Every table [rows + 1][LDE]: one spare row and four pad columns hold the sentinel."""
    out = []
    for e in E:
        b = np.full((e.shape[0] + 1, LDE), SENT, np.float32)
        b[:-1, :XH.D] = e
        out.append(dev(b))
    return out


def run_update(hip, fold, bag, out, Gd, wd, lr=None, block=None, stream=None):
    _, _, _, E = XH.inputs(bag, out)
    Ed = table_buffers(E)
    groups, r0 = [], 0
    for t, r in enumerate(XH.ROWS):
        groups.append((Ed[t], LDE, XH.D * (t + 1), Gd[r0:], r))
        r0 += r
    torch.cuda.synchronize()
    if block is None:
        fold.call("ffh_fold_table_update", fold.groups(groups), len(groups), wd, XH.IN, XH.D, out, C.c_float(lr), stream)
    else:
        fold.call("ffh_fold_table_update_lr", fold.groups(groups), len(groups), wd, XH.IN, XH.D, out, block, stream)
    torch.cuda.synchronize()
    return [e.cpu().numpy() for e in Ed]


@pytest.mark.parametrize("out", XH.OUTS)
@pytest.mark.parametrize("bag", [1, 2])
def test_table_update(hip, fold, bag, out):
    dy, w, ids, E = XH.inputs(bag, out)
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(XH.NTAB, bag, out, XH.BATCH) + 256
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(ws, n)
    dyd, wd, idd = dev(dy), dev(w), [dev(i) for i in ids]
    Gd = torch.full((sum(XH.ROWS) + 1, out), SENT, device=DEV)
    tabs, r0 = [], 0
    for t, r in enumerate(XH.ROWS):
        tabs.append((idd[t], Gd[r0:], dyd, r, out))
        r0 += r
    fold.call("ffh_fold_segment_sum", hip.emb_tables(tabs), XH.NTAB, bag, out, XH.BATCH, None)
    got = run_update(hip, fold, bag, out, Gd, wd, lr=XH.LR)
    refs = XH.references(bag, out)
    for t, r in enumerate(XH.ROWS):
        ref, mass = refs[t]
        assert np.all(got[t][-1] == SENT) and np.all(got[t][:, XH.D:] == SENT), f"{r} rows: the spare row or the pad was written"
        XH.assert_update_within(got[t][:-1, :XH.D], ref, mass, E[t], XH.LR, f"table update, {r} rows, bag {bag}, out {out}")
        un = XH.unhit(t, bag, out)
        assert got[t][:-1, :XH.D][un].tobytes() == E[t][un].tobytes(), f"{r} rows: a row nobody hit changed"
        assert np.all(np.any(got[t][:-1, :XH.D][~un] != E[t][~un], axis=1)), f"{r} rows: a row that was hit did not move"
    again = run_update(hip, fold, bag, out, Gd, wd, lr=XH.LR)
    side = torch.cuda.Stream()
    other = run_update(hip, fold, bag, out, Gd, wd, lr=XH.LR, stream=side.cuda_stream)
    lr = capi.lr_api(hip)
    blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device=DEV)
    lr.init(blk, XH.LR)
    torch.cuda.synchronize()
    assert np.float32(lr.read(blk).lr) == np.float32(XH.LR)
    twin = run_update(hip, fold, bag, out, Gd, wd, block=blk)
    for t in range(XH.NTAB):
        assert again[t].tobytes() == got[t].tobytes(), "two runs differ"
        assert other[t].tobytes() == got[t].tobytes(), "a run on another stream differs"
        assert twin[t].tobytes() == got[t].tobytes(), "the _lr twin differs from the float form at the same rate"


def test_table_update_refuses_narrow_tables(hip, fold):
    e = torch.full((4, 32), SENT, device=DEV); g = torch.zeros(4, 256, device=DEV); w = torch.zeros(256, 64, device=DEV)
    assert fold.rc("ffh_fold_table_update", fold.groups([(e, 32, 0, g, 4)]), 1, w, 64, 32, 256, C.c_float(0.1), None) == FH.UNSUPPORTED
    assert fold.rc("ffh_fold_table_update", fold.groups([(e, 32, 0, g, 4)]), 1, w, 64, 64, 200, C.c_float(0.1), None) == FH.UNSUPPORTED
    torch.cuda.synchronize()
    assert np.all(e.cpu().numpy() == SENT)
