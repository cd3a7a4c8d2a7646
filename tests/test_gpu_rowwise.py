"""Row-wise Adagrad on the GPU (include/ff_hip_rowwise.h): the row rule FFH_SPARSE_OPT_ROWWISE_ADAGRAD of the fused table update, bit for bit
against ffmodel.rowwise_adagrad_reference (one float32 numpy operation per rounded operation, the TREE sum order included).  The gradient is the
row's canonical sum, taken as tests/test_gpu_adagrad.py takes it, from code that is not under test: the CPU oracle's plain-SGD fused update with
lr = -1 on an all-zero table (rows renamed by their rank among the rows hit: a monotone map leaves every sum as it is).
The model-level tests are tests/test_gpu_rowwise_model.py."""
import ctypes as C

import numpy as np
import pytest

import bf16_helpers as B
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xADA6
EPS = 1e-10
STEPS = 2
IT0 = 5      # the bf16 update counter's value at the first step
_FORMS = [("fused", "scalar"), ("apply", "scalar"), ("fused", "lr"), ("apply", "lr")]


@pytest.fixture(scope="module")
def lr(hip):
    return capi.lr_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


@pytest.fixture(scope="module", autouse=True)
def _extension(hip):
    assert capi.rowwise_api(hip).lib.ffh_rowwise_abi_version() == capi.rowwise_header_abi_version() == 1


def _block(lr, base=0.05, W=3, S=3, N=4):
    """a schedule short enough to change the rate on every step of a test"""
    import torch
    blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device=DEV)
    lr.init(blk, base, W, S, N)
    return blk


@pytest.fixture(scope="module")
def rates(lr):
    """the float rates of the first steps of _block's schedule, as the block itself reports them"""
    blk = _block(lr)
    out = []
    for _ in range(STEPS):
        out.append(float(np.float32(lr.read(blk).lr)))
        lr.call("ffh_lr_state_advance", blk, None)
    assert len(set(out)) == STEPS, out
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _ws(hip, nt, L, D, batch):
    import torch
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(nt, L, D, batch) + 256
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(buf, n)
    return buf


def _opt(lr_value, wd, kind=capi.SPARSE_OPT_ROWWISE_ADAGRAD):
    o = capi.SparseOpt()
    o.kind = kind
    o.lr, o.weight_decay, o.epsilon = lr_value, wd, EPS
    o.momentum, o.nesterov, o.beta1, o.beta2 = 0.5, 1, 0.3, 0.4      # not Adagrad's: must not be read
    return o


def _canonical_sums(oracle, idx, g, aggr):
    """(rows hit, ascending; their canonical gradient sums [n][D]) from the oracle's plain-SGD update with lr = -1 on zeros"""
    uniq, inv = np.unique(idx, return_inverse=True)
    sums = oracle.embedding_bwd_sgd_fused(inv.reshape(idx.shape).astype(np.int64), g, np.zeros((len(uniq), g.shape[1]), np.float32), -1.0, aggr)
    return uniq, sums


def _round_rows(w32, mode, it, table, rows, col0=0):
    """tests/bf16_helpers.py's rounding on the given global rows of a table"""
    if mode == B.ROUND_NEAREST:
        return B.rne(w32)
    r = B.sr_bits(SEED, it, table, rows.astype(np.uint64)[:, None], (col0 + np.arange(w32.shape[1], dtype=np.uint64))[None, :])
    return B.sr(w32, r)


def _run_forms(hip, lr, b16, rates, shape, master, idx, g, A, wd, aggr, mode, kind, state_cols, forms=_FORMS):
    """Two steps of each form from `master`; yields (what, w tables, S tables, last route)."""
    import torch
    batch, L, D, rows = shape
    T = len(rows)
    for form, entry in forms:
        w = [m.clone() for m in master]
        S = [torch.full((R, state_cols) if state_cols else (R,), A, device=DEV) for R in rows]
        st = hip.emb_states([(S[t], None) for t in range(T)])
        blk = _block(lr)
        counter = torch.tensor([IT0], dtype=torch.int64, device=DEV)
        route = None
        for s in range(STEPS):
            opt = _opt(rates[s] if entry == "scalar" else 123.0, wd, kind)      # (the _lr entries ignore opt.lr)
            if mode is None:
                tabs = hip.emb_tables([(idx[s][t], w[t], g[s][t], rows[t], D) for t in range(T)])
                args = (tabs, st, T, L, D, batch, aggr, C.byref(opt))
                if form == "apply":
                    hip.check(hip.lib.ffh_embedding_bwd_sort_multi(hip.ctx, tabs, T, L, D, batch, None), "sort")
                name = "ffh_embedding_bwd_opt_fused_multi" if form == "fused" else "ffh_embedding_bwd_opt_apply_multi"
                if entry == "lr":
                    lr.call(name + "_lr", *args, blk, None)
                else:
                    hip.check(getattr(hip.lib, name)(hip.ctx, *args, None), name)
            else:
                tabs = b16.tables([(idx[s][t], w[t], g[s][t], rows[t], D, 10 + t, 0) for t in range(T)])
                rnd = b16.rounding(mode, SEED, counter)
                args = (tabs, st, T, L, D, batch, aggr, C.byref(opt), C.byref(rnd))
                if form == "apply":
                    b16.base.check(b16.lib.ffh_embedding_bwd_sort_multi_bf16(b16.ctx, tabs, T, L, D, batch, None), "sort16")
                name = "ffh_embedding_bwd_opt_fused_multi_bf16" if form == "fused" else "ffh_embedding_bwd_opt_apply_multi_bf16"
                if entry == "lr":
                    lr.call(name + "_lr", *args, blk, None)
                else:
                    b16.base.check(getattr(b16.lib, name)(b16.ctx, *args, None), name)
            lr.call("ffh_lr_state_advance", blk, None)
            counter += 1
            torch.cuda.synchronize()
            route = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
        yield f"{form}/{entry}", w, S, route


def _inputs(shape, mode):
    import torch
    batch, L, D, rows = shape
    rng = np.random.default_rng(batch * 31 + D + len(rows))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(batch + D)
    idx_np = [[rng.integers(0, R, (batch, L)) for R in rows] for _ in range(STEPS)]
    g_np = [[rng.standard_normal((batch, D)).astype(np.float32) for _ in rows] for _ in range(STEPS)]
    idx = [[torch.from_numpy(i).to(DEV) for i in step] for step in idx_np]
    g = [[torch.from_numpy(x).to(DEV) for x in step] for step in g_np]
    master = []
    for R in rows:
        m = torch.randn((R, D), device=DEV, generator=gen) * 0.1
        master.append(m.bfloat16().view(torch.int16) if mode is not None else m)
    return idx_np, g_np, idx, g, master


def _sparse_case(hip, lr, b16, oracle, rates, shape, route, A, wd=0.0, aggr=capi.AGGR_MODE_SUM, mode=None):
    """Two steps of every form (fused / sort + apply, scalar / _lr entry) from the same start; all end in the reference's bits, and rows nobody
    hit keep w and S bit for bit.  mode: None = fp32 tables, else the bf16 rounding mode."""
    import torch
    batch, L, D, rows = shape
    T = len(rows)
    ws = _ws(hip, T, L, D, batch)
    idx_np, g_np, idx, g, master = _inputs(shape, mode)
    widen = lambda t: t.view(torch.bfloat16).float() if mode is not None else t

    # ---- the reference trajectory of the rows any step hits (everything else must not move)
    hit, w_ref, S_ref = [], [], []
    for t, R in enumerate(rows):
        u = np.unique(np.concatenate([idx_np[s][t].ravel() for s in range(STEPS)]))
        hit.append(u)
        w_ref.append(widen(master[t][torch.from_numpy(u).to(DEV)]).cpu().numpy())
        S_ref.append(np.full(len(u), A, np.float32))
        for s in range(STEPS):
            uniq, sums = _canonical_sums(oracle, idx_np[s][t], g_np[s][t], aggr)
            pos = np.searchsorted(u, uniq)
            wn, Sn = ffmodel.rowwise_adagrad_reference(w_ref[t][pos], sums, S_ref[t][pos], rates[s], EPS, wd)
            if mode is not None:
                wn = B.widen(_round_rows(wn, mode, IT0 + s, 10 + t, uniq))
            w_ref[t][pos], S_ref[t][pos] = wn, Sn

    for what, w, S, got_route in _run_forms(hip, lr, b16, rates, shape, master, idx, g, A, wd, aggr, mode, capi.SPARSE_OPT_ROWWISE_ADAGRAD, 0):
        assert got_route.startswith(route), (got_route, route)      # (ffh_embedding_last_route, read behind every call)
        for t, R in enumerate(rows):
            u = torch.from_numpy(hit[t]).to(DEV)
            gw = widen(w[t][u]).cpu().numpy()
            gS = S[t][u].cpu().numpy()
            assert gS.tobytes() == S_ref[t].tobytes(), f"{what}: table {t}: {np.count_nonzero(gS.view(np.uint32) != S_ref[t].view(np.uint32))} of {gS.size} accumulators differ"
            assert gw.tobytes() == w_ref[t].tobytes(), f"{what}: table {t}: {np.count_nonzero(gw.view(np.uint32) != w_ref[t].view(np.uint32))} of {gw.size} weights differ"
            # rows not hit: w and S bit for bit
            moved = (w[t] != master[t]).any(dim=1) if mode is not None else (_bits(w[t]) != _bits(master[t])).any(dim=1)
            moved |= _bits(S[t]) != _bits(torch.full((1,), A, device=DEV))
            moved[u] = False
            assert not bool(moved.any()), f"{what}: table {t}: {int(moved.sum())} rows nobody hit have moved"
        del w, S
    del ws, master
    torch.cuda.empty_cache()


# (batch, bag, D, rows per table), the route it must take (read off emb_bwd_phases: batch * bag <= 2048: the small kernel; <= 65536 with ids of more
# than 9 bits: the bucket form; above: the LSD sort), aggregation.  Each is the smallest shape that reaches its hazard.
_SHAPES = {
    "small_4_lanes": ((1000, 1, 16, (50, 70_000)), "small", capi.AGGR_MODE_SUM),           # 4 lanes per row, 16 rows per wave
    "d48_12_lanes_fold": ((4096, 1, 48, (3, 50_000)), "buckets:", capi.AGGR_MODE_SUM),      # 12-lane groups, five to a wave, unaligned; the 3-row table folds
    "vec1_13_lanes": ((3000, 1, 13, (40, 5000)), "buckets:", capi.AGGR_MODE_SUM),           # VEC 1, 13-lane groups
    "vec1_70_unequal_trips": ((3000, 1, 70, (40, 5000)), "buckets:", capi.AGGR_MODE_SUM),   # VEC 1, 70 > 64 vectors
    "d256_full_wave_bags": ((4096, 2, 256, (3, 20_000)), "buckets:", capi.AGGR_MODE_SUM),   # exactly one full wave per row, bags
    "d320_lsd_unequal_trips": ((24_000, 3, 320, (100_000, 5)), "lsd:", capi.AGGR_MODE_SUM),   # the LSD route; 80 vectors at VEC 4; folds
    "d512_two_trips": ((2048, 1, 512, (3, 10_000)), "small", capi.AGGR_MODE_SUM),           # two full trips
}


@pytest.mark.parametrize("A", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(_SHAPES))
def test_row_rule_equals_the_restatement_on_the_canonical_sum(hip, lr, b16, oracle, rates, shape, A):
    sh, route, aggr = _SHAPES[shape]
    if shape == "d256_full_wave_bags" and A:
        aggr = capi.AGGR_MODE_AVG      # once
    _sparse_case(hip, lr, b16, oracle, rates, sh, route, A, aggr=aggr)


@pytest.mark.parametrize("shape", ["small_4_lanes", "vec1_13_lanes"])
def test_row_rule_with_weight_decay(hip, lr, b16, oracle, rates, shape):
    sh, route, aggr = _SHAPES[shape]
    _sparse_case(hip, lr, b16, oracle, rates, sh, route, 0.1, wd=1e-3, aggr=aggr)


_SHAPES16 = {
    "small_4_lanes": _SHAPES["small_4_lanes"],
    "d48_12_lanes_fold": _SHAPES["d48_12_lanes_fold"],
    "vec1_13_lanes": _SHAPES["vec1_13_lanes"],
    "d320_lsd_unequal_trips": _SHAPES["d320_lsd_unequal_trips"],
    # more tables in one call than FFH_BF16_MAX_STATEFUL_TABLES (32): that limit is momentum's and Adam's
    "34_tables": ((256, 1, 8, (300,) * 34), "small", capi.AGGR_MODE_SUM),
}


@pytest.mark.parametrize("mode", [B.ROUND_NEAREST, B.ROUND_STOCHASTIC], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("shape", list(_SHAPES16))
def test_row_rule_on_bf16_tables(hip, lr, b16, oracle, rates, shape, mode):
    sh, route, aggr = _SHAPES16[shape]
    _sparse_case(hip, lr, b16, oracle, rates, sh, route, 0.1 if shape == "d320_lsd_unequal_trips" else 0.0, aggr=aggr, mode=mode)


def test_the_cases_cover_every_route():
    """Every case asserts the route its calls reported; taken together they are all three."""
    assert {route for _, route, _ in _SHAPES.values()} == {"small", "buckets:", "lsd:"}
    assert {route for _, route, _ in _SHAPES16.values()} == {"small", "buckets:", "lsd:"}


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_width_one_is_the_element_wise_rule(hip, lr, b16, rates, wd):
    """D == 1 (the entry points accept it): TREE(t) = t[0] and t[0] / 1.0f = t[0], so the row-wise kind and FFH_SPARSE_OPT_ADAGRAD with an [R][1]
    state leave the same bits in w and S."""
    import torch
    shape = (1000, 1, 1, (50,))
    _ws(hip, 1, 1, 1, 1000)
    idx_np, g_np, idx, g, master = _inputs(shape, None)
    out = {}
    for kind, cols in ((capi.SPARSE_OPT_ROWWISE_ADAGRAD, 0), (capi.SPARSE_OPT_ADAGRAD, 1)):
        out[kind] = [(what, w[0].cpu().numpy(), S[0].cpu().numpy().reshape(-1))
                     for what, w, S, _ in _run_forms(hip, lr, b16, rates, shape, master, idx, g, 0.1, wd, capi.AGGR_MODE_SUM, None, kind, cols)]
    for (what, w8, S8), (_, w3, S3) in zip(out[capi.SPARSE_OPT_ROWWISE_ADAGRAD], out[capi.SPARSE_OPT_ADAGRAD]):
        assert w8.tobytes() == w3.tobytes() and S8.tobytes() == S3.tobytes(), what
        assert np.count_nonzero(S8 != np.float32(0.1)) >= 40      # (the update ran)


def test_rows_wider_than_the_registers_hold_are_refused(hip):
    """out_dim 1028 in the 16-byte form (more than four vectors per lane): FFH_ERR_UNSUPPORTED for this kind, nothing launched."""
    import torch
    R, D, batch = 8, 1028, 4
    _ws(hip, 1, 1, D, batch)
    idx = torch.zeros((batch, 1), dtype=torch.int64, device=DEV)
    g, w, S = torch.ones((batch, D), device=DEV), torch.ones((R, D), device=DEV), torch.ones(R, device=DEV)
    opt = _opt(0.1, 0.0)
    rc = hip.lib.ffh_embedding_bwd_opt_fused_multi(hip.ctx, hip.emb_tables([(idx, w, g, R, D)]), hip.emb_states([(S, None)]), 1, 1, D, batch,
                                                   capi.AGGR_MODE_SUM, C.byref(opt), None)
    assert rc not in (0, -1) and "out_dim" in hip.lib.ffh_last_error_string(hip.ctx).decode()
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and bool((S == 1).all())


def test_bad_arguments_launch_nothing(hip, lr, b16):
    """Each returns FFH_ERR_BAD_ARG (-1) and leaves weights and state untouched: missing s0, null states, kinds 4 .. 7 and 9, null opt; the same
    through one _bf16 and one _lr entry."""
    import torch
    R, D, batch = 300, 8, 64
    _ws(hip, 1, 1, D, batch)
    idx = torch.zeros((batch, 1), dtype=torch.int64, device=DEV)
    g = torch.ones((batch, D), device=DEV)
    w = torch.ones((R, D), device=DEV)
    S = torch.ones(R, device=DEV)
    w16 = torch.ones((R, D), dtype=torch.int16, device=DEV)
    tabs = hip.emb_tables([(idx, w, g, R, D)])
    tabs16 = b16.tables([(idx, w16, g, R, D)])
    rnd = b16.rounding(B.ROUND_NEAREST)
    ok, none = hip.emb_states([(S, None)]), hip.emb_states([(None, S)])
    opt = _opt(0.1, 0.0)
    fused, apply_ = hip.lib.ffh_embedding_bwd_opt_fused_multi, hip.lib.ffh_embedding_bwd_opt_apply_multi
    fused16, fused_lr = b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16, lr.lib.ffh_embedding_bwd_opt_fused_multi_lr
    blk = _block(lr)
    assert fused(hip.ctx, tabs, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None) == -1
    assert "s0" in hip.lib.ffh_last_error_string(hip.ctx).decode()
    assert fused(hip.ctx, tabs, None, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None) == -1
    assert fused(hip.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, None, None) == -1
    assert apply_(hip.ctx, tabs, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None) == -1
    for kind in (4, 5, 6, 7, 9):
        unknown = _opt(0.1, 0.0, kind)
        assert fused(hip.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(unknown), None) == -1, kind
        assert "kind" in hip.lib.ffh_last_error_string(hip.ctx).decode()
        assert fused16(b16.ctx, tabs16, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(unknown), C.byref(rnd), None) == -1, kind
        assert fused_lr(lr.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(unknown), capi.ptr(blk), None) == -1, kind
    assert fused16(b16.ctx, tabs16, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), C.byref(rnd), None) == -1
    assert fused16(b16.ctx, tabs16, None, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), C.byref(rnd), None) == -1
    assert fused_lr(lr.ctx, tabs, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), capi.ptr(blk), None) == -1
    assert fused_lr(lr.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, None, capi.ptr(blk), None) == -1
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and bool((S == 1).all()) and bool((w16 == 1).all())
