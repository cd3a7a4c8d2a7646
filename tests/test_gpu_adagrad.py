"""Adagrad on the GPU (include/ff_hip_adagrad.h): the dense launch and the row rule of the fused table update, bit for bit against
ffmodel.adagrad_reference (one float32 numpy operation per rounded operation).  The sparse rule's gradient is the row's canonical sum, taken
from code that is not under test: the CPU oracle's plain-SGD fused update with lr = -1 on an all-zero table, which leaves w = fmaf(1, sum, 0) = sum.
(The oracle walks the sorted (row, position) list and cuts it at absolute positions of that list, so renaming the rows by their rank among the
rows hit -- a monotone map -- leaves every sum as it is: the reference table has one row per row hit, not 4,000,000.)
The model-level tests are tests/test_gpu_adagrad_model.py."""
import ctypes as C

import numpy as np
import pytest

import bf16_helpers as B
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xADA6
EPS = 1e-10
ZERO_GRAD = 1      # FFH_OPT_ZERO_GRAD


@pytest.fixture(scope="module")
def ag(hip):
    return capi.adagrad_api(hip)


@pytest.fixture(scope="module")
def lr(hip):
    return capi.lr_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


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
    for _ in range(3):
        out.append(float(np.float32(lr.read(blk).lr)))
        lr.call("ffh_lr_state_advance", blk, None)
    assert len(set(out)) == 3, out
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


# =====================================================================================================================================
# 5. the dense kernel
# =====================================================================================================================================
@pytest.mark.parametrize("entry", ["scalar", "lr"])
@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (4, 0), (7, 0), (1024, 0), (1027, 0), (65536 + 4, 0), (1024, 1)],
                         ids=lambda v: str(v))
def test_dense_kernel_equals_the_restatement(hip, ag, lr, rates, entry, n, offset):
    """n % 4 == 0 at 16-byte alignment: the vector form; otherwise (odd n, or offset = 1 element) the scalar form.  3 consecutive steps, with
    and without weight decay and FFH_OPT_ZERO_GRAD; the elements around the range keep their bits."""
    import torch
    rng = np.random.default_rng(n * 13 + offset)
    pad = 8
    for wd in (0.0, 1e-3):
        for zg in (0, ZERO_GRAD):
            w0 = rng.standard_normal(n + 2 * pad).astype(np.float32)
            S0 = np.abs(rng.standard_normal(n + 2 * pad)).astype(np.float32) * np.float32(0.01)
            lo, hi = pad + offset, pad + offset + n
            w, S = torch.from_numpy(w0).to(DEV), torch.from_numpy(S0).to(DEV)
            wr, Sr = w0[lo:hi].copy(), S0[lo:hi].copy()
            blk = _block(lr)
            for step in range(3):
                g0 = rng.standard_normal(n + 2 * pad).astype(np.float32)
                g0[lo:hi][::5] = 0.0
                g = torch.from_numpy(g0).to(DEV)
                if entry == "lr":
                    ag.call("ffh_adagrad_update_lr", w[lo:], g[lo:], S[lo:], n, blk, EPS, wd, zg, None)
                    lr.call("ffh_lr_state_advance", blk, None)
                else:
                    ag.call("ffh_adagrad_update", w[lo:], g[lo:], S[lo:], n, rates[step], EPS, wd, zg, None)
                torch.cuda.synchronize()
                wr, Sr = ffmodel.adagrad_reference(wr, g0[lo:hi], Sr, rates[step], EPS, wd)
                gw, gS, gg = w.cpu().numpy(), S.cpu().numpy(), g.cpu().numpy()
                what = f"n={n} wd={wd} zero_grad={zg} step={step}"
                assert gw[lo:hi].tobytes() == wr.tobytes(), f"w: {what}: {np.count_nonzero(gw[lo:hi].view(np.uint32) != wr.view(np.uint32))} differ"
                assert gS[lo:hi].tobytes() == Sr.tobytes(), f"S: {what}"
                assert gg[lo:hi].tobytes() == (np.zeros(n, np.float32) if zg else g0[lo:hi]).tobytes(), f"g: {what}"
                for got, before in ((gw, w0), (gS, S0), (gg, g0)):
                    assert got[:lo].tobytes() == before[:lo].tobytes() and got[hi:].tobytes() == before[hi:].tobytes(), f"outside the range: {what}"


def test_dense_kernel_bad_arguments(hip, ag, lr):
    import torch
    w = torch.ones(8, device=DEV)
    before = w.clone()
    assert ag.rc("ffh_adagrad_update", w, w, None, 8, 0.1, EPS, 0.0, 0, None) == -1
    assert ag.rc("ffh_adagrad_update", w, w, w, 8, 0.1, EPS, 0.0, 2, None) == -1
    assert ag.rc("ffh_adagrad_update", w, w, w, -1, 0.1, EPS, 0.0, 0, None) == -1
    assert ag.rc("ffh_adagrad_update_lr", w, w, w, 8, None, EPS, 0.0, 0, None) == -1
    assert ag.rc("ffh_adagrad_update", None, None, None, 0, 0.1, EPS, 0.0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(w, before)
    assert ag.lib.ffh_adagrad_abi_version() == capi.adagrad_header_abi_version()


# =====================================================================================================================================
# 14 (kernel side). the mirrors of a weight range in the bf16-pipe modes
# =====================================================================================================================================
@pytest.mark.parametrize("math_mode", [1, 2], ids=["tensor-op-twin", "split-three-plane"])
@pytest.mark.parametrize("entry", ["scalar", "lr"])
def test_dense_kernel_keeps_the_twin_and_the_three_plane_image(hip, ag, lr, rates, math_mode, entry):
    """After the update the registered bf16 twin / three-plane image of the weights is what a fresh conversion of the updated fp32 weights
    gives (ffh_convert_f32_to_bf16 / _bf16x3), bit for bit: the vector form writes it in the same launch, the scalar form (a misaligned
    sub-range) by the conversion behind it."""
    import torch
    rng = np.random.default_rng(math_mode)
    n = 4096
    twin_mode = math_mode == 1
    reg = hip.lib.ffh_ctx_bf16_mirror_set if twin_mode else hip.lib.ffh_ctx_bf16x3_mirror_set
    side_n = n if twin_mode else n // 32 * 96

    def convert(w, side):
        if twin_mode:
            hip.check(hip.lib.ffh_convert_f32_to_bf16(hip.ctx, side.data_ptr(), w.data_ptr(), n, None), "convert")
        else:
            hip.check(hip.lib.ffh_convert_f32_to_bf16x3(hip.ctx, w.data_ptr(), 1, n, n, None), "convert x3")

    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, math_mode) == 0
    try:
        for lo, cnt in ((0, n), (1, n - 5)):      # the whole range (vector form); a misaligned part of it (scalar form + conversion)
            w = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
            g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
            S = torch.zeros(n, device=DEV)
            side = torch.zeros(side_n, dtype=torch.int16, device=DEV)
            assert reg(hip.ctx, w.data_ptr(), n * 4, side.data_ptr()) == 0
            try:
                convert(w, side)
                torch.cuda.synchronize()
                stale = side.clone()
                if entry == "lr":
                    ag.call("ffh_adagrad_update_lr", w[lo:], g[lo:], S[lo:], cnt, _block(lr), EPS, 1e-3, ZERO_GRAD, None)
                else:
                    ag.call("ffh_adagrad_update", w[lo:], g[lo:], S[lo:], cnt, rates[0], EPS, 1e-3, ZERO_GRAD, None)
                torch.cuda.synchronize()
                got = side.clone()
                convert(w, side)
                torch.cuda.synchronize()
                assert torch.equal(got, side), f"{int((got != side).sum())} of {side_n} mirror words are stale"
                assert not torch.equal(got, stale)
            finally:
                assert reg(hip.ctx, w.data_ptr(), n * 4, None) == 0
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0


# =====================================================================================================================================
# 6 / 7. the sparse rule on fp32 and bf16 tables
# =====================================================================================================================================
def _ws(hip, nt, L, D, batch):
    import torch
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(nt, L, D, batch) + 256
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(buf, n)
    return buf


def _opt(lr_value, wd):
    o = capi.SparseOpt()
    o.kind = capi.SPARSE_OPT_ADAGRAD
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


_FORMS = [("fused", "scalar"), ("apply", "scalar"), ("fused", "lr"), ("apply", "lr")]
STEPS = 2
IT0 = 5      # the bf16 update counter's value at the first step


def _sparse_case(hip, lr, b16, oracle, rates, shape, route, A, wd=0.0, aggr=capi.AGGR_MODE_SUM, mode=None):
    """Two steps of every form (fused / sort + apply, scalar / _lr entry) from the same start; all end in the reference's bits.  mode: None =
    fp32 tables, else the bf16 rounding mode."""
    import torch
    batch, L, D, rows = shape
    T = len(rows)
    rng = np.random.default_rng(batch * 31 + D + T)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(batch + D)
    ws = _ws(hip, T, L, D, batch)
    idx_np = [[rng.integers(0, R, (batch, L)) for R in rows] for _ in range(STEPS)]
    g_np = [[rng.standard_normal((batch, D)).astype(np.float32) for _ in rows] for _ in range(STEPS)]
    idx = [[torch.from_numpy(i).to(DEV) for i in step] for step in idx_np]
    g = [[torch.from_numpy(x).to(DEV) for x in step] for step in g_np]
    master = []
    for R in rows:
        m = torch.randn((R, D), device=DEV, generator=gen) * 0.1
        master.append(m.bfloat16().view(torch.int16) if mode is not None else m)
    widen = lambda t: t.view(torch.bfloat16).float() if mode is not None else t

    # ---- the reference trajectory of the rows any step hits (everything else must not move)
    hit, w_ref, S_ref = [], [], []
    for t, R in enumerate(rows):
        u = np.unique(np.concatenate([idx_np[s][t].ravel() for s in range(STEPS)]))
        hit.append(u)
        w_ref.append(widen(master[t][torch.from_numpy(u).to(DEV)]).cpu().numpy())
        S_ref.append(np.full((len(u), D), A, np.float32))
        for s in range(STEPS):
            uniq, sums = _canonical_sums(oracle, idx_np[s][t], g_np[s][t], aggr)
            pos = np.searchsorted(u, uniq)
            wn, Sn = ffmodel.adagrad_reference(w_ref[t][pos], sums, S_ref[t][pos], rates[s], EPS, wd)
            if mode is not None:
                wn = B.widen(_round_rows(wn, mode, IT0 + s, 10 + t, uniq))
            w_ref[t][pos], S_ref[t][pos] = wn, Sn

    for form, entry in _FORMS:
        w = [m.clone() for m in master]
        S = [torch.full((R, D), A, device=DEV) for R in rows]
        st = hip.emb_states([(S[t], None) for t in range(T)])
        blk = _block(lr)
        counter = torch.tensor([IT0], dtype=torch.int64, device=DEV)
        for s in range(STEPS):
            opt = _opt(rates[s] if entry == "scalar" else 123.0, wd)      # (the _lr entries ignore opt.lr)
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
            got_route = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
            assert got_route.startswith(route), (got_route, route)
        what = f"{form}/{entry}"
        for t, R in enumerate(rows):
            u = torch.from_numpy(hit[t]).to(DEV)
            gw = widen(w[t][u]).cpu().numpy()
            gS = S[t][u].cpu().numpy()
            assert gw.tobytes() == w_ref[t].tobytes(), f"{what}: table {t}: {np.count_nonzero(gw.view(np.uint32) != w_ref[t].view(np.uint32))} of {gw.size} weights differ"
            assert gS.tobytes() == S_ref[t].tobytes(), f"{what}: table {t}: {np.count_nonzero(gS.view(np.uint32) != S_ref[t].view(np.uint32))} of {gS.size} accumulators differ"
            # rows not hit: w and S bit for bit
            moved = (w[t] != master[t]).any(dim=1) if mode is not None else (_bits(w[t]) != _bits(master[t])).any(dim=1)
            moved |= (_bits(S[t]) != _bits(torch.full((1, D), A, device=DEV))).any(dim=1)
            moved[u] = False
            assert not bool(moved.any()), f"{what}: table {t}: {int(moved.sum())} rows nobody hit have moved"
        del w, S
    del ws, master
    torch.cuda.empty_cache()


# (batch, bag, D, rows per table), the route it must take, aggregation
_SHAPES = {
    "tiles_folds_single_hits": ((32768, 1, 128, (4_000_000, 3, 977)), "buckets:", capi.AGGR_MODE_SUM),
    "bags": ((4096, 2, 64, (100_000, 17)), "buckets:", capi.AGGR_MODE_SUM),
    "small": ((1000, 1, 16, (50, 70_000)), "small", capi.AGGR_MODE_SUM),
    "vec1": ((3000, 1, 13, (40, 5000)), "buckets:", capi.AGGR_MODE_SUM),
    "d512_lsd": ((24_000, 3, 512, (200_000, 5)), "lsd:", capi.AGGR_MODE_SUM),
}


@pytest.mark.parametrize("A", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(_SHAPES))
def test_sparse_rule_equals_the_restatement_on_the_canonical_sum(hip, lr, b16, oracle, rates, shape, A):
    sh, route, aggr = _SHAPES[shape]
    if shape == "bags" and A:
        aggr = capi.AGGR_MODE_AVG      # once
    _sparse_case(hip, lr, b16, oracle, rates, sh, route, A, aggr=aggr)


@pytest.mark.parametrize("shape", ["small", "vec1"])
def test_sparse_rule_with_weight_decay(hip, lr, b16, oracle, rates, shape):
    sh, route, aggr = _SHAPES[shape]
    _sparse_case(hip, lr, b16, oracle, rates, sh, route, 0.1, wd=1e-3, aggr=aggr)


_SHAPES16 = {
    "bags": _SHAPES["bags"],
    "small": _SHAPES["small"],
    "vec1": _SHAPES["vec1"],
    "lsd": ((24_000, 3, 128, (200_000, 5)), "lsd:", capi.AGGR_MODE_SUM),
    # more tables in one call than FFH_BF16_MAX_STATEFUL_TABLES (32): that limit is momentum's and Adam's
    "34_tables": ((256, 1, 8, (300,) * 34), "small", capi.AGGR_MODE_SUM),
}


@pytest.mark.parametrize("mode", [B.ROUND_NEAREST, B.ROUND_STOCHASTIC], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("shape", list(_SHAPES16))
def test_sparse_rule_on_bf16_tables(hip, lr, b16, oracle, rates, shape, mode):
    sh, route, aggr = _SHAPES16[shape]
    _sparse_case(hip, lr, b16, oracle, rates, sh, route, 0.1 if shape == "lsd" else 0.0, aggr=aggr, mode=mode)


# =====================================================================================================================================
# 8. bad arguments
# =====================================================================================================================================
def test_sparse_rule_bad_arguments_launch_nothing(hip, lr, b16):
    import torch
    R, D, batch = 300, 8, 64
    _ws(hip, 1, 1, D, batch)
    idx = torch.zeros((batch, 1), dtype=torch.int64, device=DEV)
    g = torch.ones((batch, D), device=DEV)
    w = torch.ones((R, D), device=DEV)
    S = torch.ones((R, D), device=DEV)
    w16 = torch.ones((R, D), dtype=torch.int16, device=DEV)
    tabs = hip.emb_tables([(idx, w, g, R, D)])
    tabs16 = b16.tables([(idx, w16, g, R, D)])
    rnd = b16.rounding(B.ROUND_NEAREST)
    ok, none = hip.emb_states([(S, None)]), hip.emb_states([(None, S)])
    opt = _opt(0.1, 0.0)
    unknown = _opt(0.1, 0.0)
    unknown.kind = capi.SPARSE_OPT_ADAGRAD + 1
    fused, apply_ = hip.lib.ffh_embedding_bwd_opt_fused_multi, hip.lib.ffh_embedding_bwd_opt_apply_multi
    assert fused(hip.ctx, tabs, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None) == -1
    assert "s0" in hip.lib.ffh_last_error_string(hip.ctx).decode()
    assert fused(hip.ctx, tabs, None, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None) == -1
    assert fused(hip.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(unknown), None) == -1
    assert fused(hip.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, None, None) == -1
    assert apply_(hip.ctx, tabs, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None) == -1
    assert b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, tabs16, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), C.byref(rnd), None) == -1
    assert b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, tabs16, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(unknown), C.byref(rnd), None) == -1
    blk = _block(lr)
    assert lr.lib.ffh_embedding_bwd_opt_fused_multi_lr(lr.ctx, tabs, none, 1, 1, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), capi.ptr(blk), None) == -1
    assert lr.lib.ffh_embedding_bwd_opt_fused_multi_lr(lr.ctx, tabs, ok, 1, 1, D, batch, capi.AGGR_MODE_SUM, None, capi.ptr(blk), None) == -1
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and bool((S == 1).all()) and bool((w16 == 1).all())
