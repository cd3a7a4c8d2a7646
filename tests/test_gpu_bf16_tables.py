"""bf16 embedding tables on the GPU (include/ff_hip_bf16.h): init, gather and the fused plain-SGD update against the fp32
entry points on the widened table and the numpy restatement of include/ffh_bf16.h (tests/bf16_helpers.py)."""
import ctypes

import numpy as np
import pytest

import bf16_helpers as B
from dlrm_flexflow_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


def _ws(hip, nt, L, D, batch):
    import torch
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(nt, L, D, batch) + 256
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(buf, n)
    return buf


def _widen(w16):
    return w16.view(torch_().bfloat16).float()


def torch_():
    import torch
    return torch


def _rand_bf16(rng, R, D, scale=1.0):
    import torch
    w = (rng.standard_normal((R, D)) * scale).astype(np.float32)
    return torch.from_numpy(B.rne(w).view(np.int16)).to(DEV)


def _bits_equal(a, b):
    return a.view(torch_().int32).equal(b.view(torch_().int32))


def test_init_is_the_rounding_of_init_uniform(hip, b16):
    import torch
    n = 1_000_003
    w32 = torch.empty(n, device=DEV)
    w16 = torch.empty(n, dtype=torch.int16, device=DEV)
    hip.call("ffh_init_uniform", w32, n, 1234, -0.05, 0.05, None)
    b16.call("ffh_init_uniform_bf16", w16, n, 1234, -0.05, 0.05, None)
    torch.cuda.synchronize()
    assert np.array_equal(w16.cpu().numpy().view(np.uint16), B.rne(w32.cpu().numpy()))


def _gather_pair(hip, b16, tabs, L, D, batch, aggr, ld):
    """fp32 gather on the widened tables and bf16 gather: both outputs [batch][ld] per table"""
    import torch
    outs32, outs16, arr32, arr16 = [], [], [], []
    for t, (idx, w16) in enumerate(tabs):
        o32 = torch.full((batch, ld), 7.0, device=DEV)
        o16 = torch.full((batch, ld), 7.0, device=DEV)
        outs32.append(o32); outs16.append(o16)
        arr32.append((idx, _widen(w16), o32, w16.shape[0], ld))
        arr16.append((idx, w16, o16, w16.shape[0], ld))
    a32 = hip.emb_tables(arr32)
    hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, a32, len(tabs), L, D, batch, aggr, None), "fwd32")
    a16 = b16.tables(arr16)
    b16.base.check(b16.lib.ffh_embedding_fwd_multi_bf16(b16.ctx, a16, len(tabs), L, D, batch, aggr, None), "fwd16")
    torch.cuda.synchronize()
    return outs32, outs16


@pytest.mark.parametrize("D", [4, 16, 64, 128, 256, 6])
def test_gather_is_bit_identical_to_the_fp32_gather_on_the_widened_table(hip, b16, D):
    import torch
    rng = np.random.default_rng(D)
    R = 5000
    w16 = _rand_bf16(rng, R, D)
    for L in (1, 3, 8):
        for aggr in (capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG):
            for batch, ld in ((1000, D), (77, D + 4 if D % 4 == 0 else D + 3)):        # ragged tails; ld > D
                idx = torch.from_numpy(rng.integers(0, R, (batch, L))).to(DEV)
                o32, o16 = _gather_pair(hip, b16, [(idx, w16)], L, D, batch, aggr, ld)
                assert _bits_equal(o32[0], o16[0]), (D, L, aggr, batch, ld)


def test_gather_26_tables_one_launch_and_a_table_above_64_mb(hip, b16):
    import torch
    rng = np.random.default_rng(3)
    D, batch, L = 128, 4096, 1
    tabs = []
    for t in range(26):
        R = 300_000 if t == 5 else 1000 + 37 * t                    # table 5: 76.8 MB of bf16 (the nontemporal path)
        w16 = torch.empty(R * D, dtype=torch.int16, device=DEV)
        b16.call("ffh_init_uniform_bf16", w16, R * D, 100 + t, -1.0, 1.0, None)
        tabs.append((torch.from_numpy(rng.integers(0, R, (batch, L))).to(DEV), w16.view(R, D)))
    o32, o16 = _gather_pair(hip, b16, tabs, L, D, batch, capi.AGGR_MODE_SUM, D)
    for t in range(26):
        assert _bits_equal(o32[t], o16[t]), t


def test_gather_from_a_table_of_more_than_2_to_the_31_elements(hip, b16):
    import torch
    R, D, batch, L = 40_000_000, 128, 2048, 2
    w16 = torch.empty(R * D, dtype=torch.int16, device=DEV)
    b16.call("ffh_init_uniform_bf16", w16, R * D, 9, -1.0, 1.0, None)
    w16 = w16.view(R, D)
    rng = np.random.default_rng(4)
    ids = rng.integers(0, R, (batch, L))
    ids[:64, 0] = R - 1 - np.arange(64)                              # rows past element 2^31
    idx = torch.from_numpy(ids).to(DEV)
    o16 = torch.zeros(batch, D, device=DEV)
    a16 = b16.tables([(idx, w16, o16, R, D)])
    b16.base.check(b16.lib.ffh_embedding_fwd_multi_bf16(b16.ctx, a16, 1, L, D, batch, capi.AGGR_MODE_SUM, None), "fwd16")
    rows = w16[idx.view(-1)].view(batch, L, D)
    exp = torch.zeros(batch, D, device=DEV)
    for j in range(L):
        exp = exp + _widen(rows[:, j].contiguous())
    assert _bits_equal(o16, exp)
    del w16, rows
    torch.cuda.empty_cache()


@pytest.mark.parametrize("math_mode", [1, 2], ids=["tensor-op-twin", "split-three-plane"])
def test_gather_writes_the_same_twin_and_three_plane_image(hip, b16, math_mode):
    """tensor-op mode (FFH_MATH_TENSOR_OP_BF16): the registered bf16 twin; split mode (FFH_MATH_FP32_SPLIT_BF16X3): the three-plane image"""
    import torch
    rng = np.random.default_rng(5)
    R, D, batch, L, T = 3000, 64, 512, 3, 2
    tabs = [(torch.from_numpy(rng.integers(0, R, (batch, L))).to(DEV), _rand_bf16(rng, R, D)) for _ in range(T)]
    ld = T * D
    got = {}
    twin_mode = math_mode == 1
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, math_mode) == 0
    try:
        for kind in ("fp32", "bf16"):
            out = torch.zeros(batch, ld, device=DEV)
            n = batch * ld if twin_mode else (out.numel() + 31) // 32 * 96
            side = torch.zeros(n, dtype=torch.int16, device=DEV)
            reg = hip.lib.ffh_ctx_bf16_mirror_set if twin_mode else hip.lib.ffh_ctx_bf16x3_mirror_set
            assert reg(hip.ctx, out.data_ptr(), out.numel() * 4, side.data_ptr()) == 0
            try:
                if kind == "fp32":
                    a = hip.emb_tables([(i, _widen(w), out[:, t * D:], R, ld) for t, (i, w) in enumerate(tabs)])
                    hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, a, T, L, D, batch, capi.AGGR_MODE_AVG, None), "fwd32")
                else:
                    a = b16.tables([(i, w, out[:, t * D:], R, ld) for t, (i, w) in enumerate(tabs)])
                    b16.base.check(b16.lib.ffh_embedding_fwd_multi_bf16(b16.ctx, a, T, L, D, batch, capi.AGGR_MODE_AVG, None), "fwd16")
                torch.cuda.synchronize()
            finally:
                assert reg(hip.ctx, out.data_ptr(), out.numel() * 4, None) == 0
            got[kind] = (out, side)
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
    assert bool((got["fp32"][1] != 0).any())            # the gather did write the twin / image
    for x, y in zip(got["fp32"], got["bf16"]):
        assert x.view(-1).view(torch.int16).equal(y.view(-1).view(torch.int16))


# --------------------------------------------------------------------------------------------------------------------------------
# fused update
# --------------------------------------------------------------------------------------------------------------------------------
def _zipf_ids(rng, R, n):
    return np.minimum(rng.zipf(1.2, n) - 1, R - 1).astype(np.int64)


def _update_case(hip, b16, shape, mode, two_phase, seed=77):
    """one bf16 update vs the fp32 update on the widened tables + the rounding restated in numpy"""
    import torch
    T, R, D, batch, L, route = shape
    rng = np.random.default_rng(hash((R, D, batch, L, mode, two_phase)) % 2**32)
    tabs = []
    for t in range(T):
        ids = _zipf_ids(rng, R, batch * L).reshape(batch, L)
        ids[: batch // 4] = rng.integers(0, R, (batch // 4, L))
        tabs.append((torch.from_numpy(ids).to(DEV), _rand_bf16(rng, R, D, 0.05)))
    ld = T * D
    G = torch.from_numpy(rng.standard_normal((batch, ld)).astype(np.float32)).to(DEV)
    lr = 0.01
    _ws(hip, T, L, D, batch)
    w32 = [_widen(w) for _, w in tabs]
    a32 = hip.emb_tables([(i, w32[t], G[:, t * D:], R, ld) for t, (i, _) in enumerate(tabs)])
    hip.check(hip.lib.ffh_embedding_bwd_sgd_fused_multi(hip.ctx, a32, T, L, D, batch, capi.AGGR_MODE_SUM, lr, None), "fused32")
    counter = torch.tensor([5], dtype=torch.int64, device=DEV)
    new16 = [w.clone() for _, w in tabs]
    table_ids = [3 * t + 1 for t in range(T)]
    a16 = b16.tables([(i, new16[t], G[:, t * D:], R, ld, table_ids[t], 0) for t, (i, _) in enumerate(tabs)])
    rnd = b16.rounding(mode, seed, counter)
    if two_phase:
        b16.base.check(b16.lib.ffh_embedding_bwd_sort_multi_bf16(b16.ctx, a16, T, L, D, batch, None), "sort16")
        b16.base.check(b16.lib.ffh_embedding_bwd_sgd_apply_multi_bf16(b16.ctx, a16, T, L, D, batch, capi.AGGR_MODE_SUM, lr, ctypes.byref(rnd), None), "apply16")
    else:
        b16.base.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, a16, T, L, D, batch, capi.AGGR_MODE_SUM, lr, ctypes.byref(rnd), None), "fused16")
    torch.cuda.synchronize()
    got_route = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
    assert got_route.startswith(route), got_route
    for t in range(T):
        exp = B.round_table(w32[t].cpu().numpy(), mode, seed, 5, table_ids[t])
        got = new16[t].cpu().numpy().view(np.uint16)
        assert np.array_equal(got, exp), (shape, mode, two_phase, t, int((got != exp).sum()))
        touched = np.zeros(R, bool)
        touched[tabs[t][0].cpu().numpy().ravel()] = True
        assert np.array_equal(got[~touched], tabs[t][1].cpu().numpy().view(np.uint16)[~touched])
        assert (got[touched] != tabs[t][1].cpu().numpy().view(np.uint16)[touched]).any()


# (T, R, D, batch, L, route prefix)
_FORMS = [(4, 1000, 16, 512, 1, "small"), (3, 200_000, 128, 40_000, 3, "lsd:"), (4, 100_000, 64, 16_384, 1, "buckets:"),
          (2, 2000, 6, 700, 2, "small"), (2, 300_000, 128, 70_000, 1, "lsd:"),
          (2, 200_000, 6, 70_000, 1, "lsd:"), (2, 100_000, 5, 16_384, 1, "buckets:")]          # odd D: the one-element form


@pytest.mark.parametrize("shape", _FORMS, ids=lambda s: f"{s[5]}{s[2]}x{s[1]}")
@pytest.mark.parametrize("mode", [B.ROUND_STOCHASTIC, B.ROUND_NEAREST], ids=["stochastic", "nearest"])
def test_update_matches_fp32_update_then_rounding(hip, b16, shape, mode):
    _update_case(hip, b16, shape, mode, two_phase=False)
    _update_case(hip, b16, shape, mode, two_phase=True)


@pytest.mark.parametrize("cut", [16, 13], ids=["col0-16", "col0-13"])
def test_update_column_slice_uses_global_columns(hip, b16, cut):
    """a column slice (col0 > 0) draws the bits of its global columns: the two slices of a table updated one call each equal the whole
    (col0 = 13: the groups of four columns straddle the cut, and the 13- and 19-wide slices take the one-element form)"""
    import torch
    rng = np.random.default_rng(11)
    R, D, batch = 4000, 32, 1024
    idx = torch.from_numpy(rng.integers(0, R, (batch, 1))).to(DEV)
    w = _rand_bf16(rng, R, D, 0.05)
    G = torch.from_numpy(rng.standard_normal((batch, D)).astype(np.float32)).to(DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    rnd = b16.rounding(B.ROUND_STOCHASTIC, 3, counter)
    whole = w.clone()
    _ws(hip, 1, 1, D, batch)

    def upd(wt, g, width, col0):
        b16.base.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, b16.tables([(idx, wt, g, R, D, 7, col0)]), 1, 1, width, batch,
                                                                       capi.AGGR_MODE_SUM, 0.1, ctypes.byref(rnd), None), "upd")
    upd(whole, G, D, 0)
    lo, hi = w[:, :cut].contiguous(), w[:, cut:].contiguous()
    upd(lo, G, cut, 0)
    upd(hi, G[:, cut:], D - cut, cut)
    torch.cuda.synchronize()
    assert not whole.equal(w)
    assert torch.cat([lo, hi], 1).equal(whole)


def _one_update(b16, w, idx, G, R, D, batch, counter, lr=0.01, stream=None):
    rnd = b16.rounding(B.ROUND_STOCHASTIC, 99, counter)
    b16._keep = rnd
    b16.base.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, b16.tables([(idx, w, G, R, D)]), 1, 1, D, batch,
                                                                   capi.AGGR_MODE_SUM, lr, ctypes.byref(rnd), stream), "fused16")
    b16.call("ffh_bf16_counter_advance", counter, stream)


def test_counter_advances_and_graph_replay_draws_fresh_bits(hip, b16):
    import torch
    rng = np.random.default_rng(12)
    R, D, batch = 3000, 64, 2048
    idx = torch.from_numpy(rng.integers(0, R, (batch, 1))).to(DEV)
    G = torch.from_numpy(rng.standard_normal((batch, D)).astype(np.float32) * 1e-3).to(DEV)
    w0 = _rand_bf16(rng, R, D, 0.05)
    _ws(hip, 1, 1, D, batch)
    # two successive updates with identical inputs use different bits
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    a, b = w0.clone(), w0.clone()
    _one_update(b16, a, idx, G, R, D, batch, counter)
    _one_update(b16, b, idx, G, R, D, batch, counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 2 and not a.equal(b)
    # three updates captured in one graph and replayed == three eager updates
    eager = w0.clone()
    c_e = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(3):
        _one_update(b16, eager, idx, G, R, D, batch, c_e)
    torch.cuda.synchronize()
    graphed = w0.clone()
    c_g = torch.zeros(1, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p()
    hip.check(hip.lib.ffh_stream_create(hip.ctx, ctypes.byref(s)), "stream")
    g = ctypes.c_void_p()
    try:
        hip.check(hip.lib.ffh_ctx_reserve_scratch(hip.ctx, s), "scratch")
        hip.check(hip.lib.ffh_graph_begin_capture(hip.ctx, s), "begin")
        for _ in range(3):
            _one_update(b16, graphed, idx, G, R, D, batch, c_g, stream=s.value)
        hip.check(hip.lib.ffh_graph_end_capture(hip.ctx, s, ctypes.byref(g)), "end")
        assert graphed.equal(w0) and int(c_g.item()) == 0            # captured, not run
        hip.check(hip.lib.ffh_graph_launch(hip.ctx, g, s), "launch")
        hip.check(hip.lib.ffh_stream_sync(hip.ctx, s), "sync")
    finally:
        if g.value:
            hip.lib.ffh_graph_destroy(hip.ctx, g)
        hip.lib.ffh_stream_destroy(hip.ctx, s)
    assert int(c_g.item()) == 3
    assert graphed.equal(eager)


def test_updates_below_half_an_ulp_nearest_stays_stochastic_is_unbiased(hip, b16):
    import torch
    R, D, K, lr, g = 4096, 16, 16, 1e-3, -1.0                           # 65,536 elements, 16 steps of +1e-3 at 1.0 (half an ulp: 2^-8)
    idx = torch.arange(R, dtype=torch.int64, device=DEV).view(R, 1)
    G = torch.full((R, D), g, device=DEV)
    one = torch.full((R, D), 0x3F80, dtype=torch.int16, device=DEV)
    _ws(hip, 1, 1, D, R)
    res = {}
    for mode in (B.ROUND_NEAREST, B.ROUND_STOCHASTIC):
        w = one.clone()
        counter = torch.zeros(1, dtype=torch.int64, device=DEV)
        rnd = b16.rounding(mode, 2024, counter)
        for _ in range(K):
            b16.base.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, b16.tables([(idx, w, G, R, D)]), 1, 1, D, R,
                                                                           capi.AGGR_MODE_SUM, lr, ctypes.byref(rnd), None), "upd")
            b16.call("ffh_bf16_counter_advance", counter, None)
        torch.cuda.synchronize()
        res[mode] = _widen(w).double().cpu().numpy()
    assert np.all(res[B.ROUND_NEAREST] == 1.0)
    x = res[B.ROUND_STOCHASTIC]
    sigma = x.std() / np.sqrt(x.size)
    assert abs(x.mean() - (1.0 + K * lr)) <= 4 * sigma, (x.mean(), 1.0 + K * lr, sigma)
    assert x.std() > 0


def test_bad_arguments_are_refused_with_a_message(hip, b16):
    import torch
    w = torch.zeros(10, 4, dtype=torch.int16, device=DEV)
    idx = torch.zeros(4, 1, dtype=torch.int64, device=DEV)
    G = torch.zeros(4, 4, device=DEV)
    _ws(hip, 1, 1, 4, 4)
    a = b16.tables([(idx, w, G, 10, 4)])
    rnd = b16.rounding(B.ROUND_STOCHASTIC, 0, None)
    rc = b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, a, 1, 1, 4, 4, capi.AGGR_MODE_SUM, 0.1, ctypes.byref(rnd), None)
    assert rc == capi.FFH_ERR_BAD_ARG and b"counter" in hip.lib.ffh_last_error_string(hip.ctx)
    bad = b16.rounding(7, 0, None)
    rc = b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, a, 1, 1, 4, 4, capi.AGGR_MODE_SUM, 0.1, ctypes.byref(bad), None)
    assert rc == capi.FFH_ERR_BAD_ARG and b"rounding mode" in hip.lib.ffh_last_error_string(hip.ctx)
