"""Momentum / weight-decay SGD and Adam on bf16 tables (ffh_embedding_bwd_opt_{fused,apply}_multi_bf16, include/ff_hip_bf16.h version 2)
against the fp32 entry ffh_embedding_bwd_opt_fused_multi on the widened table: the table is the rounding (tests/bf16_helpers.py) of the
fp32 entry's result and the fp32 state is bit-identical to the fp32 entry's state, over the small, lsd and bucket routes, fused vs sort +
apply, a column slice (col0 != 0) and the largest table count the stateful entries take."""
import numpy as np
import pytest

import bf16_helpers as B
from dlrm_flexflow_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED_BF16


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


def _ws(hip, nt, L, D, batch):
    import torch
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(nt, L, D, batch) + 256
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(buf, n)
    return buf


def _opt(kind, **kw):
    o = capi.SparseOpt()
    o.kind = kind
    o.lr = kw.get("lr", 0.05)
    o.weight_decay = kw.get("wd", 0.0)
    o.momentum = kw.get("mom", 0.0)
    o.nesterov = 1 if kw.get("nesterov") else 0
    o.beta1, o.beta2, o.epsilon = 0.9, 0.999, 1e-8
    return o


def _run(hip, b16, T, R, D, batch, L, opt, mode, fused=True, col0=0, it=3, route=None):
    """One update of T tables by both entries; returns nothing, asserts bits."""
    import torch
    rng = np.random.default_rng(T * 7 + R + D + batch)
    ws = _ws(hip, T, L, D, batch)
    idx = [torch.from_numpy(rng.integers(0, R, (batch, L))).to(DEV) for _ in range(T)]
    g = [torch.from_numpy(rng.standard_normal((batch, D)).astype(np.float32)).to(DEV) for _ in range(T)]
    w16 = [torch.from_numpy(B.rne(rng.standard_normal((R, D)).astype(np.float32) * 0.1).view(np.int16)).to(DEV) for _ in range(T)]
    w32 = [w.view(torch.bfloat16).float().contiguous() for w in w16]
    nstate = 2 if opt.kind == capi.SPARSE_OPT_ADAM else (1 if opt.momentum > 0 else 0)
    init = [[torch.from_numpy(np.abs(rng.standard_normal((R, D))).astype(np.float32) * 0.01).to(DEV) for _ in range(nstate)] for _ in range(T)]
    s32 = [[s.clone() for s in st] for st in init]
    s16 = [[s.clone() for s in st] for st in init]
    st = lambda S: hip.emb_states([(S[t][0] if nstate > 0 else None, S[t][1] if nstate > 1 else None) for t in range(T)])
    a32 = hip.emb_tables([(idx[t], w32[t], g[t], R, D) for t in range(T)])
    hip.check(hip.lib.ffh_embedding_bwd_opt_fused_multi(hip.ctx, a32, st(s32), T, L, D, batch, capi.AGGR_MODE_SUM, opt, None), "opt32")
    counter = torch.tensor([it], dtype=torch.int64, device=DEV)
    rnd = b16.rounding(mode, SEED, counter)
    a16 = b16.tables([(idx[t], w16[t], g[t], R, D, 10 + t, col0) for t in range(T)])
    if fused:
        b16.base.check(b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, a16, st(s16), T, L, D, batch, capi.AGGR_MODE_SUM, opt, rnd, None), "opt16")
    else:
        b16.base.check(b16.lib.ffh_embedding_bwd_sort_multi_bf16(b16.ctx, a16, T, L, D, batch, None), "sort16")
        b16.base.check(b16.lib.ffh_embedding_bwd_opt_apply_multi_bf16(b16.ctx, a16, st(s16), T, L, D, batch, capi.AGGR_MODE_SUM, opt, rnd, None), "apply16")
    torch.cuda.synchronize()
    if route:
        got = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
        assert got.startswith(route), got
    for t in range(T):
        want = B.round_table(w32[t].cpu().numpy(), mode, SEED, it=it, table=10 + t, col0=col0)
        got = w16[t].cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), f"table {t}: {np.count_nonzero(got != want)} of {got.size} differ"
        for k in range(nstate):
            assert torch.equal(s32[t][k].view(torch.int32), s16[t][k].view(torch.int32)), f"state {k} of table {t}"
    del ws


_RULES = {
    "momentum": lambda: _opt(capi.SPARSE_OPT_SGD_MOMENTUM, mom=0.9),
    "momentum_nesterov_wd": lambda: _opt(capi.SPARSE_OPT_SGD_MOMENTUM, mom=0.9, nesterov=True, wd=1e-3),
    "wd_only": lambda: _opt(capi.SPARSE_OPT_SGD_MOMENTUM, wd=1e-2),
    "adam": lambda: _opt(capi.SPARSE_OPT_ADAM, lr=0.01, wd=1e-4),
}
# (T, R, D, batch, L, route prefix)
_FORMS = [(4, 1000, 16, 512, 1, "small"), (3, 200_000, 128, 40_000, 3, "lsd:"), (4, 100_000, 64, 16_384, 1, "buckets:"), (2, 2000, 6, 700, 2, "small")]


@pytest.mark.parametrize("rule", list(_RULES))
@pytest.mark.parametrize("shape", _FORMS, ids=[f[-1].rstrip(":") + f"_D{f[2]}" for f in _FORMS])
@pytest.mark.parametrize("mode", [B.ROUND_NEAREST, B.ROUND_STOCHASTIC], ids=["nearest", "stochastic"])
def test_stateful_update_is_the_fp32_update_then_rounding(hip, b16, rule, shape, mode):
    T, R, D, batch, L, route = shape
    _run(hip, b16, T, R, D, batch, L, _RULES[rule](), mode, route=route)


@pytest.mark.parametrize("rule", ["momentum_nesterov_wd", "adam"])
@pytest.mark.parametrize("shape", [_FORMS[0], _FORMS[2]], ids=["small", "buckets"])
def test_sort_then_apply_equals_fused_and_column_slice_keys(hip, b16, rule, shape):
    T, R, D, batch, L, route = shape
    _run(hip, b16, T, R, D, batch, L, _RULES[rule](), B.ROUND_STOCHASTIC, fused=False, col0=D * 3, route=route)


@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_largest_table_count_and_the_refusal_above_it(hip, b16, rule):
    import torch
    n = 32
    _run(hip, b16, n, 300, 8, 256, 1, _RULES[rule](), B.ROUND_STOCHASTIC, route="small")
    # one more table: FFH_ERR_BAD_ARG, nothing launched
    _ws(hip, n + 1, 1, 8, 16)
    idx = torch.zeros((16, 1), dtype=torch.int64, device=DEV)
    g = torch.zeros((16, 8), device=DEV)
    w = torch.zeros((300, 8), dtype=torch.int16, device=DEV)
    s = torch.zeros((300, 8), device=DEV)
    a16 = b16.tables([(idx, w, g, 300, 8)] * (n + 1))
    st = hip.emb_states([(s, s)] * (n + 1))
    rc = b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, a16, st, n + 1, 1, 8, 16, capi.AGGR_MODE_SUM, _RULES[rule](),
                                                        b16.rounding(B.ROUND_NEAREST), None)
    assert rc != 0 and "32" in hip.lib.ffh_last_error_string(hip.ctx).decode()


@pytest.mark.parametrize("shape", [_FORMS[0], _FORMS[1], _FORMS[2]], ids=["small", "lsd", "buckets"])
def test_sgd_kind_equals_the_bf16_sgd_entry(hip, b16, shape):
    import torch
    T, R, D, batch, L, route = shape
    rng = np.random.default_rng(R)
    ws = _ws(hip, T, L, D, batch)
    idx = [torch.from_numpy(rng.integers(0, R, (batch, L))).to(DEV) for _ in range(T)]
    g = [torch.from_numpy(rng.standard_normal((batch, D)).astype(np.float32)).to(DEV) for _ in range(T)]
    wa = [torch.from_numpy(B.rne(rng.standard_normal((R, D)).astype(np.float32)).view(np.int16)).to(DEV) for _ in range(T)]
    wb = [w.clone() for w in wa]
    counter = torch.tensor([5], dtype=torch.int64, device=DEV)
    rnd = b16.rounding(B.ROUND_STOCHASTIC, SEED, counter)
    aa = b16.tables([(idx[t], wa[t], g[t], R, D) for t in range(T)])
    ab = b16.tables([(idx[t], wb[t], g[t], R, D) for t in range(T)])
    b16.base.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, aa, T, L, D, batch, capi.AGGR_MODE_SUM, 0.05, rnd, None), "sgd16")
    st = hip.emb_states([(None, None)] * T)
    b16.base.check(b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, ab, st, T, L, D, batch, capi.AGGR_MODE_SUM,
                                                                  _opt(capi.SPARSE_OPT_SGD, lr=0.05), rnd, None), "opt16 sgd")
    torch.cuda.synchronize()
    assert hip.lib.ffh_embedding_last_route(hip.ctx).decode().startswith(route)
    for t in range(T):
        assert torch.equal(wa[t], wb[t])
    del ws
