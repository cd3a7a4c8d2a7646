"""The learning-rate extension (include/ff_hip_lr.h) on the GPU.

Kernel level, through the C-ABI: the state block advanced 2000 times equals the host formula bit for bit (the SGD rate and Adam's alpha_t);
the dense and the table `_lr` entries leave the bits of the scalar entries called with the block's value, on every form of the kernels.
Model level (tiny golden DLRM, --deterministic, (W,S,N) = (2,3,3), 8 steps): device route == host route, hipGraph replay == eager, Adam
captured with --device-lr == Adam on the eager path of before, overlap == --no-overlap, eval_batch() advances nothing."""
import math

import numpy as np
import pytest

import bf16_helpers as B
import lr_helpers as LH
from dlrm_flexflow_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lr(hip):
    return capi.lr_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


def _block(lr, base, W=0, S=0, N=0, beta1=0.0, beta2=0.0, first_step=0):
    import torch
    blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device=DEV)
    lr.init(blk, base, W, S, N, beta1, beta2, first_step)
    return blk


# ---------------------------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------------------------
def test_block_advanced_2000_times_equals_the_host_formula(hip, lr):
    """(W,S,N) = (50,100,300), Adam's default betas (the doubles of 0.9f / 0.999f, as AdamOptimizer holds them): at every step the SGD rate is
    the host formula's float and alpha_t the float of the host's double AdamOptimizer::next, bit for bit."""
    W, S, N, steps = 50, 100, 300, 2000
    base = float(np.float32(0.001))
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    blk = _block(lr, base, W, S, N, b1, b2)
    got = []
    for _ in range(steps):
        v = lr.read(blk)
        got.append((v.k, np.float32(v.lr), np.float32(v.alpha_t), v.beta1_t, v.beta2_t))
        lr.call("ffh_lr_state_advance", blk, None)
    b1t = b2t = 1.0
    bad = []
    for k in range(steps):
        rate = LH.schedule_f64(k, base, W, S, N)
        b1t *= b1
        b2t *= b2
        alpha_t = rate * math.sqrt(1 - b2t) / (1 - b1t)          # AdamOptimizer::next with alpha = the scheduled rate
        want = (k, np.float32(rate), np.float32(alpha_t), b1t, b2t)
        g = got[k]
        if not (g[0] == want[0] and g[1].tobytes() == want[1].tobytes() and g[2].tobytes() == want[2].tobytes() and g[3] == want[3] and g[4] == want[4]):
            bad.append((k, g, want))
    assert not bad, f"{len(bad)} of {steps} steps differ; first: {bad[0]}"


def test_block_initialised_at_a_later_step_equals_that_many_advances(hip, lr):
    a = _block(lr, 0.01, 2, 3, 3, 0.9, 0.999)
    for _ in range(7):
        lr.call("ffh_lr_state_advance", a, None)
    b = _block(lr, 0.01, 2, 3, 3, 0.9, 0.999, first_step=7)
    va, vb = lr.read(a), lr.read(b)
    assert (va.k, va.lr, va.alpha_t, va.beta1_t, va.beta2_t) == (vb.k, vb.lr, vb.alpha_t, vb.beta1_t, vb.beta2_t) and va.k == 7


def test_block_refuses_a_decay_inside_the_warmup(hip, lr):
    import torch
    blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device=DEV)
    sc = capi.LrSchedule(0.01, 5, 3, 2, 0.0, 0.0)
    assert lr.lib.ffh_lr_state_init(lr.ctx, capi.ptr(blk), sc, 0, None) != 0


# ---------------------------------------------------------------------------------------------------------------------
# dense entries
# ---------------------------------------------------------------------------------------------------------------------
_DENSE = {"sgd": dict(wd=0.0, mom=0.0, nesterov=0), "momentum_nesterov_wd": dict(wd=1e-3, mom=0.9, nesterov=1), "adam": None}


@pytest.mark.parametrize("zero_grad", [0, 1], ids=["keep_grad", "zero_grad"])
@pytest.mark.parametrize("rule", list(_DENSE))
@pytest.mark.parametrize("n", [4096, 4099], ids=["n4096_vec4", "n4099_scalar"])
def test_dense_lr_entries_equal_the_scalar_entries(hip, lr, n, rule, zero_grad):
    import torch
    rng = np.random.default_rng(n + zero_grad)
    blk = _block(lr, 0.0123, 4, 0, 0, 0.9, 0.999, first_step=1)      # mid warm-up: neither rate is the base
    v = lr.read(blk)
    mk = lambda scale=1.0: torch.from_numpy((rng.standard_normal(n) * scale).astype(np.float32)).to(DEV)
    w0, g0, s0, s1 = mk(), mk(), mk(0.1), mk(0.01).abs()
    outs = []
    for via_block in (False, True):
        w, g, a, b = w0.clone(), g0.clone(), s0.clone(), s1.clone()
        if rule == "adam":
            if via_block:
                lr.call("ffh_adam_update_lr", w, g, a, b, n, blk, 0.9, 0.999, 1e-4, 1e-8, zero_grad, None)
            else:
                hip.call("ffh_adam_update", w, g, a, b, n, float(v.alpha_t), 0.9, 0.999, 1e-4, 1e-8, zero_grad, None)
        else:
            r = _DENSE[rule]
            if via_block:
                lr.call("ffh_sgd_update_ex_lr", w, g, a, n, blk, r["wd"], r["mom"], r["nesterov"], zero_grad, None)
            else:
                hip.call("ffh_sgd_update_ex", w, g, a, n, float(v.lr), r["wd"], r["mom"], r["nesterov"], zero_grad, None)
        torch.cuda.synchronize()
        outs.append([t.view(torch.int32).cpu() for t in (w, g, a, b)])
    for name, x, y in zip(("weights", "gradients", "state 0", "state 1"), *outs):
        assert torch.equal(x, y), name
    assert not torch.equal(outs[0][0], w0.view(torch.int32).cpu())
    assert bool((outs[1][1] == 0).all()) == bool(zero_grad)


# ---------------------------------------------------------------------------------------------------------------------
# table entries: fp32 and bf16 (nearest), SGD / momentum / Adam, on the small, lsd and bucket forms
# ---------------------------------------------------------------------------------------------------------------------
def _opt(kind, lr_value, **kw):
    o = capi.SparseOpt()
    o.kind = kind
    o.lr = lr_value
    o.weight_decay = kw.get("wd", 0.0)
    o.momentum = kw.get("mom", 0.0)
    o.nesterov = 1 if kw.get("nesterov") else 0
    o.beta1, o.beta2, o.epsilon = 0.9, 0.999, 1e-8
    return o


_RULES = {
    "sgd": lambda r: _opt(capi.SPARSE_OPT_SGD, r),
    "momentum": lambda r: _opt(capi.SPARSE_OPT_SGD_MOMENTUM, r, mom=0.9, nesterov=True, wd=1e-3),
    "adam": lambda r: _opt(capi.SPARSE_OPT_ADAM, r, wd=1e-4),
}
# (T, R, D, batch, L, route prefix): three tables, D = 16 and D = 128, the smallest shapes of the sweep in tests/test_gpu_round5.py / the bf16
# optimizer tests that reach each form
_FORMS = [(3, 1000, 16, 512, 1, "small"), (3, 200_000, 128, 40_000, 3, "lsd:"), (3, 100_000, 16, 16_384, 1, "buckets:"), (3, 100_000, 128, 16_384, 1, "buckets:"),
          (3, 2000, 6, 700, 2, "small")]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rule", list(_RULES))
@pytest.mark.parametrize("shape", _FORMS, ids=[f[-1].rstrip(":") + f"_D{f[2]}" for f in _FORMS])
def test_table_lr_entries_equal_the_scalar_entries(hip, lr, b16, shape, rule, dtype):
    _table_case(hip, lr, b16, shape, rule, dtype, True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rule", ["momentum", "adam"])
@pytest.mark.parametrize("shape", [_FORMS[0], _FORMS[2]], ids=["small", "buckets"])
def test_table_lr_apply_entries_behind_a_sort(hip, lr, b16, shape, rule, dtype):
    _table_case(hip, lr, b16, shape, rule, dtype, False)


def _table_case(hip, lr, b16, shape, rule, dtype, fused):
    import torch
    T, R, D, batch, L, route = shape
    rng = np.random.default_rng(T * 7 + R + D + batch)
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(T, L, D, batch) + 256
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(ws, n)
    blk = _block(lr, 0.05, 4, 0, 0, 0.9, 0.999, first_step=2)
    v = lr.read(blk)
    rate = float(v.alpha_t if rule == "adam" else v.lr)
    assert rate != 0.05
    opt_scalar, opt_block = _RULES[rule](rate), _RULES[rule](123.0)     # the block form ignores opt.lr
    idx = [torch.from_numpy(rng.integers(0, R, (batch, L))).to(DEV) for _ in range(T)]
    g = [torch.from_numpy(rng.standard_normal((batch, D)).astype(np.float32)).to(DEV) for _ in range(T)]
    if dtype == "bf16":
        w0 = [torch.from_numpy(B.rne(rng.standard_normal((R, D)).astype(np.float32) * 0.1).view(np.int16)).to(DEV) for _ in range(T)]
    else:
        w0 = [torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32) * 0.1).to(DEV) for _ in range(T)]
    nstate = {"sgd": 0, "momentum": 1, "adam": 2}[rule]
    st0 = [[torch.from_numpy(np.abs(rng.standard_normal((R, D))).astype(np.float32) * 0.01).to(DEV) for _ in range(nstate)] for _ in range(T)]
    rnd = b16.rounding(B.ROUND_NEAREST)
    res = []
    for via_block in (False, True):
        w = [x.clone() for x in w0]
        S = [[s.clone() for s in st] for st in st0]
        states = hip.emb_states([(S[t][0] if nstate > 0 else None, S[t][1] if nstate > 1 else None) for t in range(T)])
        opt = opt_block if via_block else opt_scalar
        if dtype == "bf16":
            tabs = b16.tables([(idx[t], w[t], g[t], R, D, 10 + t, 0) for t in range(T)])
            if not fused:
                hip.check(b16.lib.ffh_embedding_bwd_sort_multi_bf16(hip.ctx, tabs, T, L, D, batch, None), "sort16")
            if via_block:
                fn = lr.lib.ffh_embedding_bwd_opt_fused_multi_bf16_lr if fused else lr.lib.ffh_embedding_bwd_opt_apply_multi_bf16_lr
                hip.check(fn(hip.ctx, tabs, states, T, L, D, batch, capi.AGGR_MODE_SUM, opt, rnd, capi.ptr(blk), None), "bf16 _lr")
            else:
                fn = b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16 if fused else b16.lib.ffh_embedding_bwd_opt_apply_multi_bf16
                hip.check(fn(hip.ctx, tabs, states, T, L, D, batch, capi.AGGR_MODE_SUM, opt, rnd, None), "bf16 scalar")
        else:
            tabs = hip.emb_tables([(idx[t], w[t], g[t], R, D) for t in range(T)])
            if not fused:
                hip.check(hip.lib.ffh_embedding_bwd_sort_multi(hip.ctx, tabs, T, L, D, batch, None), "sort")
            if via_block:
                fn = lr.lib.ffh_embedding_bwd_opt_fused_multi_lr if fused else lr.lib.ffh_embedding_bwd_opt_apply_multi_lr
                hip.check(fn(hip.ctx, tabs, states, T, L, D, batch, capi.AGGR_MODE_SUM, opt, capi.ptr(blk), None), "fp32 _lr")
            else:
                fn = hip.lib.ffh_embedding_bwd_opt_fused_multi if fused else hip.lib.ffh_embedding_bwd_opt_apply_multi
                hip.check(fn(hip.ctx, tabs, states, T, L, D, batch, capi.AGGR_MODE_SUM, opt, None), "fp32 scalar")
        torch.cuda.synchronize()
        got = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
        assert got.startswith(route), got
        res.append((w, S))
    for t in range(T):
        assert torch.equal(res[0][0][t], res[1][0][t]), f"table {t}"
        assert not torch.equal(res[0][0][t], w0[t]), f"table {t} was not updated"
        for k in range(nstate):
            assert torch.equal(res[0][1][t][k].view(torch.int32), res[1][1][t][k].view(torch.int32)), f"state {k} of table {t}"
    if rule == "sgd":      # kind SGD through a block = the plain fused update with that rate
        w = [x.clone() for x in w0]
        if dtype == "bf16":
            tabs = b16.tables([(idx[t], w[t], g[t], R, D, 10 + t, 0) for t in range(T)])
            hip.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(hip.ctx, tabs, T, L, D, batch, capi.AGGR_MODE_SUM, rate, rnd, None), "sgd16")
        else:
            tabs = hip.emb_tables([(idx[t], w[t], g[t], R, D) for t in range(T)])
            hip.check(hip.lib.ffh_embedding_bwd_sgd_fused_multi(hip.ctx, tabs, T, L, D, batch, capi.AGGR_MODE_SUM, rate, None), "sgd32")
        torch.cuda.synchronize()
        for t in range(T):
            assert torch.equal(w[t], res[1][0][t]), f"table {t}: plain fused update"
    del ws


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
SCHED = (2, 3, 3)
STEPS = 8


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("variant", ["sgd_fp32", "sgd_bf16_nearest", "sgd_sparse_opt", "momentum_sparse_opt"])
def test_device_route_equals_host_route(hip, variant):
    flags, opt = LH.VARIANTS[variant]
    host = LH.run_model(None, STEPS, SCHED, device_lr=False, flags=flags, optimizer=opt)
    dev = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags, optimizer=opt)
    assert host["route"] == 1 and dev["route"] == 2
    assert dev["lr_steps"] == STEPS and host["lr_steps"] == STEPS
    assert dev["lrs"] == host["lrs"] == [LH.schedule_f32(k, opt[1], *SCHED) for k in range(STEPS)]
    _same(host["state"], dev["state"])
    for a, b in zip(host["preds"], dev["preds"]):
        assert np.array_equal(a, b)


def test_replayed_graph_follows_the_schedule(hip):
    flags, opt = LH.VARIANTS["sgd_fp32"]
    eager = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags, optimizer=opt)
    traced = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags, optimizer=opt, trace=True)
    assert traced["replays"] >= STEPS - 2 and eager["replays"] == 0
    assert traced["lrs"] == [LH.schedule_f32(k, opt[1], *SCHED) for k in range(STEPS)]
    assert traced["lr_steps"] == STEPS
    _same(eager["state"], traced["state"])
    for a, b in zip(eager["preds"], traced["preds"]):
        assert np.array_equal(a, b)


def test_adam_captured_with_device_lr_equals_adam_on_the_eager_path(hip):
    flags = ["--sparse-embedding-optimizer"]
    parent = LH.run_model(None, 6, (0, 0, 0), device_lr=None, flags=flags, optimizer=("adam", 0.001), trace=True)      # as before: never captures
    traced = LH.run_model(None, 6, (0, 0, 0), device_lr=True, flags=flags, optimizer=("adam", 0.001), trace=True)
    assert parent["route"] == 0 and parent["replays"] == 0 and not parent["uses_graph"]
    assert traced["route"] == 2 and traced["replays"] >= 4
    _same(parent["state"], traced["state"])
    for a, b in zip(parent["preds"], traced["preds"]):
        assert np.array_equal(a, b)


def test_overlap_equals_no_overlap_on_the_device_route(hip):
    flags, opt = LH.VARIANTS["momentum_sparse_opt"]
    a = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags, optimizer=opt)
    b = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags + ["--no-overlap"], optimizer=opt)
    assert a["route"] == b["route"] == 2
    _same(a["state"], b["state"])


def test_eval_batch_advances_nothing(hip):
    flags, opt = LH.VARIANTS["sgd_fp32"]
    plain = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags, optimizer=opt)
    with_eval = LH.run_model(None, STEPS, SCHED, device_lr=True, flags=flags, optimizer=opt, eval_between=True)
    assert with_eval["lr_steps"] == STEPS and with_eval["lrs"] == plain["lrs"]
    _same(plain["state"], with_eval["state"])
