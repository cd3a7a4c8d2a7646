"""The launch table of the fused table update (csrc/emb_reduce.h), entry by entry: every (row rule x weight type x VEC x route x entry) is one
case, 120 in all, one per update kernel.  A wrong entry -- the bf16 form of a rule naming the fp32 kernel, say -- compiles and launches; here it
ends in other bits than the reference, or in another route.

Each case runs one step of two tables through the scalar entry and the `_lr` entry (the scalar one with the rate the block reports) from the same
start and asserts: the route the call reported; that both entries leave the same bits in weights and state; that the case's entry leaves the
reference's bits in the rows hit; that rows nobody hit keep weights and state.  The reference is the CPU oracle's update for SGD, momentum and
Adam, and for the two Adagrad rules the numpy restatements on the oracle's canonical sums, as tests/test_gpu_adagrad.py and
tests/test_gpu_rowwise.py take them; on bf16 tables the same on the widened table, rounded to nearest once.

Shapes (read off emb_bwd_phases, embedding.hip): `small`: batch * bag = 512 <= 2048.  `lsd:`: 2304 > 2048 lookups and ids of 9 bits (300 rows),
so one pass and no bucket form.  `buckets:`: 4096 <= 65536 lookups and ids of 13 bits (5000 rows) > 9; the 3-row table's rows fold across tiles.
D = 8 is the 16-byte form (VEC 4), D = 6 the scalar one (VEC 1)."""
import ctypes as C

import numpy as np
import pytest

import bf16_helpers as B
import test_gpu_adagrad as AG
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xD15C
EPS = 1e-10
IT = 5      # the bf16 update counter (unused by round-to-nearest)

_KINDS = {"sgd": capi.SPARSE_OPT_SGD, "momentum": capi.SPARSE_OPT_SGD_MOMENTUM, "adam": capi.SPARSE_OPT_ADAM,
          "adagrad": capi.SPARSE_OPT_ADAGRAD, "rowwise": capi.SPARSE_OPT_ROWWISE_ADAGRAD}
# route token -> (batch, rows per table); bag 1
_ROUTES = {"small": (512, (1000, 40)), "lsd:": (2304, (300, 40)), "buckets:": (4096, (5000, 3))}
_DIMS = {4: 8, 1: 6}      # VEC -> D
_CASES = [(rule, wt, vec, route, entry) for rule in _KINDS for wt in ("fp32", "bf16") for vec in _DIMS for route in _ROUTES for entry in ("scalar", "lr")]
assert len(_CASES) == 120


@pytest.fixture(scope="module")
def lr(hip):
    return capi.lr_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


def _opt(rule, rate):
    o = capi.SparseOpt()
    o.kind = _KINDS[rule]
    o.lr = rate
    o.beta1, o.beta2 = 0.9, 0.999
    o.epsilon = 1e-8 if rule == "adam" else EPS
    if rule == "momentum":
        o.weight_decay, o.momentum, o.nesterov = 1e-3, 0.9, 1
    elif rule == "adam":
        o.weight_decay = 1e-4
    return o


def _start(rule, wt, D, route):
    """ids, gradients, weights (fp32, and their bf16 bits on bf16 tables) and state of the two tables, as numpy arrays"""
    batch, rows = _ROUTES[route]
    rng = np.random.default_rng([SEED, batch, D, list(_KINDS).index(rule)])
    tables = []
    for R in rows:
        ids = rng.integers(0, R, (batch, 1))
        ids[ids % 5 == 2] = (ids[ids % 5 == 2] + 1) % R      # rows = 2 (mod 5) are hit by nobody
        w = (rng.standard_normal((R, D)) * 0.1).astype(np.float32)
        bits = B.rne(w) if wt == "bf16" else None
        if bits is not None:
            w = B.widen(bits)
        s0 = s1 = None
        if rule == "momentum":
            s0 = (np.abs(rng.standard_normal((R, D))) * 0.01).astype(np.float32)
        elif rule == "adam":
            s0 = (rng.standard_normal((R, D)) * 0.01).astype(np.float32)
            s1 = (np.abs(rng.standard_normal((R, D))) * 0.01).astype(np.float32)
        elif rule == "adagrad":
            s0 = np.full((R, D), 0.1, np.float32)
        elif rule == "rowwise":
            s0 = np.full((R,), 0.1, np.float32)
        hit = np.zeros(R, bool)
        hit[ids.ravel()] = True
        assert hit.any() and not hit.all()
        tables.append(dict(R=R, idx=ids, g=rng.standard_normal((batch, D)).astype(np.float32), w=w, bits=bits, s0=s0, s1=s1, hit=hit))
    return tables


def _reference(oracle, rule, wt, rate, tb):
    """(weights, s0, s1) of the rows hit after the step: fp32 weights, or their bf16 bits"""
    hit = tb["hit"]
    if rule in ("sgd", "momentum", "adam"):
        w, s0, s1 = oracle.embedding_bwd_opt(tb["idx"], tb["g"], tb["w"], _opt(rule, rate), tb["s0"], tb["s1"])
        w, s0, s1 = w[hit], None if s0 is None else s0[hit], None if s1 is None else s1[hit]
    else:
        uniq, sums = AG._canonical_sums(oracle, tb["idx"], tb["g"], capi.AGGR_MODE_SUM)
        assert np.array_equal(uniq, np.flatnonzero(hit))
        step = ffmodel.adagrad_reference if rule == "adagrad" else ffmodel.rowwise_adagrad_reference
        w, s0 = step(tb["w"][hit], sums, tb["s0"][hit], rate, EPS, 0.0)
        s1 = None
    return (B.rne(w) if wt == "bf16" else w), s0, s1


_RESULTS = {}


def _run(hip, lr, b16, oracle, rule, wt, vec, route):
    """Both entries on the GPU and the reference, once per (rule, weight type, VEC, route)"""
    key = (rule, wt, vec, route)
    if key in _RESULTS:
        return _RESULTS[key]
    import torch
    D = _DIMS[vec]
    batch, rows = _ROUTES[route]
    T, L = len(rows), 1
    tables = _start(rule, wt, D, route)
    ws = AG._ws(hip, T, L, D, batch)
    blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device=DEV)
    lr.init(blk, 0.05, 3, 3, 4, 0.9, 0.999, 1)      # mid warm-up: neither rate is the base
    v = lr.read(blk)
    rate = float(np.float32(v.alpha_t if rule == "adam" else v.lr))
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)
    idx, g = [dev(tb["idx"]) for tb in tables], [dev(tb["g"]) for tb in tables]
    got = {}
    for entry in ("scalar", "lr"):
        w = [dev(tb["bits"] if wt == "bf16" else tb["w"]) for tb in tables]
        s0, s1 = [dev(tb["s0"]) for tb in tables], [dev(tb["s1"]) for tb in tables]
        st = hip.emb_states(list(zip(s0, s1)))
        opt = _opt(rule, rate if entry == "scalar" else 123.0)      # (the _lr entries ignore opt.lr)
        if wt == "fp32":
            tabs = hip.emb_tables([(idx[t], w[t], g[t], rows[t], D) for t in range(T)])
            args = (tabs, st, T, L, D, batch, capi.AGGR_MODE_SUM, C.byref(opt))
            name = "ffh_embedding_bwd_opt_fused_multi"
            if entry == "lr":
                lr.call(name + "_lr", *args, blk, None)
            else:
                hip.check(getattr(hip.lib, name)(hip.ctx, *args, None), name)
        else:
            tabs = b16.tables([(idx[t], w[t], g[t], rows[t], D, 10 + t, 0) for t in range(T)])
            rnd = b16.rounding(B.ROUND_NEAREST, SEED, torch.tensor([IT], dtype=torch.int64, device=DEV))
            args = (tabs, st, T, L, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), C.byref(rnd))
            name = "ffh_embedding_bwd_opt_fused_multi_bf16"
            if entry == "lr":
                lr.call(name + "_lr", *args, blk, None)
            else:
                b16.base.check(getattr(b16.lib, name)(b16.ctx, *args, None), name)
        torch.cuda.synchronize()
        host = lambda ts: [None if x is None else x.cpu().numpy() for x in ts]
        got[entry] = dict(route=hip.lib.ffh_embedding_last_route(hip.ctx).decode(),
                          w=[x.view(np.uint16) if wt == "bf16" else x for x in host(w)], s0=host(s0), s1=host(s1))
    del ws
    ref = [_reference(oracle, rule, wt, rate, tb) for tb in tables]
    _RESULTS[key] = (tables, ref, got)
    return _RESULTS[key]


def _same(a, b):
    return (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("rule,wt,vec,route,entry", _CASES, ids=["-".join(map(str, c)).replace(":", "") for c in _CASES])
def test_every_entry_of_the_launch_table(hip, lr, b16, oracle, rule, wt, vec, route, entry):
    tables, ref, got = _run(hip, lr, b16, oracle, rule, wt, vec, route)
    mine, other = got[entry], got["lr" if entry == "scalar" else "scalar"]
    assert mine["route"].startswith(route), (mine["route"], route)
    for t, tb in enumerate(tables):
        hit = tb["hit"]
        start = dict(w=tb["bits"] if wt == "bf16" else tb["w"], s0=tb["s0"], s1=tb["s1"])
        for k, what in enumerate(("w", "s0", "s1")):
            a, b, r, s = mine[what][t], other[what][t], ref[t][k], start[what]
            assert _same(a, b), f"table {t}: {what}: the scalar and the _lr entry differ"
            if a is None:
                assert r is None and s is None
                continue
            assert a[hit].tobytes() == r.tobytes(), f"table {t}: {what}: {np.count_nonzero(a[hit] != r)} of {r.size} elements of the rows hit differ from the reference"
            assert a[~hit].tobytes() == s[~hit].tobytes(), f"table {t}: {what}: rows nobody hit have moved"
        assert not _same(mine["w"][t][hit], start["w"][hit])      # (the update ran)
