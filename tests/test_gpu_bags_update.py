"""The fused table update with a bag size per table (include/ff_hip_bags_update.h), through the C-ABI.

The reference is always the uniform fused entry, called once per table (in_dim = the table's own bag size) from the same start; weights, every
state array and bf16 bit patterns are compared with assert_array_equal -- the ragged call promises the uniform call's bits, table by table.

Shapes (read off emb_bwd_bags, embedding.hip, and emb_bags_update.h):
  small form    batch 64, bags [1, 7, 3] and [32, 1]: every N_t <= 2048, one table at exactly 2048 and one at 64.
  sorted form   batch 500, bags [1, 100, 1, 7] in three orders: N_t = 500 / 50,000 / 500 / 3,500, so the offsets of a table depend on what lies
                before it, tables below 2048 entries ride in a sorted call, no N_t is a multiple of the tile (128 .. 1024), and 500 / 3,500 are no
                multiples of FFH_EMB_CHUNK (32) or FFH_EMB_CHUNK1 (1024).  Rows 3 / 300 / 5,000 / 70,000: one or two sort passes per table.  The
                3-row table takes the bag of 100: its three runs cross every tile and 1024-block (nchunks1 = 49 against 1 and 4 beside it).
  a long list   batch 6,000, bags [100, 1], rows [5, 40,000]: 600,000 entries (1,172 level-1 slots, beyond the fold's stage of 1,024).
Rows = 2 (mod 5) are hit by nobody (as tests/test_gpu_emb_dispatch.py builds its ids) and must keep weights and state."""
import ctypes as C

import numpy as np
import pytest

import bf16_helpers as B
from dlrm_flexflow_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xBA65
EPS = 1e-10
IT = 5      # the bf16 update counter

_KINDS = {"sgd": capi.SPARSE_OPT_SGD, "momentum": capi.SPARSE_OPT_SGD_MOMENTUM, "adam": capi.SPARSE_OPT_ADAM,
          "adagrad": capi.SPARSE_OPT_ADAGRAD, "rowwise": capi.SPARSE_OPT_ROWWISE_ADAGRAD}
_DIMS = {4: 8, 1: 6}      # VEC -> D
# form -> (batch, bags, rows)
_FORMS = {"small": (64, (1, 7, 3), (300, 3, 5000)), "lsd": (500, (1, 100, 1, 7), (300, 3, 5000, 70000))}
_SWEEP = [(rule, wt, vec, form, entry) for rule in _KINDS for wt in ("fp32", "bf16") for vec in _DIMS for form in _FORMS for entry in ("scalar", "lr")]
assert len(_SWEEP) == 80


@pytest.fixture(scope="module")
def lr(hip):
    return capi.lr_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


@pytest.fixture(scope="module")
def bu(hip):
    return capi.bags_update_api(hip)


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


def _start(rule, wt, D, batch, bags, rows, tag=0):
    rng = np.random.default_rng([SEED, batch, D, list(_KINDS).index(rule), tag] + list(bags))
    tables = []
    for L, R in zip(bags, rows):
        ids = rng.integers(0, R, (batch, L))
        ids[ids % 5 == 2] = (ids[ids % 5 == 2] + 1) % R      # rows = 2 (mod 5) are hit by nobody
        w = (rng.standard_normal((R, D)) * 0.1).astype(np.float32)
        bits = B.rne(w) if wt == "bf16" else None
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
        tables.append(dict(R=R, L=L, idx=ids, g=rng.standard_normal((batch, D)).astype(np.float32), w=bits if wt == "bf16" else w, s0=s0, s1=s1, hit=hit))
    return tables


class _Runner:
    """One start on the device; `ragged()` and `uniform(groups)` each run one step from it and return the tables' (w, s0, s1) as numpy."""

    def __init__(self, hip, lr, b16, bu, tables, rule, wt, D, batch, aggr=capi.AGGR_MODE_SUM, entry="scalar", mode=B.ROUND_NEAREST, plain=False):
        import torch
        self.torch = torch
        self.hip, self.lr, self.b16, self.bu = hip, lr, b16, bu
        self.tables, self.rule, self.wt, self.D, self.batch, self.aggr, self.entry, self.mode, self.plain = tables, rule, wt, D, batch, aggr, entry, mode, plain
        self.bags = [tb["L"] for tb in tables]
        dev = self._dev
        self.idx, self.g = [dev(tb["idx"]) for tb in tables], [dev(tb["g"]) for tb in tables]
        self.blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device=DEV)
        lr.init(self.blk, 0.05, 3, 3, 4, 0.9, 0.999, 1)      # mid warm-up: neither rate is the base
        v = lr.read(self.blk)
        self.rate = float(np.float32(v.alpha_t if rule == "adam" else v.lr))
        need = max([bu.workspace_bytes(self.bags, D, batch)] + [int(hip.lib.ffh_embedding_bwd_workspace_bytes(len(self.bags), L, D, batch)) for L in self.bags])
        self.ws_bytes = need + 256
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)
        hip.set_workspace(self.ws, self.ws_bytes)
        self.route = None

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)

    def _fresh(self):
        w = [self._dev(tb["w"]) for tb in self.tables]
        s0, s1 = [self._dev(tb["s0"]) for tb in self.tables], [self._dev(tb["s1"]) for tb in self.tables]
        return w, s0, s1

    def _rounding(self):
        return self.b16.rounding(self.mode, SEED, self.torch.tensor([IT], dtype=self.torch.int64, device=DEV))

    def _tabs(self, w, sel):
        if self.wt == "fp32":
            return self.hip.emb_tables([(self.idx[t], w[t], self.g[t], self.tables[t]["R"], self.D) for t in sel])
        return self.b16.tables([(self.idx[t], w[t], self.g[t], self.tables[t]["R"], self.D, 10 + t, 0) for t in sel])

    def _host(self, w, s0, s1):
        self.torch.cuda.synchronize()
        host = lambda ts: [None if x is None else x.cpu().numpy() for x in ts]
        return dict(w=[x.view(np.uint16) if self.wt == "bf16" else x for x in host(w)], s0=host(s0), s1=host(s1))

    def descriptor(self, w, s0, s1, **over):
        sel = range(len(self.tables))
        kw = dict(in_dims=self.bags, out_dim=self.D, batch=self.batch, aggr=self.aggr, states=self.hip.emb_states(list(zip(s0, s1))))
        kw["tables" if self.wt == "fp32" else "tables_bf16"] = self._tabs(w, sel)
        if self.wt == "bf16":
            kw["rounding"] = self._rounding()
        if self.plain:
            kw["lr"] = self.rate
            kw["states"] = None
        else:
            kw["opt"] = _opt(self.rule, self.rate if self.entry == "scalar" else 123.0)      # (with an lr_block opt.lr is ignored)
            if self.entry == "lr":
                kw["lr_block"] = self.blk
        kw.update(over)
        return capi.BagsUpdateApi.descriptor(**kw)

    def ragged(self):
        w, s0, s1 = self._fresh()
        self.bu.call(self.descriptor(w, s0, s1))
        out = self._host(w, s0, s1)
        self.route = self.hip.lib.ffh_embedding_last_route(self.hip.ctx).decode()
        return out

    def uniform(self, groups=None):
        """the uniform fused entry, once per group of tables of one bag size (default: once per table)"""
        w, s0, s1 = self._fresh()
        hip, b16, lr = self.hip, self.b16, self.lr
        for sel in (groups or [[t] for t in range(len(self.tables))]):
            L = self.tables[sel[0]]["L"]
            assert all(self.tables[t]["L"] == L for t in sel)
            tabs, T = self._tabs(w, sel), len(sel)
            st = hip.emb_states([(s0[t], s1[t]) for t in sel])
            opt = _opt(self.rule, self.rate if self.entry == "scalar" else 123.0)
            if self.wt == "fp32":
                if self.plain:
                    hip.check(hip.lib.ffh_embedding_bwd_sgd_fused_multi(hip.ctx, tabs, T, L, self.D, self.batch, self.aggr, self.rate, None), "sgd_fused_multi")
                elif self.entry == "lr":
                    lr.call("ffh_embedding_bwd_opt_fused_multi_lr", tabs, st, T, L, self.D, self.batch, self.aggr, C.byref(opt), self.blk, None)
                else:
                    hip.check(hip.lib.ffh_embedding_bwd_opt_fused_multi(hip.ctx, tabs, st, T, L, self.D, self.batch, self.aggr, C.byref(opt), None), "opt_fused_multi")
            else:
                rnd = self._rounding()
                if self.plain:
                    hip.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, tabs, T, L, self.D, self.batch, self.aggr, self.rate, C.byref(rnd), None), "sgd_fused_multi_bf16")
                elif self.entry == "lr":
                    lr.call("ffh_embedding_bwd_opt_fused_multi_bf16_lr", tabs, st, T, L, self.D, self.batch, self.aggr, C.byref(opt), C.byref(rnd), self.blk, None)
                else:
                    hip.check(b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, tabs, st, T, L, self.D, self.batch, self.aggr, C.byref(opt), C.byref(rnd), None),
                              "opt_fused_multi_bf16")
        return self._host(w, s0, s1)


def _assert_same(tables, got, ref, moved=True):
    for t, tb in enumerate(tables):
        hit = tb["hit"]
        for what in ("w", "s0", "s1"):
            a, r, s = got[what][t], ref[what][t], tb[what]
            if a is None:
                assert r is None and s is None
                continue
            np.testing.assert_array_equal(a, r, err_msg=f"table {t} (bag {tb['L']}, {tb['R']} rows): {what} differs from the uniform call's")
            np.testing.assert_array_equal(a[~hit], s[~hit], err_msg=f"table {t}: {what}: rows nobody hit have moved")
        if moved:
            assert not np.array_equal(got["w"][t][hit], tb["w"][hit]), f"table {t}: the update did not run"


def _compare(hip, lr, b16, bu, batch, bags, rows, rule="sgd", wt="fp32", D=8, tag=0, route=None, groups=None, **kw):
    tables = _start(rule, wt, D, batch, bags, rows, tag)
    run = _Runner(hip, lr, b16, bu, tables, rule, wt, D, batch, **kw)
    got = run.ragged()
    if route is not None:
        assert run.route == route, run.route
    _assert_same(tables, got, run.uniform(groups))
    return run, tables, got


# ---- the forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bags,rows", [((1, 7, 3), (300, 3, 5000)), ((32, 1), (40, 1000))], ids=["1-7-3", "32-1"])
def test_small_form(hip, lr, b16, bu, bags, rows):
    _compare(hip, lr, b16, bu, 64, bags, rows, route="bags:small")


@pytest.mark.parametrize("bags,rows", [((1, 100, 1, 7), (300, 3, 5000, 70000)), ((100, 1, 1, 7), (3, 300, 5000, 70000)), ((7, 1, 1, 100), (70000, 5000, 300, 3))],
                         ids=["heavy-middle", "heavy-first", "heavy-last"])
def test_sorted_form_offsets_and_partial_tiles(hip, lr, b16, bu, bags, rows):
    _compare(hip, lr, b16, bu, 500, bags, rows, route="bags:lsd:passes=2")


def test_a_long_list_beside_a_short_one(hip, lr, b16, bu):
    _compare(hip, lr, b16, bu, 6000, (100, 1), (5, 40000), route="bags:lsd:passes=2")


def test_three_sort_passes_beside_tables_of_two_and_one(hip, lr, b16, bu):
    """300,000 rows are 19 bits: three 7-bit digits for the call; the 300-row table sorts in two of them and the 3-row table in one, so the
    tables end in different key buffers."""
    _compare(hip, lr, b16, bu, 500, (7, 100, 1), (300, 300000, 3), rule="adagrad", route="bags:lsd:passes=3")


@pytest.mark.parametrize("rule,wt,vec,form,entry", _SWEEP, ids=["-".join(map(str, c)) for c in _SWEEP])
def test_every_rule_weight_type_width_and_entry(hip, lr, b16, bu, rule, wt, vec, form, entry):
    batch, bags, rows = _FORMS[form]
    _compare(hip, lr, b16, bu, batch, bags, rows, rule=rule, wt=wt, D=_DIMS[vec], entry=entry, route="bags:small" if form == "small" else "bags:lsd:passes=2")


@pytest.mark.parametrize("wt", ["fp32", "bf16"])
@pytest.mark.parametrize("form", list(_FORMS))
def test_plain_sgd_without_a_rule(hip, lr, b16, bu, form, wt):
    batch, bags, rows = _FORMS[form]
    _compare(hip, lr, b16, bu, batch, bags, rows, wt=wt, plain=True)


@pytest.mark.parametrize("rule", ["sgd", "rowwise", "adam"])
@pytest.mark.parametrize("form", list(_FORMS))
def test_stochastic_rounding_with_the_same_counter(hip, lr, b16, bu, form, rule):
    batch, bags, rows = _FORMS[form]
    _compare(hip, lr, b16, bu, batch, bags, rows, rule=rule, wt="bf16", mode=B.ROUND_STOCHASTIC)


@pytest.mark.parametrize("aggr", [capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG], ids=["sum", "avg"])
@pytest.mark.parametrize("form", list(_FORMS))
def test_sum_and_avg(hip, lr, b16, bu, form, aggr):
    batch, bags, rows = _FORMS[form]
    _compare(hip, lr, b16, bu, batch, bags, rows, rule="adagrad", aggr=aggr, tag=1)


@pytest.mark.parametrize("batch,L", [(64, 3), (500, 7)], ids=["small", "lsd"])
def test_equal_bag_sizes_give_the_uniform_multi_table_call(hip, lr, b16, bu, batch, L):
    _compare(hip, lr, b16, bu, batch, (L, L, L), (300, 3, 5000), rule="momentum", groups=[[0, 1, 2]])


def test_two_calls_from_one_start_give_the_same_bits(hip, lr, b16, bu):
    batch, bags, rows = _FORMS["lsd"]
    tables = _start("adagrad", "fp32", 8, batch, bags, rows)
    run = _Runner(hip, lr, b16, bu, tables, "adagrad", "fp32", 8, batch)
    a, b = run.ragged(), run.ragged()
    _assert_same(tables, a, b)


def test_route_strings(hip, lr, b16, bu):
    run, _, _ = _compare(hip, lr, b16, bu, 64, (1, 7, 3), (300, 3, 5000))
    assert run.route == "bags:small"
    run, _, _ = _compare(hip, lr, b16, bu, 500, (1, 7), (300, 40))      # 9-bit ids: one pass
    assert run.route == "bags:lsd:passes=1"


# ---- refusals: nothing runs ----------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_tables_alone(hip, lr, b16, bu):
    import torch
    batch, bags, rows = _FORMS["small"]
    tables = _start("adagrad", "fp32", 8, batch, bags, rows)
    run = _Runner(hip, lr, b16, bu, tables, "adagrad", "fp32", 8, batch)
    w, s0, s1 = run._fresh()
    bf_tabs = b16.tables([(run.idx[t], w[t], run.g[t], rows[t], 8) for t in range(3)])
    no_state = hip.emb_states([(None, None)] * 3)
    BAD, UNSUP, WS = -1, -3, -4
    cases = [
        ("in_dims < 1", dict(in_dims=[1, 0, 3]), BAD),
        ("null in_dims", dict(in_dims=None, ntables=3), BAD),
        ("both table arrays", dict(tables_bf16=bf_tabs, rounding=b16.rounding(B.ROUND_NEAREST)), BAD),
        ("neither table array", dict(tables=None), BAD),
        ("too many tables", dict(ntables=capi.BAGS_UPDATE_MAX_TABLES + 1), BAD),
        ("missing state", dict(states=no_state), BAD),
        ("null states", dict(states=None), BAD),
        ("in_dims above FFH_BAGS_MAX_IN_DIM", dict(in_dims=[1, capi.BAGS_MAX_IN_DIM + 1, 3]), UNSUP),
        ("batch * in_dims >= 2^31", dict(in_dims=[1, 7, 3], batch=2**31 // 7 + 1), UNSUP),
    ]
    for what, over, code in cases:
        assert bu.rc(run.descriptor(w, s0, s1, **over)) == code, what
    assert bu.rc(None) == BAD
    hip.set_workspace(run.ws, bu.workspace_bytes(bags, 8, batch) - 256)      # a workspace too small
    assert bu.rc(run.descriptor(w, s0, s1)) == WS
    hip.set_workspace(run.ws, run.ws_bytes)
    torch.cuda.synchronize()
    got = run._host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    bu.call(run.descriptor(w, s0, s1))      # ... and the same descriptor, unmodified, runs
    _assert_same(tables, run._host(w, s0, s1), run.uniform())


def test_argument_checks_on_bf16_tables(hip, lr, b16, bu):
    """The refusals of the bf16 descriptor, which is converted before the shared checks run: the per-call cap at 65 tables among them."""
    batch, bags, rows = _FORMS["small"]
    tables = _start("rowwise", "bf16", 8, batch, bags, rows)
    run = _Runner(hip, lr, b16, bu, tables, "rowwise", "bf16", 8, batch)
    w, s0, s1 = run._fresh()
    BAD, UNSUP = -1, -3
    cases = [
        ("too many tables", dict(ntables=capi.BAGS_UPDATE_MAX_TABLES + 1), BAD),
        ("in_dims < 1", dict(in_dims=[1, 0, 3]), BAD),
        ("null in_dims", dict(in_dims=None, ntables=3), BAD),
        ("null states", dict(states=None), BAD),
        ("in_dims above FFH_BAGS_MAX_IN_DIM", dict(in_dims=[1, capi.BAGS_MAX_IN_DIM + 1, 3]), UNSUP),
        ("batch * in_dims >= 2^31", dict(in_dims=[1, 7, 3], batch=2**31 // 7 + 1), UNSUP),
    ]
    for what, over, code in cases:
        assert bu.rc(run.descriptor(w, s0, s1, **over)) == code, what
    got = run._host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    bu.call(run.descriptor(w, s0, s1))      # ... and the same descriptor, unmodified, runs
    _assert_same(tables, run._host(w, s0, s1), run.uniform())


def test_bf16_momentum_takes_at_most_32_tables(hip, lr, b16, bu):
    batch, n = 8, 33
    tables = _start("momentum", "bf16", 8, batch, (1,) * (n - 1) + (2,), (7,) * n)
    run = _Runner(hip, lr, b16, bu, tables, "momentum", "bf16", 8, batch)
    w, s0, s1 = run._fresh()
    assert bu.rc(run.descriptor(w, s0, s1)) == -1
    got = run._host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])


def test_a_ragged_call_spoils_a_pending_sort(hip, lr, b16, bu):
    batch, bags, rows = _FORMS["small"]
    tables = _start("sgd", "fp32", 8, batch, bags, rows)
    run = _Runner(hip, lr, b16, bu, tables, "sgd", "fp32", 8, batch, plain=True)
    w, s0, s1 = run._fresh()
    one = run._tabs(w, [1])
    L = bags[1]
    hip.check(hip.lib.ffh_embedding_bwd_sort_multi(hip.ctx, one, 1, L, 8, batch, None), "sort_multi")
    bu.call(run.descriptor(w, s0, s1))
    after = run._host(w, s0, s1)
    assert hip.lib.ffh_embedding_bwd_sgd_apply_multi(hip.ctx, one, 1, L, 8, batch, capi.AGGR_MODE_SUM, run.rate, None) == -4
    got = run._host(w, s0, s1)
    np.testing.assert_array_equal(got["w"][1], after["w"][1])      # the refused apply ran nothing
    _assert_same(tables, got, run.uniform())
