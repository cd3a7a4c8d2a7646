"""The ragged table update in two calls (include/ff_hip_bags_sort.h): ffh_embedding_bwd_sort_multi_bags, then ffh_embedding_bwd_apply_multi_bags,
through the C-ABI.

The reference is always the fused ragged call (ffh_embedding_bwd_fused_multi_bags) from the same start; weights, every state array and bf16 bit
patterns are compared with assert_array_equal -- the pair launches what the fused call launches, so it promises its bits.  The sort call is given
a descriptor that holds ONLY what it may read (ids, row counts, bag sizes, ntables, out_dim, batch): null weights, gradients, states, rule,
rounding and rate block, a leading dimension of 0 and an aggregation mode that does not exist.

Shapes, starts and the runner are those of tests/test_gpu_bags_update.py (the smallest at which the layout can go wrong; read there why):
  small form    batch 64, bags (1, 7, 3), rows (300, 3, 5000): the sort lives in the apply kernel, the sort call launches nothing.
  sorted form   batch 500, bags (1, 100, 1, 7), rows (300, 3, 5000, 70000), and a second table order.
  a long list   batch 6,000, bags (100, 1), rows (5, 40,000).
Rows = 2 (mod 5) are hit by nobody and must keep weights and state."""
import ctypes as C

import numpy as np
import pytest

import bf16_helpers as B
import test_gpu_bags_update as U
from dlrm_flexflow_amd import capi

pytestmark = pytest.mark.gpu
DEV = U.DEV
WS_ERR = -4
_FORMS = U._FORMS
_ROUTE = {"small": "bags:small", "lsd": "bags:lsd:passes=2"}
_SWEEP = U._SWEEP
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


@pytest.fixture(scope="module")
def bs(hip):
    return capi.bags_sort_api(hip)


class _Pair(U._Runner):
    """The runner of tests/test_gpu_bags_update.py with the two-call form beside the fused one."""

    def __init__(self, bs, *args, **kw):
        super().__init__(*args, **kw)
        self.bs = bs
        self.counter = self.torch.tensor([U.IT], dtype=self.torch.int64, device=DEV)      # (kept alive across the two calls)
        self.routes = None

    def _rounding(self):
        return self.b16.rounding(self.mode, U.SEED, self.counter)

    def _route(self):
        return self.hip.lib.ffh_embedding_last_route(self.hip.ctx).decode()

    def sort_descriptor(self):
        """what the sort may read, and nothing else"""
        ent = [(self.idx[t], None, None, tb["R"], 0) for t, tb in enumerate(self.tables)]
        kw = dict(in_dims=self.bags, out_dim=self.D, batch=self.batch, aggr=77)
        if self.wt == "fp32":
            kw["tables"] = self.hip.emb_tables(ent)
        else:
            kw["tables_bf16"] = self.b16.tables([e + (10 + t, 0) for t, e in enumerate(ent)])
        return capi.BagsUpdateApi.descriptor(**kw)

    def pair(self, sort_stream=None, apply_stream=None, between=None):
        """sort, (`between`), apply from a fresh start; the tables as numpy"""
        w, s0, s1 = self._fresh()
        self.torch.cuda.synchronize()
        self.bs.sort(self.sort_descriptor(), sort_stream)
        routes = [self._route()]
        if between is not None:
            between(w)
        self.bs.apply(self.descriptor(w, s0, s1), apply_stream)
        routes.append(self._route())
        self.routes = routes
        if apply_stream is not None:
            self.hip.check(self.hip.lib.ffh_stream_sync(self.hip.ctx, apply_stream), "sync")
        out = self._host(w, s0, s1)
        assert int(self.counter.cpu()[0]) == U.IT      # neither call advances the update counter
        return out


def _make(hip, lr, b16, bu, bs, form_or_shape, rule="sgd", wt="fp32", D=8, tag=0, **kw):
    batch, bags, rows = _FORMS[form_or_shape] if isinstance(form_or_shape, str) else form_or_shape
    tables = U._start(rule, wt, D, batch, bags, rows, tag)
    return _Pair(bs, hip, lr, b16, bu, tables, rule, wt, D, batch, **kw), tables


def _compare(hip, lr, b16, bu, bs, shape, route=None, **kw):
    run, tables = _make(hip, lr, b16, bu, bs, shape, **kw)
    ref = run.ragged()
    got = run.pair()
    if route is not None:
        assert run.route == route and run.routes == [route, route], (run.route, run.routes)
    U._assert_same(tables, got, ref)
    return run, tables


# ---- the forms -----------------------------------------------------------------------------------------------------------------------
def test_small_form_the_sort_call_only_leaves_the_note(hip, lr, b16, bu, bs):
    _compare(hip, lr, b16, bu, bs, "small", route="bags:small")


@pytest.mark.parametrize("bags,rows", [((1, 100, 1, 7), (300, 3, 5000, 70000)), ((7, 1, 1, 100), (70000, 5000, 300, 3))], ids=["heavy-middle", "heavy-last"])
def test_sorted_form_in_two_table_orders(hip, lr, b16, bu, bs, bags, rows):
    _compare(hip, lr, b16, bu, bs, (500, bags, rows), route="bags:lsd:passes=2")


def test_a_long_list_beside_a_short_one(hip, lr, b16, bu, bs):
    _compare(hip, lr, b16, bu, bs, (6000, (100, 1), (5, 40000)), route="bags:lsd:passes=2")


@pytest.mark.parametrize("rule,wt,vec,form,entry", _SWEEP, ids=["-".join(map(str, c)) for c in _SWEEP])
def test_every_rule_weight_type_width_and_entry(hip, lr, b16, bu, bs, rule, wt, vec, form, entry):
    _compare(hip, lr, b16, bu, bs, form, rule=rule, wt=wt, D=U._DIMS[vec], entry=entry, route=_ROUTE[form])


@pytest.mark.parametrize("wt", ["fp32", "bf16"])
def test_plain_sgd_without_a_rule(hip, lr, b16, bu, bs, wt):
    _compare(hip, lr, b16, bu, bs, "lsd", wt=wt, plain=True, route=_ROUTE["lsd"])


@pytest.mark.parametrize("form", list(_FORMS))
def test_avg(hip, lr, b16, bu, bs, form):
    _compare(hip, lr, b16, bu, bs, form, rule="adagrad", aggr=capi.AGGR_MODE_AVG, tag=1, route=_ROUTE[form])


@pytest.mark.parametrize("form", list(_FORMS))
def test_stochastic_rounding_with_the_same_counter(hip, lr, b16, bu, bs, form):
    _compare(hip, lr, b16, bu, bs, form, rule="rowwise", wt="bf16", mode=B.ROUND_STOCHASTIC, route=_ROUTE[form])


# ---- ordering is the caller's: streams and an event -----------------------------------------------------------------------------------
@pytest.fixture()
def two_streams(hip):
    s1, s2, ev = C.c_void_p(), C.c_void_p(), C.c_void_p()
    hip.check(hip.lib.ffh_stream_create(hip.ctx, C.byref(s1)), "stream")
    hip.check(hip.lib.ffh_stream_create(hip.ctx, C.byref(s2)), "stream")
    hip.check(hip.lib.ffh_event_create(hip.ctx, C.byref(ev)), "event")
    yield s1.value, s2.value, ev.value
    import torch
    torch.cuda.synchronize()
    hip.check(hip.lib.ffh_event_destroy(hip.ctx, ev), "event destroy")
    hip.check(hip.lib.ffh_stream_destroy(hip.ctx, s1), "stream destroy")
    hip.check(hip.lib.ffh_stream_destroy(hip.ctx, s2), "stream destroy")


@pytest.mark.parametrize("gather_between", [False, True], ids=["bare", "gather-between"])
def test_sort_on_one_stream_apply_on_another_behind_an_event(hip, lr, b16, bu, bs, two_streams, gather_between):
    """The sort on one stream, the apply on another behind an event; once with the gather of the same tables between the two (it reads the
    ids and the weights and does not touch the workspace -- the step's own order)."""
    import torch
    s1, s2, ev = two_streams
    run, tables = _make(hip, lr, b16, bu, bs, "lsd", rule="adagrad")
    ref = run.ragged()
    bags_api = capi.bags_api(hip)
    out = [torch.zeros((run.batch, run.D), dtype=torch.float32, device=DEV) for _ in tables]
    torch.cuda.synchronize()

    def between(w):
        if gather_between:
            tabs = hip.emb_tables([(run.idx[t], w[t], out[t], tb["R"], run.D) for t, tb in enumerate(tables)])
            bags_api.call("ffh_embedding_fwd_multi_bags", tabs, capi.BagsApi.in_dims(run.bags), len(tables), run.D, run.batch, capi.AGGR_MODE_SUM, stream=s1)
        hip.check(hip.lib.ffh_event_record(hip.ctx, ev, s1), "record")
        hip.check(hip.lib.ffh_stream_wait_event(hip.ctx, s2, ev), "wait")

    got = run.pair(sort_stream=s1, apply_stream=s2, between=between)
    U._assert_same(tables, got, ref)
    if gather_between:      # the gather saw the weights of before the apply
        for t, tb in enumerate(tables):
            terms = tb["w"][tb["idx"]].astype(np.float64)      # [batch][L][D]; an fp32 sum of L terms in any order: within L * 2^-23 of the terms' mass
            bound = tb["L"] * 2.0**-23 * np.abs(terms).sum(1) + 1e-7
            assert (np.abs(out[t].cpu().numpy() - terms.sum(1)) <= bound).all(), f"table {t}: the gather between the calls did not see the start's weights"


# ---- the note: one apply per sort, of the same tables, on the same workspace ---------------------------------------------------------------
def _uniform_one(run, w, what, t=1):
    """a uniform call on table t alone (plain SGD entries): "fused", "sort" or "apply"; returns the status code"""
    hip = run.hip
    one, L = run._tabs(w, [t]), run.bags[t]
    if what == "sort":
        return hip.lib.ffh_embedding_bwd_sort_multi(hip.ctx, one, 1, L, run.D, run.batch, None)
    fn = hip.lib.ffh_embedding_bwd_sgd_fused_multi if what == "fused" else hip.lib.ffh_embedding_bwd_sgd_apply_multi
    return fn(hip.ctx, one, 1, L, run.D, run.batch, capi.AGGR_MODE_SUM, 0.01, None)


_REFUSALS = ["no-sort", "second-apply", "bag-list-of-the-same-sum", "batch", "idx-pointer", "ragged-fused-between", "uniform-fused-between",
             "uniform-sort-between", "uniform-note-for-the-ragged-apply", "workspace"]


@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("case", _REFUSALS)
def test_the_apply_refuses_without_a_matching_fresh_sort(hip, lr, b16, bu, bs, form, case):
    """Each refusal is FFH_ERR_WORKSPACE with every weight and state byte as it was; a fresh sort + apply afterwards gives the fused bits."""
    import torch
    run, tables = _make(hip, lr, b16, bu, bs, form, rule="adagrad")
    ref = run.ragged()                      # (a fused call: whatever note an earlier test left on this workspace is gone)
    w, s0, s1 = run._fresh()                # the tables the refused apply is pointed at
    w2, t0, t1 = run._fresh()               # ... and those the work in between runs on
    torch.cuda.synchronize()
    over = {}
    if case == "no-sort":
        pass
    elif case == "second-apply":
        bs.sort(run.sort_descriptor())
        bs.apply(run.descriptor(w2, t0, t1))
    elif case == "bag-list-of-the-same-sum":
        bs.sort(run.sort_descriptor())
        over = dict(in_dims=list(reversed(run.bags)))      # (1, 7, 3) against (3, 7, 1): the same lookups in all, another layout
        assert list(reversed(run.bags)) != list(run.bags)
    elif case == "batch":
        bs.sort(run.sort_descriptor())
        over = dict(batch=run.batch - 1)
    elif case == "idx-pointer":
        bs.sort(run.sort_descriptor())
        other_ids = run.idx[0].clone()                     # the same ids at another address
        over = dict(tables=hip.emb_tables([(other_ids if t == 0 else run.idx[t], w[t], run.g[t], tb["R"], run.D) for t, tb in enumerate(tables)]))
    elif case == "ragged-fused-between":
        bs.sort(run.sort_descriptor())
        bu.call(run.descriptor(w2, t0, t1))
    elif case == "uniform-fused-between":
        bs.sort(run.sort_descriptor())
        assert _uniform_one(run, w2, "fused") == 0
    elif case == "uniform-sort-between":
        bs.sort(run.sort_descriptor())
        assert _uniform_one(run, w2, "sort") == 0
    elif case == "uniform-note-for-the-ragged-apply":
        assert _uniform_one(run, w2, "sort") == 0
    elif case == "workspace":
        bs.sort(run.sort_descriptor())
        other = torch.empty(run.ws_bytes, dtype=torch.uint8, device=DEV)
        hip.set_workspace(other, run.ws_bytes)
    assert bs.apply_rc(run.descriptor(w, s0, s1, **over)) == WS_ERR, case
    if case == "workspace":
        hip.set_workspace(run.ws, run.ws_bytes)
    got = run._host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"], err_msg=f"{case}: table {t}: the refused apply wrote weights")
        np.testing.assert_array_equal(got["s0"][t], tb["s0"], err_msg=f"{case}: table {t}: the refused apply wrote state")
    U._assert_same(tables, run.pair(), ref)      # after the refusal: a fresh pair is the fused call


@pytest.mark.parametrize("form", list(_FORMS))
def test_a_ragged_note_never_serves_the_uniform_apply(hip, lr, b16, bu, bs, form):
    """Tables of ONE bag size sorted by the ragged entry: the uniform apply of the very same tables still refuses, and the ragged apply then runs."""
    batch, L = _FORMS[form][0], 7
    run, tables = _make(hip, lr, b16, bu, bs, (batch, (L, L, L), (300, 3, 5000)), rule="sgd", plain=True)
    ref = run.ragged()
    w, s0, s1 = run._fresh()
    bs.sort(run.sort_descriptor())
    tabs = run._tabs(w, range(3))
    assert hip.lib.ffh_embedding_bwd_sgd_apply_multi(hip.ctx, tabs, 3, L, run.D, batch, capi.AGGR_MODE_SUM, run.rate, None) == WS_ERR
    got = run._host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
    bs.apply(run.descriptor(w, s0, s1))          # the refused uniform apply left the ragged note alone
    U._assert_same(tables, run._host(w, s0, s1), ref)


def test_argument_errors_are_the_fused_entrys(hip, lr, b16, bu, bs):
    """Same codes as ffh_embedding_bwd_fused_multi_bags, from both calls, with nothing launched and no note left behind."""
    run, tables = _make(hip, lr, b16, bu, bs, "lsd", rule="adagrad")
    ref = run.ragged()
    w, s0, s1 = run._fresh()
    BAD, UNSUP = -1, -3
    cases = [
        ("in_dims < 1", dict(in_dims=[1, 0, 3, 7]), BAD),
        ("null in_dims", dict(in_dims=None, ntables=4), BAD),
        ("neither table array", dict(tables=None), BAD),
        ("too many tables", dict(ntables=capi.BAGS_UPDATE_MAX_TABLES + 1), BAD),
        ("in_dims above FFH_BAGS_MAX_IN_DIM", dict(in_dims=[1, capi.BAGS_MAX_IN_DIM + 1, 3, 7]), UNSUP),
        ("batch * in_dims >= 2^31", dict(in_dims=[1, 7, 3, 1], batch=2**31 // 7 + 1), UNSUP),
    ]
    for what, over, code in cases:
        u = run.descriptor(w, s0, s1, **over)
        assert bu.rc(u) == code and bs.sort_rc(u) == code and bs.apply_rc(u) == code, what
    assert bs.sort_rc(None) == BAD and bs.apply_rc(None) == BAD
    assert bs.apply_rc(run.descriptor(w, s0, s1, states=None)) == BAD      # the apply alone reads the states
    hip.set_workspace(run.ws, bu.workspace_bytes(run.bags, run.D, run.batch) - 256)
    assert bs.sort_rc(run.sort_descriptor()) == WS_ERR
    hip.set_workspace(run.ws, run.ws_bytes)
    assert bs.apply_rc(run.descriptor(w, s0, s1)) == WS_ERR                 # none of the refused sorts left a note
    got = run._host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    U._assert_same(tables, run.pair(), ref)
