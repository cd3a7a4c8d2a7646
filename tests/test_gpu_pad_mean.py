"""Mean pooling over variable-length embedding bags (include/ff_hip_pad_mean.h) through the C-ABI, bit for bit against the header's identities
(tests/pad_mean_helpers.py): the EXISTING pad entries in SUM mode with the division by max(count, 1) done on the host in float32, and -- with
no pad in the input -- the existing ragged entries in AVG mode on the same tables.  The shapes are those of tests/test_gpu_pad.py.  Every id
pattern carries one empty bag, one full bag and one bag with exactly one lookup per table of more than one slot (pin_counts)."""
import numpy as np
import pytest

import bf16_helpers as B
import pad_helpers as PH
import pad_mean_helpers as PM
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
DEV = PH.DEV
SUM, AVG = capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG
BAD, UNSUP, WS = capi.FFH_ERR_BAD_ARG, capi.FFH_ERR_UNSUPPORTED, -4
GATHER_BAGS = PM.GATHER_BAGS
FORMS = {"small": (64, (1, 7, 32), "bags:small:pad:mean"), "lsd": (500, (7, 1, 100), "bags:lsd:passes=%d:pad:mean")}
ROWS = (300, 3, 5000)


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def bags(hip):
    return capi.bags_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


@pytest.fixture(scope="module")
def pd(hip):
    return capi.pad_api(hip)


@pytest.fixture(scope="module")
def pm(hip):
    return capi.pad_mean_api(hip)


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("batch", [37, 600])
@pytest.mark.parametrize("D", [4, 6, 16, 128])
def test_mean_gather_equals_the_scaled_pad_gather(hip, D, batch, bf16):
    """Identity 2, the numpy restatement, +0 for a bag of only pads, the sentinel columns; pattern "none": identity 1."""
    for pattern in PH.PATTERNS:
        W, ids = PM.gather_case(D, batch, bf16, pattern)
        got = PM.gather(hip, W, ids, D, batch, bf16, "mean")
        ref = PM.gather(hip, W, ids, D, batch, bf16, "pad-sum")      # the existing pad gather in SUM mode ...
        for t in range(len(GATHER_BAGS)):                           # ... times float32(1) / float32(max(count, 1)) on the host
            cols = slice(4 + t * D, 4 + (t + 1) * D)
            ref[:, cols] = ref[:, cols] * PM.inv_count(ids[t])[:, None]
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=pattern)      # and 7.0 wherever no table writes
        assert (got[:, :4] == 7.0).all() and (got[:, -4:] == 7.0).all()
        for t, L in enumerate(GATHER_BAGS):
            cols = slice(4 + t * D, 4 + (t + 1) * D)
            np.testing.assert_array_equal(got[:, cols].view(np.uint32), ffmodel.padded_bag_reference(W[t], ids[t], mean=True).view(np.uint32),
                                          err_msg=f"{pattern} table {t}")
            cnt = ffmodel.padded_bag_counts(ids[t])
            assert not got[cnt == 0][:, cols].view(np.uint32).any(), f"{pattern} table {t}: a bag of only pads is not all +0"
            if L > 1:
                assert cnt[PM.EMPTY_BAG] == 0 and cnt[PM.FULL_BAG] == L and cnt[PM.ONE_BAG] == 1
    # identity 1 needs ids without any pad: the pinned bags carry pads, so it runs on the unpinned ids
    W, _ = PM.gather_case(D, batch, bf16, "none")
    rng = np.random.default_rng([PH.SEED, D, batch, 1])
    full = [rng.integers(0, PM.gather_rows(t), (batch, L)).astype(np.int64) for t, L in enumerate(GATHER_BAGS)]
    got = PM.gather(hip, W, full, D, batch, bf16, "mean")
    np.testing.assert_array_equal(got.view(np.uint32), PM.gather(hip, W, full, D, batch, bf16, "plain-avg").view(np.uint32), err_msg="no pads: the ragged AVG gather")


@pytest.mark.parametrize("math_mode", [1, 2], ids=["tensor-op-twin", "split-three-plane"])
def test_twin_and_three_plane_image_of_the_destination(hip, bags, pd, pm, math_mode):
    """The fp32 destination equals identity 2 to the bit, and the registered bf16 twin / three-plane image holds what the EXISTING pad gather
    writes for a table set whose sums are the scaled values: table t' has one row per sample, row b being the scaled output row b, gathered
    with bag size 1 and ids 0 .. batch - 1 in SUM mode (its sum is +0 + the row: the same fp32 values, and the twin of those).
    D = 16, ld = 96 (a multiple of 32), batch 37, the generator's pads at fill 0.5."""
    torch = torch_()
    D, batch = 16, 37
    nt, ld = len(GATHER_BAGS), 96
    W, ids = PM.gather_case(D, batch, False, "mask")
    reg = hip.lib.ffh_ctx_bf16_mirror_set if math_mode == 1 else hip.lib.ffh_ctx_bf16x3_mirror_set
    side_n = batch * ld if math_mode == 1 else batch * ld // 32 * 96
    out = torch.zeros((batch, ld), device=DEV)
    side = [torch.full((side_n,), 0x1111, dtype=torch.int16, device=DEV) for _ in range(2)]
    scaled = [ffmodel.padded_bag_reference(W[t], ids[t]) * PM.inv_count(ids[t])[:, None] for t in range(nt)]      # identity 2 on the host (the sum: test above)
    wd = [[torch.from_numpy(w).to(DEV) for w in W], [torch.from_numpy(np.ascontiguousarray(s)).to(DEV) for s in scaled]]
    rowid = torch.arange(batch, dtype=torch.int64, device=DEV)
    idd = [[torch.from_numpy(i).to(DEV) for i in ids], [rowid] * nt]
    tabs = lambda e: hip.emb_tables([(idd[e][t], wd[e][t], out.data_ptr() + 4 * D * t, PM.gather_rows(t) if e == 0 else batch, ld) for t in range(nt)])
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, math_mode) == 0
    try:
        try:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[0].data_ptr()) == 0
            pm.fwd(tabs(0), bags.in_dims(GATHER_BAGS), nt, D, batch, AVG)
            torch.cuda.synchronize()
            got = out.clone()
            out.zero_()
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[1].data_ptr()) == 0        # the same base: replaced
            pd.fwd(tabs(1), bags.in_dims([1] * nt), nt, D, batch, SUM)
            torch.cuda.synchronize()
        finally:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, None) == 0
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
    g = got.cpu().numpy()
    for t in range(nt):
        np.testing.assert_array_equal(g[:, t * D:(t + 1) * D].view(np.uint32), scaled[t].view(np.uint32), err_msg=f"table {t}")
    assert got.view(torch.int32).equal(out.view(torch.int32))
    assert torch.equal(side[0], side[1]), f"{int((side[0] != side[1]).sum())} of {side_n} mirror words differ"
    assert int((side[1] != 0x1111).sum()) > side_n // 4                                          # the existing kernel did write it


def test_gather_argument_checks_launch_nothing(hip, bags, b16, pm):
    torch = torch_()
    D, batch = 16, 37
    W, ids = PM.gather_case(D, batch, False, "mask")
    wd = [torch.from_numpy(w).to(DEV) for w in W[:2]]
    idd = [torch.from_numpy(i).to(DEV) for i in ids[:2]]
    out = torch.full((batch, 2 * D), 7.0, device=DEV)
    ent = [(idd[t], wd[t], out.data_ptr() + 4 * D * t, PM.gather_rows(t), 2 * D) for t in range(2)]
    for bf16, arr in ((False, hip.emb_tables(ent)), (True, b16.tables(ent))):
        assert pm.fwd_rc(arr, bags.in_dims(GATHER_BAGS[:2]), 2, D, batch, SUM, bf16=bf16) == BAD
        assert "ffh_embedding_fwd_multi_bags_pad" in hip.lib.ffh_last_error_string(hip.ctx).decode()
        assert pm.fwd_rc(arr, None, 2, D, batch, AVG, bf16=bf16) == BAD
        assert pm.fwd_rc(arr, bags.in_dims([1, 0]), 2, D, batch, AVG, bf16=bf16) == BAD
        assert pm.fwd_rc(arr, bags.in_dims([1, capi.BAGS_MAX_IN_DIM + 1]), 2, D, batch, AVG, bf16=bf16) == UNSUP
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the update ------------------------------------------------------------------------------------------------------------------------
def _passes(rows):
    """passes of the pad form: nine-bit digits over the bits that hold the largest pad key, max(rows)"""
    return (max(1, max(rows).bit_length()) + 8) // 9


def _compare(hip, rule, wt, D, form, rows, pattern="mask", tag=0, ids=None, **kw):
    batch, bag_list, route = FORMS[form]
    tables = PM.start(rule, wt, D, batch, bag_list, rows, pattern, tag, ids)
    run = PM.MeanRunner(hip, tables, rule, wt, D, batch, **kw)
    got = run.mean()
    assert run.route == (route % _passes(rows) if "%" in route else route), run.route
    PH.assert_same(tables, got, run.ref(), f"{rule}/{wt}/D={D}/{form}/{pattern}")
    return run, tables, got


_RULES = list(PH.KINDS) + ["plain"]
_WEIGHTS = {"fp32": ("fp32", B.ROUND_NEAREST), "bf16-nearest": ("bf16", B.ROUND_NEAREST), "bf16-stochastic": ("bf16", B.ROUND_STOCHASTIC)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("D", [4, 6, 16])
@pytest.mark.parametrize("weights", list(_WEIGHTS))
@pytest.mark.parametrize("rule", _RULES)
def test_every_rule_weight_type_rounding_and_width(hip, rule, weights, D, form):
    """Identity 3 for every ffh_sparse_opt kind and plain SGD without a rule; the pads are the generator's at fill 0.5 plus the pinned bags."""
    wt, mode = _WEIGHTS[weights]
    plain = rule == "plain"
    _compare(hip, "sgd" if plain else rule, wt, D, form, ROWS, mode=mode, plain=plain)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wt", ["fp32", "bf16"])
def test_without_pads_the_mean_update_is_the_ragged_avg_update(hip, wt, form):
    """Identity 1: pattern "none" without the pinned bags, against ffh_embedding_bwd_fused_multi_bags with FFH_AGGR_MODE_AVG on the same tables."""
    batch, bag_list, _ = FORMS[form]
    tables = PM.start("momentum", wt, 16, batch, bag_list, ROWS, "none", pin=False)
    run = PM.MeanRunner(hip, tables, "momentum", wt, 16, batch)
    got = run.mean()
    PH.assert_same(tables, got, run.plain_avg(), "no pads: the ragged AVG update")
    PH.assert_same(tables, got, run.ref(), "no pads: identity 3")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("pattern", [p for p in PH.PATTERNS if p not in ("mask", "all")])
def test_pad_patterns(hip, pattern, form):
    _compare(hip, "momentum", "fp32", 16, form, ROWS, pattern=pattern)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wt", ["fp32", "bf16"])
def test_tables_of_only_pads_change_no_byte(hip, wt, form):
    batch, bag_list, _ = FORMS[form]
    tables = PM.start("adam", wt, 16, batch, bag_list, ROWS, "all", pin=False)
    run = PM.MeanRunner(hip, tables, "adam", wt, 16, batch, mode=B.ROUND_STOCHASTIC)
    got = run.mean()
    for t, tb in enumerate(tables):
        assert not tb["hit"].any()
        for k in ("w", "s0", "s1"):
            np.testing.assert_array_equal(got[k][t], tb[k], err_msg=f"table {t}: {k}")


def test_duplicates_of_one_row_across_chunk_boundaries_with_pads_between(hip):
    """The ids of the test of that name in tests/test_gpu_pad.py: bags of 100 on batch 500, positions 0, 2, 4, ... hold row 1, positions 1, 3,
    5, ... are pads (every seventh: row 0), so row 1's 25,000 entries cross every FFH_EMB_CHUNK and FFH_EMB_CHUNK1 cut of the sorted list."""
    batch, bag_list, _ = FORMS["lsd"]
    rng = np.random.default_rng(3)
    ids = [rng.integers(0, 511, (batch, bag_list[0])), rng.integers(0, 2, (batch, bag_list[1]))]
    heavy = np.full(batch * 100, PH.PAD, np.int64)
    heavy[0::2] = 1
    heavy[1::14] = 0
    ids.append(heavy.reshape(batch, 100))
    for rule in ("sgd", "rowwise"):
        _compare(hip, rule, "fp32", 16, "lsd", (511, 2, 3), ids=ids)


def test_rate_from_the_lr_block(hip):
    for form in FORMS:
        _compare(hip, "adam", "bf16", 16, form, ROWS, lr_block=True)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wt", ["fp32", "bf16"])
def test_pad_sort_and_mean_apply_equal_the_fused_call(hip, wt, form):
    batch, bag_list, _ = FORMS[form]
    tables = PM.start("adagrad", wt, 16, batch, bag_list, (512, 3, 5000), "mask")
    run = PM.MeanRunner(hip, tables, "adagrad", wt, 16, batch)
    fused, pair = run.mean(), run.mean(pair=True)
    PH.assert_same(tables, pair, fused, "pair against fused")
    PH.assert_same(tables, run.mean(), fused, "a second fused call from the same start")
    PH.assert_same(tables, fused, run.ref(pair=True), "identity 3, the reference run as the pair")


@pytest.mark.parametrize("form", list(FORMS))
def test_a_pad_sort_feeds_one_apply_and_a_plain_sort_none(hip, form):
    batch, bag_list, _ = FORMS[form]
    tables = PM.start("adagrad", "fp32", 16, batch, bag_list, ROWS, "none", pin=False)      # (no pads: the ids are valid for either sort)
    run = PM.MeanRunner(hip, tables, "adagrad", "fp32", 16, batch)
    w, s0, s1 = run.fresh()
    u = run.descriptor(w, s0, s1, aggr=AVG)
    run.bs.sort(u)
    assert run.pm.apply_rc(u) == WS          # a plain sort, the mean apply
    got = run.host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    run.pd.sort(u)                           # a pad sort feeds the mean apply ...
    run.pm.apply(u)
    assert run.pm.apply_rc(u) == WS          # ... exactly once
    assert run.pd.apply_rc(run.descriptor(w, s0, s1)) == WS      # and the pad apply finds nothing left either
    PH.assert_same(tables, run.host(w, s0, s1), run.ref())


def test_update_argument_checks_leave_the_tables_alone(hip, b16):
    torch = torch_()
    batch, bag_list, _ = FORMS["small"]
    tables = PM.start("adagrad", "fp32", 8, batch, bag_list, ROWS, "mask")
    run = PM.MeanRunner(hip, tables, "adagrad", "fp32", 8, batch)
    w, s0, s1 = run.fresh()
    cases = [("SUM", dict(aggr=SUM), BAD), ("null in_dims", dict(in_dims=None, ntables=3, aggr=AVG), BAD)]
    for entry in (run.pm.fused_rc, run.pm.apply_rc):
        for what, over, code in cases:
            assert entry(run.descriptor(w, s0, s1, **over)) == code, what
        assert entry(run.descriptor(w, s0, s1, aggr=SUM)) == BAD and "_multi_bags_pad" in hip.lib.ffh_last_error_string(hip.ctx).decode()
    assert run.pm.fused_rc(None) == BAD
    big = run.descriptor(w, s0, s1, aggr=AVG)
    big.tables[1].num_entries = 2**32 - 1      # above 2^32 - 2: the pad key would be the reduce kernel's "no key"
    assert run.pm.fused_rc(big) == UNSUP
    # a workspace of the old query's size: too small for the counts
    small_ws = torch.empty(run.old_ws_bytes, dtype=torch.uint8, device=DEV)
    hip.set_workspace(small_ws, run.old_ws_bytes)
    try:
        assert run.pm.fused_rc(run.descriptor(w, s0, s1, aggr=AVG)) == WS
        run.pd.sort(run.descriptor(w, s0, s1))
        assert run.pm.apply_rc(run.descriptor(w, s0, s1, aggr=AVG)) == WS
    finally:
        hip.set_workspace(run.ws, run.ws_bytes)
    got = run.host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    run.pm.fused(run.descriptor(w, s0, s1, aggr=AVG))      # ... and the same descriptor, unmodified, runs
    PH.assert_same(tables, run.host(w, s0, s1), run.ref())
