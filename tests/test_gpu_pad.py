"""Variable-length embedding bags (include/ff_hip_pad.h) through the C-ABI, bit for bit against the header's zero-row reference
(tests/pad_helpers.py): the existing ragged entries on the table with one all-zero row appended and every pad pointed at it.

Shapes, read off bag_rows (embedding_fwd.hip), emb_bwd_bags (embedding.hip) and emb_bags_update.h:
  gather   bags (1, 3, 4, 7, 100) in one call: L = 1, the short-bag form (U = 4, one id per row in flight), exactly one group of four ids of the
           long-bag form, one group plus a tail of three, and a long bag; D = 4, 16, 128 (16-byte form; 1, 4 and 32 lanes per row) and 6 (scalar
           form); batch 37 (a partial row block) and 600 (several workgroups per table).
  update   small form: batch 64, bags (1, 7, 32): N_t = 64 / 448 / 2048 <= 2048; sorted form: batch 500, bags (7, 1, 100): N_t = 3500 / 500 / 50000,
           none a multiple of the reduce tile, 3500 and 500 no multiples of FFH_EMB_CHUNK1 (1024), 500 none of FFH_EMB_CHUNK (32).
           Row counts 1, 2, 511, 512, 513, 262144: at 512 and 262144 the pad key needs a digit the real ids do not."""
import numpy as np
import pytest

import bf16_helpers as B
import pad_helpers as PH
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
DEV = PH.DEV
SUM, AVG = capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG
BAD, UNSUP, WS = capi.FFH_ERR_BAD_ARG, capi.FFH_ERR_UNSUPPORTED, -4
GATHER_BAGS = (1, 3, 4, 7, 100)
FORMS = {"small": (64, (1, 7, 32), "bags:small:pad"), "lsd": (500, (7, 1, 100), "bags:lsd:passes=%d:pad")}


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


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
def _rows(t):
    return 23 + 17 * t


def _gather_case(D, batch, bf16, pattern):
    rng = np.random.default_rng([PH.SEED, D, batch])
    W, ids = [], []
    for t, L in enumerate(GATHER_BAGS):
        w = rng.standard_normal((_rows(t), D)).astype(np.float32)
        w[0, :] = -0.0                                              # (+0) + (-0) = +0
        if bf16:
            w = B.widen(B.rne(w))
        i = rng.integers(0, _rows(t), (batch, L)).astype(np.int64)
        i[1, :] = 0                                                 # a bag of the -0 row alone (where the pattern leaves it)
        W.append(w)
        ids.append(PH.apply_pattern(i, pattern, t, len(GATHER_BAGS)))
    return W, ids


def _gather(hip, bags, b16, pd, W, ids, D, batch, bf16, which):
    """[batch][ld] with 7.0 where nothing may be written.  which: "pad" (the pad entry, tables of R rows), "zero-row" (the existing entry on the
    extended tables) or "plain" (the existing entry on the same tables: only for ids without pads)."""
    torch = torch_()
    nt, ld = len(GATHER_BAGS), 4 + len(GATHER_BAGS) * D + 4
    out = torch.full((batch, ld), 7.0, device=DEV)
    ext = which == "zero-row"
    conv = (lambda w: torch.from_numpy(B.rne(w).view(np.int16)).to(DEV)) if bf16 else (lambda w: torch.from_numpy(w).to(DEV))
    wd = [conv(PH.extend(w) if ext else w) for w in W]
    idd = [torch.from_numpy(PH.to_zero_row(i, _rows(t)) if ext else i).to(DEV) for t, i in enumerate(ids)]
    ent = [(idd[t], wd[t], out.data_ptr() + 4 * (4 + t * D), _rows(t) + (1 if ext else 0), ld) for t in range(nt)]
    arr = b16.tables(ent) if bf16 else hip.emb_tables(ent)
    dims = bags.in_dims(GATHER_BAGS)
    if which == "pad":
        pd.fwd(arr, dims, nt, D, batch, SUM, bf16=bf16)
    else:
        bags.call("ffh_embedding_fwd_multi_bags_bf16" if bf16 else "ffh_embedding_fwd_multi_bags", arr, dims, nt, D, batch, SUM)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("batch", [37, 600])
@pytest.mark.parametrize("D", [4, 6, 16, 128])
def test_pad_gather_equals_the_zero_row_gather(hip, bags, b16, pd, D, batch, bf16):
    for pattern in PH.PATTERNS:
        W, ids = _gather_case(D, batch, bf16, pattern)
        got = _gather(hip, bags, b16, pd, W, ids, D, batch, bf16, "pad")
        ref = _gather(hip, bags, b16, pd, W, ids, D, batch, bf16, "plain" if pattern == "none" else "zero-row")
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=pattern)      # and 7.0 wherever no table writes
        for t in range(len(GATHER_BAGS)):
            cols = slice(4 + t * D, 4 + (t + 1) * D)
            np.testing.assert_array_equal(got[:, cols].view(np.uint32), ffmodel.padded_bag_reference(W[t], ids[t]).view(np.uint32), err_msg=f"{pattern} table {t}")
            empty = (ids[t] < 0).all(axis=1)
            assert not got[empty, cols].view(np.uint32).any(), f"{pattern} table {t}: a bag of only pads is not all +0"
        if pattern == "all":
            assert not got[:, 4:-4].view(np.uint32).any()
        if pattern == "mask":
            n = sum(int((i < 0).sum()) for i in ids)
            assert 0.4 < n / sum(i.size for i in ids) < 0.6


@pytest.mark.parametrize("math_mode", [1, 2], ids=["tensor-op-twin", "split-three-plane"])
def test_twin_and_three_plane_image_of_the_destination(hip, bags, pd, math_mode):
    """With a registered bf16 twin or three-plane image of the destination the pad gather leaves in it what ffh_embedding_fwd_multi_bags writes
    on the zero-row tables.  D = 16, ld = 96 (a multiple of 32), batch 37, the generator's pads at fill 0.5."""
    torch = torch_()
    D, batch = 16, 37
    nt, ld = len(GATHER_BAGS), 96
    W, ids = _gather_case(D, batch, False, "mask")
    reg = hip.lib.ffh_ctx_bf16_mirror_set if math_mode == 1 else hip.lib.ffh_ctx_bf16x3_mirror_set
    side_n = batch * ld if math_mode == 1 else batch * ld // 32 * 96
    out = torch.zeros((batch, ld), device=DEV)
    side = [torch.full((side_n,), 0x1111, dtype=torch.int16, device=DEV) for _ in range(2)]
    wd = [[torch.from_numpy(w).to(DEV) for w in W], [torch.from_numpy(PH.extend(w)).to(DEV) for w in W]]
    idd = [[torch.from_numpy(i).to(DEV) for i in ids], [torch.from_numpy(PH.to_zero_row(i, _rows(t))).to(DEV) for t, i in enumerate(ids)]]
    tabs = lambda e: hip.emb_tables([(idd[e][t], wd[e][t], out.data_ptr() + 4 * D * t, _rows(t) + e, ld) for t in range(nt)])
    dims = bags.in_dims(GATHER_BAGS)
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, math_mode) == 0
    try:
        try:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[0].data_ptr()) == 0
            pd.fwd(tabs(0), dims, nt, D, batch, SUM)
            torch.cuda.synchronize()
            got = out.clone()
            out.zero_()
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[1].data_ptr()) == 0        # the same base: replaced
            bags.call("ffh_embedding_fwd_multi_bags", tabs(1), dims, nt, D, batch, SUM)
            torch.cuda.synchronize()
        finally:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, None) == 0
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
    assert got.view(torch.int32).equal(out.view(torch.int32))
    assert torch.equal(side[0], side[1]), f"{int((side[0] != side[1]).sum())} of {side_n} mirror words differ"
    assert int((side[1] != 0x1111).sum()) > side_n // 4                                          # the existing kernel did write it


def test_gather_argument_checks_launch_nothing(hip, bags, b16, pd):
    torch = torch_()
    D, batch = 16, 37
    W, ids = _gather_case(D, batch, False, "mask")
    wd = [torch.from_numpy(w).to(DEV) for w in W[:2]]
    idd = [torch.from_numpy(i).to(DEV) for i in ids[:2]]
    out = torch.full((batch, 2 * D), 7.0, device=DEV)
    ent = [(idd[t], wd[t], out.data_ptr() + 4 * D * t, _rows(t), 2 * D) for t in range(2)]
    for bf16, arr in ((False, hip.emb_tables(ent)), (True, b16.tables(ent))):
        assert pd.fwd_rc(arr, bags.in_dims(GATHER_BAGS[:2]), 2, D, batch, AVG, bf16=bf16) == UNSUP
        assert pd.fwd_rc(arr, None, 2, D, batch, SUM, bf16=bf16) == BAD
        assert pd.fwd_rc(arr, bags.in_dims([1, 0]), 2, D, batch, SUM, bf16=bf16) == BAD
        assert pd.fwd_rc(arr, bags.in_dims([1, capi.BAGS_MAX_IN_DIM + 1]), 2, D, batch, SUM, bf16=bf16) == UNSUP
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the update ------------------------------------------------------------------------------------------------------------------------
def _passes(rows):
    """passes of the pad form: nine-bit digits over the bits that hold the largest pad key, max(rows)"""
    return (max(1, max(rows).bit_length()) + 8) // 9


def _compare(hip, rule, wt, D, form, rows, pattern="mask", tag=0, ids=None, **kw):
    batch, bag_list, route = FORMS[form]
    tables = PH.start(rule, wt, D, batch, bag_list, rows, pattern, tag, ids)
    run = PH.UpdateRunner(hip, tables, rule, wt, D, batch, **kw)
    got = run.pad()
    assert run.route == (route % _passes(rows) if "%" in route else route), run.route
    PH.assert_same(tables, got, run.zero_row(), f"{rule}/{wt}/D={D}/{form}/{pattern}")
    return run, tables, got


_RULES = list(PH.KINDS) + ["plain"]
_WEIGHTS = {"fp32": ("fp32", B.ROUND_NEAREST), "bf16-nearest": ("bf16", B.ROUND_NEAREST), "bf16-stochastic": ("bf16", B.ROUND_STOCHASTIC)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("D", [4, 6, 16])
@pytest.mark.parametrize("weights", list(_WEIGHTS))
@pytest.mark.parametrize("rule", _RULES)
def test_every_rule_weight_type_rounding_and_width(hip, rule, weights, D, form):
    """Every ffh_sparse_opt kind and plain SGD without a rule; the pads are the generator's at fill 0.5, so rows are hit by real lookups and by
    pads in one step.  Rows (300, 3, 5000): the 3-row table's runs cross every chunk and tile with pads between their entries."""
    wt, mode = _WEIGHTS[weights]
    plain = rule == "plain"
    _compare(hip, "sgd" if plain else rule, wt, D, form, (300, 3, 5000), mode=mode, plain=plain)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("R", [1, 2, 511, 512, 513, 262144])
def test_row_counts_around_a_digit_of_the_pad_key(hip, R, form):
    """The pad key R needs bit_length(R) bits: at 512 and 262144 one digit more than the ids 0 .. R - 1 (the route string counts the passes)."""
    assert [_passes([r]) for r in (1, 2, 511, 512, 513, 262143, 262144)] == [1, 1, 1, 2, 2, 2, 3]
    for wt in ("fp32", "bf16"):
        _compare(hip, "adagrad", wt, 4, form, (R, R, R))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("pattern", [p for p in PH.PATTERNS if p not in ("mask", "all")])
def test_pad_patterns(hip, pattern, form):
    run, tables, got = _compare(hip, "momentum", "fp32", 16, form, (300, 3, 5000), pattern=pattern)
    if pattern == "none":      # ... and with no pad in the input: the existing entry on the SAME tables
        w, s0, s1 = run.fresh()
        run.bu.call(run.descriptor(w, s0, s1))
        PH.assert_same(tables, got, run.host(w, s0, s1), "no pads, same tables")
    if pattern == "one-table":
        np.testing.assert_array_equal(got["w"][1], tables[1]["w"])
        np.testing.assert_array_equal(got["s0"][1], tables[1]["s0"])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wt", ["fp32", "bf16"])
def test_tables_of_only_pads_change_no_byte(hip, wt, form):
    batch, bag_list, _ = FORMS[form]
    tables = PH.start("adam", wt, 16, batch, bag_list, (300, 3, 5000), "all")
    run = PH.UpdateRunner(hip, tables, "adam", wt, 16, batch, mode=B.ROUND_STOCHASTIC)
    got = run.pad()
    for t, tb in enumerate(tables):
        assert not tb["hit"].any()
        for k in ("w", "s0", "s1"):
            np.testing.assert_array_equal(got[k][t], tb[k], err_msg=f"table {t}: {k}")


def test_duplicates_of_one_row_across_chunk_boundaries_with_pads_between(hip):
    """Bags of 100 on batch 500: positions 0, 2, 4, ... hold row 1, positions 1, 3, 5, ... are pads (every seventh: row 0).  Row 1's 25,000
    entries cross every FFH_EMB_CHUNK and FFH_EMB_CHUNK1 cut of the sorted list, and in position order pads lie between any two of them."""
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
        _compare(hip, "adam", "bf16", 16, form, (300, 3, 5000), lr_block=True)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wt", ["fp32", "bf16"])
def test_sort_and_apply_pair_equals_the_fused_call(hip, wt, form):
    batch, bag_list, _ = FORMS[form]
    tables = PH.start("adagrad", wt, 16, batch, bag_list, (512, 3, 5000), "mask")
    run = PH.UpdateRunner(hip, tables, "adagrad", wt, 16, batch)
    fused, pair = run.pad(), run.pad(pair=True)
    PH.assert_same(tables, pair, fused, "pair against fused")
    PH.assert_same(tables, run.pad(), fused, "a second fused call from the same start")


@pytest.mark.parametrize("form", list(FORMS))
def test_a_pad_sort_and_a_plain_apply_do_not_mix(hip, form):
    batch, bag_list, _ = FORMS[form]
    tables = PH.start("adagrad", "fp32", 16, batch, bag_list, (300, 3, 5000), "none")      # (no pads: the ids are valid for either entry)
    run = PH.UpdateRunner(hip, tables, "adagrad", "fp32", 16, batch)
    w, s0, s1 = run.fresh()
    u = run.descriptor(w, s0, s1)
    run.pd.sort(u)
    assert run.bs.apply_rc(u) == WS          # a pad sort, the plain apply
    run.bs.sort(u)
    assert run.pd.apply_rc(u) == WS          # a plain sort, the pad apply
    got = run.host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    run.pd.sort(u)                           # ... and the pair, unmixed, runs
    run.pd.apply(u)
    assert run.pd.apply_rc(u) == WS          # once
    PH.assert_same(tables, run.host(w, s0, s1), run.zero_row())


def test_update_argument_checks_leave_the_tables_alone(hip, b16):
    batch, bag_list, _ = FORMS["small"]
    tables = PH.start("adagrad", "fp32", 8, batch, bag_list, (300, 3, 5000), "mask")
    run = PH.UpdateRunner(hip, tables, "adagrad", "fp32", 8, batch)
    w, s0, s1 = run.fresh()
    bf = b16.tables([(run.idx[t], w[t], run.g[t], tb["R"], 8) for t, tb in enumerate(tables)])
    cases = [("AVG", dict(aggr=AVG), UNSUP), ("both table arrays", dict(tables_bf16=bf, rounding=b16.rounding(B.ROUND_NEAREST)), BAD),
             ("neither table array", dict(tables=None), BAD), ("null in_dims", dict(in_dims=None, ntables=3), BAD)]
    for entry in (run.pd.fused_rc, run.pd.apply_rc):
        for what, over, code in cases:
            assert entry(run.descriptor(w, s0, s1, **over)) == code, what
    for what, over, code in cases[1:]:
        assert run.pd.sort_rc(run.descriptor(w, s0, s1, **over)) == code, what
    assert run.pd.fused_rc(None) == BAD
    big = run.descriptor(w, s0, s1)
    big.tables[1].num_entries = 2**32 - 1      # above 2^32 - 2: the pad key would be the reduce kernel's "no key"
    assert run.pd.fused_rc(big) == UNSUP
    got = run.host(w, s0, s1)
    for t, tb in enumerate(tables):
        np.testing.assert_array_equal(got["w"][t], tb["w"])
        np.testing.assert_array_equal(got["s0"][t], tb["s0"])
    run.pd.fused(run.descriptor(w, s0, s1))      # ... and the same descriptor, unmodified, runs
    PH.assert_same(tables, run.host(w, s0, s1), run.zero_row())


# ---- ffh_pad_mask_indices ----------------------------------------------------------------------------------------------------------------
def _mask(pd, n, seed, first, fill):
    torch = torch_()
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    pd.mask(ids, n, seed, first, fill)
    torch.cuda.synchronize()
    return ids.cpu().numpy()


def test_mask_equals_the_numpy_restatement(pd):
    n = 5000
    for seed, first, fill in ((1, 0, 0.5), (2**63 + 5, 0, 0.25), (1, 1234, 0.5), (7, 2**40, 0.9), (7, 0, 0.0)):
        keep = ffmodel.pad_mask_reference(seed, first, n, fill)
        np.testing.assert_array_equal(_mask(pd, n, seed, first, fill), np.where(keep, np.arange(n), PH.PAD), err_msg=str((seed, first, fill)))
    whole = _mask(pd, n, 1, 0, 0.5)      # a continuation: the second part of a stream is the stream's second part
    np.testing.assert_array_equal(_mask(pd, n - 1234, 1, 1234, 0.5) < 0, whole[1234:] < 0)
    assert 0.45 < (whole < 0).mean() < 0.55


def test_mask_past_its_grid_cap(pd):
    """ffh_grid(count, 256) caps at 2048 workgroups: 256 * 2048 + 77 slots take a second trip of the grid-stride loop (4 MB of ids)."""
    n = 256 * 2048 + 77
    got = _mask(pd, n, 11, 3, 0.5)
    np.testing.assert_array_equal(got, np.where(ffmodel.pad_mask_reference(11, 3, n, 0.5), np.arange(n), PH.PAD))
    assert (got[256 * 2048:] < 0).any() and (got[256 * 2048:] >= 0).any()


def test_fill_one_changes_nothing(pd):
    np.testing.assert_array_equal(_mask(pd, 3000, 5, 0, 1.0), np.arange(3000))
    assert pd.mask_rc(None, 0, 5, 0, 0.5) == 0 and pd.mask_rc(None, 5, 5, 0, 0.5) == BAD
