"""8-bit embedding rows (include/ff_hip_q8.h) on the GPU, library level, all bit for bit.

The quantizer against ffmodel.q8_quantize_reference over whole allocations (32 sentinel bytes before and behind every image); the gathers
against (i) ffh_embedding_fwd per table -- the existing kernel -- on the dequantized fp32 table and (ii) a numpy float32 sum in ascending j
from +0.  Shapes are those of tests/test_gpu_bags.py: D = 16 (several rows per wave), 128, 260 (65 dwords of codes: more than a wave's
lanes, a second trip per lane) and, for the quantizer, 4 (one lane per row, a dword of codes per lane) and 1040 (65 chunks of 16 elements: a
second turn of the form that stores 16 bytes of codes per lane, which D = 16 and 128 take in one turn); batches and row counts 1, 37 and 1000."""
import numpy as np
import pytest

import bf16_helpers as B16
import q8_helpers as Q
from bags_helpers import MLPERF_BAGS
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUM, AVG = capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG
SENT, GUARD = 0xAB, 32
assert 260 // 4 > 64      # D = 260: more dwords of codes than lanes in a wave

BAG_LISTS = {"one": [1], "hundred": [100], "heavy-middle": [1, 100, 1], "heavy-first": [100, 1, 1, 7], "heavy-last": [7, 1, 1, 100],
             "mlperf": MLPERF_BAGS, "max-tables": [1, 5] * 32}
assert len(BAG_LISTS["max-tables"]) == capi.MAX_TABLES and len(MLPERF_BAGS) == 26


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def q8(hip):
    return capi.q8_api(hip)


@pytest.fixture(scope="module")
def bags(hip):
    return capi.bags_api(hip)


# ---- the quantizer ---------------------------------------------------------------------------------------------------------------------
def _quantize(q8, tables, D, bf16, padded):
    """Quantizes `tables` (float32 arrays holding what the source holds) in ONE call; returns per table (whole allocation, expected)."""
    torch = torch_()
    rb = Q.row_bytes_for(D, padded)
    src, bufs, keep = [], [], []
    for w in tables:
        n = w.shape[0]
        wd = torch.from_numpy(B16.rne(w).view(np.int16) if bf16 else w).to(DEV)
        buf = torch.full((GUARD + n * rb + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        assert (buf.data_ptr() + GUARD) % 4 == 0
        src.append((wd, buf.data_ptr() + GUARD, n, rb, int(bf16)))
        bufs.append(buf); keep.append(wd)
    q8.quantize(q8.sources(src), len(tables), D)
    torch.cuda.synchronize()
    out = []
    for w, buf in zip(tables, bufs):
        want = np.full(buf.numel(), SENT, np.uint8)
        want[GUARD:-GUARD] = Q.pack(w, rb).reshape(-1)
        out.append((buf.cpu().numpy(), want))
    return out


@pytest.mark.parametrize("padded", [False, True], ids=["D+8", "16-byte-rows"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [4, 16, 128, 260, 1040])
def test_quantizer_equals_the_numpy_rule_over_whole_allocations(q8, D, bf16, padded):
    """Tables of 1, 37 and 1000 rows in one call; the special rows of q8_helpers lead the two larger ones."""
    rng = np.random.default_rng(1000 * D + 2 * bf16 + padded)
    tables = [Q.make_table(rng, n, D, bf16, special=n > 1) for n in (1, 37, 1000)]
    if not padded:
        assert q8.row_bytes(D) == D + 8 == Q.row_bytes_for(D, False)
    for k, (got, want) in enumerate(_quantize(q8, tables, D, bf16, padded)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"D {D} bf16 {bf16} padded {padded} table {k}: {bad.size} bytes differ, first at {bad[:4] - GUARD} (row_bytes {Q.row_bytes_for(D, padded)})"
    codes, scale, bias = ffmodel.q8_quantize_reference(tables[1][:2])
    assert not codes.any() and bias[0].view(np.uint32) == 0                                  # the -0 row: codes 0, bias +0
    assert np.array_equal(ffmodel.q8_dequantize_reference(codes, scale, bias)[1], tables[1][1])     # the constant row is exact


@pytest.mark.parametrize("trips_per_workgroup", [1, 2, 3])
def test_quantizer_past_its_grid_cap(q8, trips_per_workgroup):
    """D = 4: a workgroup takes 256 rows of one table per trip.  Two tables whose trips together are exactly the grid cap (every workgroup
    one full trip), the cap and three more (three workgroups take a second trip), twice the cap and three more (three or more)."""
    D = 4
    cap, rpt = q8.quantize_max_workgroups(), q8.quantize_rows_per_trip(D)
    assert rpt == 256
    extra = 0 if trips_per_workgroup == 1 else 3
    total = (trips_per_workgroup - 1) * cap + (cap if trips_per_workgroup == 1 else extra)
    first = 5                                                 # trips of the first table, the last of them partial
    rows = [first * rpt - 7, (total - first) * rpt - (0 if trips_per_workgroup == 1 else 100)]
    trips = sum(-(-n // rpt) for n in rows)
    assert trips == total and -(-trips // min(trips, cap)) == trips_per_workgroup          # the most trips any workgroup makes
    if trips_per_workgroup == 1:
        assert trips == cap and rows[1] % rpt == 0                                           # the last workgroup's one trip is a full one
    rng = np.random.default_rng(trips_per_workgroup)
    tables = [Q.make_table(rng, n, D) for n in rows]
    for k, (got, want) in enumerate(_quantize(q8, tables, D, False, False)):
        assert np.array_equal(got, want), f"table {k} of {rows} rows"


# ---- the gathers -----------------------------------------------------------------------------------------------------------------------
def _rows(t):
    return 23 + 17 * t      # small tables: heavy repeats


def _case(seed, D, bag_list, batch):
    """Host side of a case: per table the fp32 weights (special rows first, row 0 all -0), its dequantized image and the ids."""
    rng = np.random.default_rng(seed)
    W, ids = [], []
    for t, L in enumerate(bag_list):
        w = Q.make_table(rng, _rows(t), D)
        i = rng.integers(0, _rows(t), (batch, L)).astype(np.int64)
        i[0, :] = i[0, 0]                                           # a bag that repeats one row
        if batch > 2:
            i[2, :] = 0                                             # bags of the -0 row: (+0) + (+0)
        W.append(w); ids.append(i)
    return W, ids


def _numpy_sum(w, i, aggr):
    acc = np.zeros((i.shape[0], w.shape[1]), np.float32)            # +0
    with np.errstate(all="ignore"):
        for j in range(i.shape[1]):                                 # ascending j, one float32 add each
            acc = acc + w[i[:, j]]
        return acc * np.float32(np.float32(1.0) / np.float32(i.shape[1])) if aggr == AVG else acc


def _device_case(hip, W, ids, D):
    """Per table: the packed rows (row_bytes D + 8 on even tables, rounded up to 16 on odd ones), the dequantized fp32 table, the ids."""
    torch = torch_()
    rbs = [Q.row_bytes_for(D, t % 2 == 1) for t in range(len(W))]
    rows = [torch.from_numpy(Q.pack(w, rb)).to(DEV) for w, rb in zip(W, rbs)]
    deq = [Q.dequantized(w) for w in W]
    wd = [torch.from_numpy(w).to(DEV) for w in deq]
    idd = [torch.from_numpy(i).to(DEV) for i in ids]
    return rbs, rows, deq, wd, idd


def _check(hip, q8, bags, seed, D, bag_list, batch, aggr, col0=4, tail=4, uniform=False):
    """The q8 gather (ragged entry, or the uniform entry with all bags equal) into a column slice of a wider buffer filled with 7.0."""
    torch = torch_()
    nt = len(bag_list)
    W, ids = _case(seed, D, bag_list, batch)
    rbs, rows, deq, wd, idd = _device_case(hip, W, ids, D)
    offs, ld = [col0 + t * D for t in range(nt)], col0 + nt * D + tail
    out = torch.full((batch, ld), 7.0, device=DEV)
    ref = torch.full((batch, ld), 7.0, device=DEV)
    arr = q8.tables([(idd[t], rows[t], out.data_ptr() + 4 * offs[t], _rows(t), ld, rbs[t]) for t in range(nt)])
    if uniform:
        assert len(set(bag_list)) == 1
        q8.fwd(arr, nt, bag_list[0], D, batch, aggr)
    else:
        q8.fwd_bags(arr, bags.in_dims(bag_list), nt, D, batch, aggr)
    for t in range(nt):                                             # (i): the existing kernel, one table at a time, on the dequantized table
        hip.call("ffh_embedding_fwd", idd[t], ref.data_ptr() + 4 * offs[t], wd[t], bag_list[t], D, batch, _rows(t), ld, aggr, None)
    torch.cuda.synchronize()
    what = (D, batch, aggr, col0, tail, uniform)
    assert out.view(torch.int32).equal(ref.view(torch.int32)), what                 # (i), and 7.0 wherever no table writes
    got = out.cpu().numpy()
    for t, off in enumerate(offs):                                                   # (ii)
        np.testing.assert_array_equal(got[:, off:off + D].view(np.uint32), _numpy_sum(deq[t], ids[t], aggr).view(np.uint32), err_msg=f"{what} table {t}")
    assert np.all(got[:, :col0] == 7.0) and np.all(got[:, offs[-1] + D:] == 7.0)
    if batch > 2:
        assert np.all(got[2, offs[0]:offs[0] + D].view(np.uint32) == 0)              # bags of the -0 row: +0


@pytest.mark.parametrize("name", list(BAG_LISTS))
@pytest.mark.parametrize("D", [16, 128, 260])
def test_ragged_gather_equals_the_fp32_gather_on_the_dequantized_table(hip, q8, bags, D, name):
    """SUM and AVG at batches 1, 37 and 1000; the tables side by side behind 4 other columns, as under a Concat.  "max-tables" at batch
    1000 is past the grid cap: its tables' row blocks (D = 128: 32 tables x 32 + 32 x 63) exceed the 2048 workgroups."""
    bag_list = BAG_LISTS[name]
    if name == "max-tables" and D == 128:
        assert 32 * -(-1000 // 32) + 32 * -(-1000 // 16) > 2048
    for k, (batch, aggr) in enumerate(((1, SUM), (37, AVG), (1000, SUM), (37, SUM), (1000, AVG))):
        _check(hip, q8, bags, 100 * D + k, D, bag_list, batch, aggr)


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("D", [16, 128, 260])
def test_uniform_gather_equals_the_fp32_gather_on_the_dequantized_table(hip, q8, bags, D, L):
    for k, (batch, aggr) in enumerate(((1, SUM), (37, AVG), (1000, SUM), (1000, AVG))):
        _check(hip, q8, bags, 10 * D + L + k, D, [L] * 5, batch, aggr, uniform=True)


def test_uniform_gather_past_its_grid_cap(hip, q8, bags):
    """64 tables share 1024 workgroups: 16 each, of 32 rows at D = 128 -- a batch of 1000 is beyond that share of 512 rows."""
    D, batch, nt = 128, 1000, capi.MAX_TABLES
    assert -(-batch // 32) > 1024 // nt
    for aggr in (SUM, AVG):
        _check(hip, q8, bags, 5, D, [3] * nt, batch, aggr, uniform=True)


@pytest.mark.parametrize("col0,tail", [(0, 0), (8, 0)])
def test_contiguous_destinations(hip, q8, bags, col0, tail):
    for D in (16, 128):
        _check(hip, q8, bags, D + col0, D, BAG_LISTS["heavy-first"], 37, SUM, col0=col0, tail=tail)
        _check(hip, q8, bags, D + col0, D, [3, 3], 1000, AVG, col0=col0, tail=tail, uniform=True)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("math_mode", [1, 2], ids=["tensor-op-twin", "split-three-plane"])
def test_twin_and_three_plane_image_of_the_destination(hip, q8, bags, math_mode, ragged):
    """With a registered bf16 twin (tensor-op mode) or three-plane image (split mode) of the destination, the q8 gather leaves in it the
    bits the fp32 gather leaves from the dequantized table.  D = 16, ld = 64 (a multiple of 32), batch 37."""
    torch = torch_()
    D, batch = 16, 37
    bag_list = [100, 1, 1, 7] if ragged else [3, 3, 3, 3]
    nt, ld = len(bag_list), 64
    W, ids = _case(math_mode, D, bag_list, batch)
    rbs, rows, deq, wd, idd = _device_case(hip, W, ids, D)
    reg = hip.lib.ffh_ctx_bf16_mirror_set if math_mode == 1 else hip.lib.ffh_ctx_bf16x3_mirror_set
    side_n = batch * ld if math_mode == 1 else batch * ld // 32 * 96
    out = torch.zeros((batch, ld), device=DEV)
    side = [torch.full((side_n,), 0x1111, dtype=torch.int16, device=DEV) for _ in range(2)]
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, math_mode) == 0
    try:
        try:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[0].data_ptr()) == 0
            arr = q8.tables([(idd[t], rows[t], out.data_ptr() + 4 * D * t, _rows(t), ld, rbs[t]) for t in range(nt)])
            if ragged:
                q8.fwd_bags(arr, bags.in_dims(bag_list), nt, D, batch, SUM)
            else:
                q8.fwd(arr, nt, bag_list[0], D, batch, SUM)
            torch.cuda.synchronize()
            got = out.clone()
            out.zero_()
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[1].data_ptr()) == 0        # the same base: replaced
            for L in sorted(set(bag_list)):                                                        # the fp32 gather: the reference here
                sel = [t for t in range(nt) if bag_list[t] == L]
                tabs = hip.emb_tables([(idd[t], wd[t], out.data_ptr() + 4 * D * t, _rows(t), ld) for t in sel])
                hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, tabs, len(sel), L, D, batch, SUM, None), "fwd_multi")
            torch.cuda.synchronize()
        finally:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, None) == 0
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
    assert got.view(torch.int32).equal(out.view(torch.int32))
    assert torch.equal(side[0], side[1]), f"{int((side[0] != side[1]).sum())} of {side_n} mirror words differ"
    assert int((side[1] != 0x1111).sum()) > side_n // 2                                            # the fp32 gather did write it


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing(hip, q8, bags):
    torch = torch_()
    D, batch = 16, 37
    rb = D + 8
    W, ids = _case(1, D, [2, 3], batch)
    rbs, rows, deq, wd, idd = _device_case(hip, W, ids, D)
    rows = [torch.from_numpy(Q.pack(w, rb)).to(DEV) for w in W]
    out = torch.full((batch, 2 * D + 4), 7.0, device=DEV)
    ld = 2 * D + 4
    BAD, UNS = capi.FFH_ERR_BAD_ARG, capi.FFH_ERR_UNSUPPORTED

    def entry(t, **kw):
        e = dict(idx=idd[t % 2], rows=rows[t % 2], io=out.data_ptr() + 4 * D * (t % 2), n=_rows(t % 2), ld=ld, rb=rb)
        e.update(kw)
        return (e["idx"], e["rows"], e["io"], e["n"], e["ld"], e["rb"])

    def both(tabs, nt=2, dims=(2, 3), D_=D, aggr=SUM):
        """(uniform rc, ragged rc) of one table list"""
        return (q8.fwd_rc(tabs, nt, 2, D_, batch, aggr), q8.fwd_bags_rc(tabs, bags.in_dims(dims), nt, D_, batch, aggr))

    good = q8.tables([entry(0), entry(1)])
    for field in ("idx", "rows", "io"):
        assert both(q8.tables([entry(0), entry(1, **{field: None})])) == (BAD, BAD), field
    assert q8.fwd_rc(None, 2, 2, D, batch, SUM) == BAD and q8.fwd_bags_rc(None, bags.in_dims([2, 3]), 2, D, batch, SUM) == BAD
    many = capi.MAX_TABLES + 1
    assert both(q8.tables([entry(t) for t in range(many)]), nt=many, dims=[1] * many) == (BAD, BAD)
    assert both(good, aggr=99) == (BAD, BAD)
    assert both(q8.tables([entry(0), entry(1, rb=D + 4)])) == (BAD, BAD)                    # row_bytes < out_dim + 8
    assert both(q8.tables([entry(0), entry(1, rb=D + 10)])) == (BAD, BAD)                   # row_bytes % 4 != 0
    assert q8.fwd_rc(good, 2, 0, D, batch, SUM) == BAD
    assert q8.fwd_bags_rc(good, bags.in_dims([2, 0]), 2, D, batch, SUM) == BAD
    assert q8.fwd_bags_rc(good, bags.in_dims([-1, 3]), 2, D, batch, SUM) == BAD
    assert q8.fwd_bags_rc(good, None, 2, D, batch, SUM) == BAD
    assert q8.fwd_bags_rc(good, bags.in_dims([2, capi.BAGS_MAX_IN_DIM + 1]), 2, D, batch, SUM) == UNS
    # where the 16-byte output form does not apply: there is no scalar form
    assert both(q8.tables([entry(0, rb=D + 12), entry(1, rb=D + 12)]), D_=D + 2) == (UNS, UNS)            # out_dim % 4 != 0 (row_bytes valid for it)
    assert both(q8.tables([entry(0), entry(1, io=out.data_ptr() + 4 * D + 4)])) == (UNS, UNS)               # io not 16-byte aligned
    assert both(q8.tables([entry(0, ld=ld + 1), entry(1, ld=ld + 1)])) == (UNS, UNS)                        # ld % 4 != 0
    assert both(q8.tables([entry(0), entry(1, rows=rows[1].data_ptr() + 2)])) == (UNS, UNS)                 # rows not 4-byte aligned
    # the quantizer
    img = torch.full((_rows(0) * rb,), SENT, dtype=torch.uint8, device=DEV)
    w0 = torch.from_numpy(W[0]).to(DEV)
    src = lambda **kw: q8.sources([tuple({**dict(w=w0, rows=img, n=_rows(0), rb=rb, bf16=0), **kw}.values())])
    assert q8.quantize_rc(src(w=None), 1, D) == BAD and q8.quantize_rc(src(rows=None), 1, D) == BAD
    assert q8.quantize_rc(None, 1, D) == BAD
    assert q8.quantize_rc(src(), capi.MAX_TABLES + 1, D) == BAD
    assert q8.quantize_rc(src(rb=D + 4), 1, D) == BAD and q8.quantize_rc(src(rb=D + 10), 1, D) == BAD
    assert q8.quantize_rc(src(rb=D + 12), 1, D + 2) == UNS
    assert q8.quantize_rc(src(rows=img.data_ptr() + 2), 1, D) == UNS
    assert q8.quantize_rc(src(w=w0.data_ptr() + 4), 1, D) == UNS
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == SENT).all())
    assert both(good, nt=0) == (0, 0)                                                          # no tables: nothing to do
    assert q8.fwd_bags_rc(good, bags.in_dims([2, 3]), 2, D, 0, SUM) == 0 and q8.fwd_rc(good, 2, 2, D, 0, SUM) == 0
    assert q8.quantize_rc(src(), 0, D) == 0 and q8.quantize_rc(src(n=0), 1, D) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == SENT).all())
