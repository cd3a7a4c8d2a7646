"""The gather with a bag size per table (include/ff_hip_bags.h) on the GPU, library level, all bit for bit: the ragged call against
(i) ffh_embedding_fwd per table -- the existing kernel -- and (ii) a numpy float32 sum in ascending j from +0.

Shapes are the smallest that reach every branch: D = 16 (several rows per wave), 128, 260 (65 vectors of 4 floats: more than the 64 lanes of a
row, a second trip per lane) and 3 (the scalar form); batches 1, 37 and 1000, none a multiple of the rows per workgroup (8 .. 256); bag lists
that are short only, long only (>= 4 ids: the form that keeps several ids of a row in flight, with a tail that is no multiple of 4), the heavy
table first, in the middle and last, the 26 MLPerf sizes, and FFH_MAX_TABLES tables.  Tables are small, so ids repeat heavily."""
import numpy as np
import pytest

import bf16_helpers as B16
from bags_helpers import MLPERF_BAGS
from dlrm_flexflow_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUM, AVG = capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG
assert 260 // 4 > 64      # D = 260: more vectors than lanes in a wave

BAG_LISTS = {"one": [1], "hundred": [100], "heavy-middle": [1, 100, 1], "heavy-first": [100, 1, 1, 7], "heavy-last": [7, 1, 1, 100],
             "mlperf": MLPERF_BAGS, "max-tables": [1, 5] * 32}
assert len(BAG_LISTS["max-tables"]) == capi.MAX_TABLES and len(MLPERF_BAGS) == 26


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def bags(hip):
    return capi.bags_api(hip)


@pytest.fixture(scope="module")
def b16(hip):
    return capi.bf16_api(hip)


def _rows(t):
    return 23 + 17 * t      # small tables: heavy repeats


def _case(seed, D, bag_list, batch, bf16=False):
    """Host side of a case: per table the fp32 weights (bf16 tables: the widened values, exactly representable) and the ids."""
    rng = np.random.default_rng(seed)
    W, ids = [], []
    for t, L in enumerate(bag_list):
        w = rng.standard_normal((_rows(t), D)).astype(np.float32)
        w[0, :] = -0.0                                              # (+0) + (-0) = +0: a bag of row 0 alone must give +0
        if bf16:
            w = (B16.rne(w).astype(np.uint32) << 16).view(np.float32)
        i = rng.integers(0, _rows(t), (batch, L)).astype(np.int64)
        i[0, :] = i[0, 0]                                           # a bag that repeats one row
        if batch > 2:
            i[2, :] = 0
        W.append(w); ids.append(i)
    return W, ids


def _numpy_sum(w, i, aggr):
    acc = np.zeros((i.shape[0], w.shape[1]), np.float32)            # +0
    for j in range(i.shape[1]):                                     # ascending j, one float32 add each
        acc = acc + w[i[:, j]]
    return acc * np.float32(np.float32(1.0) / np.float32(i.shape[1])) if aggr == AVG else acc


def _layout(nt, D, col0, tail):
    """Columns of a Concat-like destination: `col0` columns of something else, the tables side by side, `tail` more columns."""
    return [col0 + t * D for t in range(nt)], col0 + nt * D + tail


def _run(hip, bags, b16, W, ids, bag_list, D, batch, aggr, col0, tail, bf16):
    """Returns (ragged output, per-table ffh_embedding_fwd output): two [batch][ld] buffers, 7.0 where nothing may be written."""
    torch = torch_()
    nt = len(bag_list)
    offs, ld = _layout(nt, D, col0, tail)
    out = torch.full((batch, ld), 7.0, device=DEV)
    ref = torch.full((batch, ld), 7.0, device=DEV)
    wd = [torch.from_numpy(w).to(DEV) for w in W]
    w16 = [torch.from_numpy(B16.rne(w).view(np.int16)).to(DEV) for w in W] if bf16 else None
    idd = [torch.from_numpy(i).to(DEV) for i in ids]
    dims = bags.in_dims(bag_list)
    if bf16:
        arr = b16.tables([(idd[t], w16[t], out.data_ptr() + 4 * offs[t], _rows(t), ld) for t in range(nt)])
        bags.call("ffh_embedding_fwd_multi_bags_bf16", arr, dims, nt, D, batch, aggr)
    else:
        arr = hip.emb_tables([(idd[t], wd[t], out.data_ptr() + 4 * offs[t], _rows(t), ld) for t in range(nt)])
        bags.call("ffh_embedding_fwd_multi_bags", arr, dims, nt, D, batch, aggr)
    for t in range(nt):                                             # (i): the existing kernel, one table at a time, on the (widened) fp32 table
        hip.call("ffh_embedding_fwd", idd[t], ref.data_ptr() + 4 * offs[t], wd[t], bag_list[t], D, batch, _rows(t), ld, aggr, None)
    torch.cuda.synchronize()
    return out, ref, offs


def _check(hip, bags, b16, seed, D, bag_list, batch, aggr, col0=0, tail=0, bf16=False):
    torch = torch_()
    W, ids = _case(seed, D, bag_list, batch, bf16)
    out, ref, offs = _run(hip, bags, b16, W, ids, bag_list, D, batch, aggr, col0, tail, bf16)
    what = (D, batch, aggr, col0, tail, bf16)
    assert out.view(torch.int32).equal(ref.view(torch.int32)), what                 # (i), and 7.0 wherever no table writes
    got = out.cpu().numpy()
    for t, off in enumerate(offs):                                                   # (ii)
        np.testing.assert_array_equal(got[:, off:off + D].view(np.uint32), _numpy_sum(W[t], ids[t], aggr).view(np.uint32), err_msg=f"{what} table {t}")
    assert np.all(got[:, :col0] == 7.0) and np.all(got[:, offs[-1] + D:] == 7.0)
    if batch > 2:
        assert np.all(got[2, offs[0]:offs[0] + D].view(np.uint32) == 0)              # bags of the -0 row: +0


@pytest.mark.parametrize("name", list(BAG_LISTS))
@pytest.mark.parametrize("D", [16, 128, 260, 3])
def test_ragged_gather_equals_the_per_table_gather_and_numpy(hip, bags, b16, D, name):
    """SUM and AVG at batches 1, 37 and 1000, the destination a column slice of a wider buffer (the tables side by side behind 4 other columns,
    as under a Concat; D = 3: behind 5)."""
    bag_list = BAG_LISTS[name]
    for k, (batch, aggr) in enumerate(((1, SUM), (37, AVG), (1000, SUM), (37, SUM), (1000, AVG))):
        _check(hip, bags, b16, 100 * D + k, D, bag_list, batch, aggr, col0=4 if D % 4 == 0 else 5, tail=4)


@pytest.mark.parametrize("name", ["heavy-middle", "mlperf"])
@pytest.mark.parametrize("D", [16, 128, 3])
def test_ragged_gather_from_bf16_tables(hip, bags, b16, D, name):
    """The _bf16 entry: the same comparison on the widened table."""
    for k, (batch, aggr) in enumerate(((37, SUM), (1000, AVG))):
        _check(hip, bags, b16, 7 * D + k, D, BAG_LISTS[name], batch, aggr, col0=4 if D % 4 == 0 else 5, tail=4, bf16=True)


@pytest.mark.parametrize("D,col0", [(16, 0), (128, 0), (16, 3), (128, 1)])
def test_contiguous_and_misaligned_destinations(hip, bags, b16, D, col0):
    """ld == the tables' columns exactly (col0 = 0, no tail), and a destination that is not 16-byte aligned (the scalar form at D % 4 == 0)."""
    for batch, aggr in ((37, SUM), (1000, AVG)):
        _check(hip, bags, b16, D + col0, D, BAG_LISTS["heavy-first"], batch, aggr, col0=col0, tail=0)
        _check(hip, bags, b16, D + col0, D, BAG_LISTS["heavy-first"], batch, aggr, col0=col0, tail=0, bf16=True)


@pytest.mark.parametrize("L", [1, 3, 4, 7, 100])
@pytest.mark.parametrize("bf16", [False, True])
def test_equal_bag_sizes_give_the_bits_of_the_uniform_call(hip, bags, b16, L, bf16):
    torch = torch_()
    D, batch, nt = 128, 1000, 5
    W, ids = _case(L, D, [L] * nt, batch, bf16)
    for aggr in (SUM, AVG):
        out, _, offs = _run(hip, bags, b16, W, ids, [L] * nt, D, batch, aggr, 0, 0, bf16)
        ld = nt * D
        uni = torch.full((batch, ld), 7.0, device=DEV)
        idd = [torch.from_numpy(i).to(DEV) for i in ids]
        if bf16:
            w16 = [torch.from_numpy(B16.rne(w).view(np.int16)).to(DEV) for w in W]
            arr = b16.tables([(idd[t], w16[t], uni.data_ptr() + 4 * offs[t], _rows(t), ld) for t in range(nt)])
            b16.call("ffh_embedding_fwd_multi_bf16", arr, nt, L, D, batch, aggr, None)
        else:
            wd = [torch.from_numpy(w).to(DEV) for w in W]
            arr = hip.emb_tables([(idd[t], wd[t], uni.data_ptr() + 4 * offs[t], _rows(t), ld) for t in range(nt)])
            hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, arr, nt, L, D, batch, aggr, None), "fwd_multi")
        torch.cuda.synchronize()
        assert out.view(torch.int32).equal(uni.view(torch.int32)), (L, bf16, aggr)


@pytest.mark.parametrize("math_mode", [1, 2], ids=["tensor-op-twin", "split-three-plane"])
def test_twin_and_three_plane_image_of_the_destination(hip, bags, math_mode):
    """With a registered bf16 twin (tensor-op mode) or three-plane image (split mode) of the destination, the ragged gather leaves in it what the
    uniform kernel writes for the same tables taken one bag size at a time.  D = 16, ld = 64 (a multiple of 32), batch 37."""
    torch = torch_()
    D, batch, bag_list = 16, 37, [100, 1, 1, 7]
    nt, ld = len(bag_list), 64
    W, ids = _case(math_mode, D, bag_list, batch)
    wd = [torch.from_numpy(w).to(DEV) for w in W]
    idd = [torch.from_numpy(i).to(DEV) for i in ids]
    reg = hip.lib.ffh_ctx_bf16_mirror_set if math_mode == 1 else hip.lib.ffh_ctx_bf16x3_mirror_set
    side_n = batch * ld if math_mode == 1 else batch * ld // 32 * 96
    out = torch.zeros((batch, ld), device=DEV)
    side = [torch.full((side_n,), 0x1111, dtype=torch.int16, device=DEV) for _ in range(2)]
    tabs = lambda sel: hip.emb_tables([(idd[t], wd[t], out.data_ptr() + 4 * D * t, _rows(t), ld) for t in sel])
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, math_mode) == 0
    try:
        try:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[0].data_ptr()) == 0
            bags.call("ffh_embedding_fwd_multi_bags", tabs(range(nt)), bags.in_dims(bag_list), nt, D, batch, SUM)
            torch.cuda.synchronize()
            got = out.clone()
            out.zero_()
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, side[1].data_ptr()) == 0        # the same base: replaced
            for L in sorted(set(bag_list)):                                                        # the uniform kernel: the reference here
                sel = [t for t in range(nt) if bag_list[t] == L]
                hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, tabs(sel), len(sel), L, D, batch, SUM, None), "fwd_multi")
            torch.cuda.synchronize()
        finally:
            assert reg(hip.ctx, out.data_ptr(), batch * ld * 4, None) == 0
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
    assert got.view(torch.int32).equal(out.view(torch.int32))
    assert torch.equal(side[0], side[1]), f"{int((side[0] != side[1]).sum())} of {side_n} mirror words differ"
    assert int((side[1] != 0x1111).sum()) > side_n // 2                                            # the uniform kernel did write it


def test_argument_checks_launch_nothing(hip, bags, b16):
    torch = torch_()
    D, batch = 16, 37
    W, ids = _case(1, D, [2, 3], batch)
    wd = [torch.from_numpy(w).to(DEV) for w in W]
    idd = [torch.from_numpy(i).to(DEV) for i in ids]
    out = torch.full((batch, 2 * D), 7.0, device=DEV)
    entry = lambda t: (idd[t % 2], wd[t % 2], out.data_ptr() + 4 * D * (t % 2), _rows(t % 2), 2 * D)
    arr = hip.emb_tables([entry(0), entry(1)])
    arr16 = b16.tables([entry(0), entry(1)])
    BAD, UNS = capi.FFH_ERR_BAD_ARG, capi.FFH_ERR_UNSUPPORTED
    for name, a in (("ffh_embedding_fwd_multi_bags", arr), ("ffh_embedding_fwd_multi_bags_bf16", arr16)):
        assert bags.rc(name, a, bags.in_dims([2, 0]), 2, D, batch, SUM) == BAD
        assert bags.rc(name, a, bags.in_dims([-1, 3]), 2, D, batch, SUM) == BAD
        assert bags.rc(name, a, bags.in_dims([2, capi.BAGS_MAX_IN_DIM + 1]), 2, D, batch, SUM) == UNS
        assert bags.rc(name, a, None, 2, D, batch, SUM) == BAD
        assert bags.rc(name, a, bags.in_dims([2, 3]), 2, D, batch, 99) == BAD
    many = capi.MAX_TABLES + 1
    assert bags.rc("ffh_embedding_fwd_multi_bags", hip.emb_tables([entry(t) for t in range(many)]), bags.in_dims([1] * many), many, D, batch, SUM) == BAD
    assert bags.rc("ffh_embedding_fwd_multi_bags_bf16", b16.tables([entry(t) for t in range(many)]), bags.in_dims([1] * many), many, D, batch, SUM) == BAD
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert bags.rc("ffh_embedding_fwd_multi_bags", arr, bags.in_dims([2, 3]), 0, D, batch, SUM) == 0       # no tables, no batch: nothing to do
    assert bags.rc("ffh_embedding_fwd_multi_bags", arr, bags.in_dims([2, 3]), 2, D, 0, SUM) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
