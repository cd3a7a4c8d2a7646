"""GPU tests (-m gpu): the four MFMA kernels of csrc/interaction.hip swept against a float64 reference.

tests/interaction_helpers.py holds the generator, the reference and the checker (tests/test_interaction_sweep_cpu.py proves them on the oracle
library).  Here: the fixed edge table (every branch of the kernels and of the dispatch that the models' own shape does not reach: reused LDS
images, a wave's second and third sample, d == 128 on the VEC == 1 kernels, several 128-column chunks, all strides different), 12 seeds of random
shapes, sample rows beyond 4 GiB, the refusals -- which must not have written anything --, the empty batch, and the same bits from two launches.
"""
import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import interaction_helpers as IH
from interaction_helpers import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def be():
    return IH.TorchBackend()


def _report_worst():
    print("worst |got - ref| / bound so far:", {k: round(v, 4) for k, v in sorted(IH.WORST.items())})


@pytest.mark.parametrize("name", IH.EDGE_NAMES)
def test_interaction_edge_table(hip, be, name):
    cases = IH.edge_table(IH.num_cus(hip))[name]
    assert cases
    for case in cases:
        _, rep = IH.run_and_check(hip, be, case)
        assert rep.ok(), f"{case!r}\n{rep}"
    print(name, "kernels:", sorted({IH.kernel(c) for c in cases}))
    _report_worst()


@pytest.mark.parametrize("seed", range(12))
def test_interaction_random_shapes(hip, be, seed):
    for case in IH.draw_cases(seed, IH.num_cus(hip)):
        _, rep = IH.run_and_check(hip, be, case)
        print(repr(case), "worst:", {k: round(v, 3) for k, v in rep.worst.items()})
        assert rep.ok(), f"{case!r}\n{rep}"
    _report_worst()


# ---------------------------------------------------------------------------------------------------------------------------
# sample rows beyond 4 GiB: the buffers stay on the device, the valid rows are gathered there
BIG_LD, BIG_B = (1 << 20) + 4, 1030             # row 1024 starts 16 KiB past 2^32 bytes


def _big(rows):
    """[BIG_B][BIG_LD] floats of sentinel on the device (and three more behind), `rows` [BIG_B][w] in the leading columns."""
    t = torch.full((BIG_B * BIG_LD + 3,), IH.SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    t[:BIG_B * BIG_LD].view(BIG_B, BIG_LD)[:, :rows.shape[1]] = torch.from_numpy(rows).to(DEV)
    return t


def _gather(t, w):
    return t[:BIG_B * BIG_LD].view(BIG_B, BIG_LD)[:, :w].contiguous().cpu().numpy()


def _not_sentinel(t):
    """One reduction on the device: the words that do not hold the sentinel."""
    return sum(int((piece != IH.SENTINEL_BITS).sum()) for piece in t.view(torch.int32).split(1 << 28))


@pytest.mark.parametrize("dist", ["integer", "uniform"])
def test_interaction_offsets_beyond_4_gib(hip, be, dist):
    """c = 2, d = 128, ldz = ldzg = 2^20 + 4, 1030 samples: the last six sample rows of z and z_grad start beyond 2^32 bytes, where a 32-bit
    byte offset wraps onto the first rows.  Forward, then backward (accumulating on the exact inputs, overwriting on the others)."""
    if torch.cuda.mem_get_info()[0] < 12e9:
        pytest.skip("less than 12 GB of device memory free")
    c, d = 2, 128
    assert (BIG_B - 1) * BIG_LD * 4 > 1 << 32
    fwd = Case("beyond-4-gib fwd", "fwd", BIG_B, c, d, ldz=BIG_LD, dist=dist, seed=4)
    bwd = Case("beyond-4-gib bwd", "bwd", BIG_B, c, d, ldz=BIG_LD, ldzg=BIG_LD, dist=dist, seed=5, overwrite=dist != "integer")
    assert IH.kernel(fwd).startswith("fwd_lds") and IH.kernel(bwd).startswith("bwd_d128")
    try:
        # forward
        inp = IH.make_inputs(fwd)
        zrows = inp["z"].reshape(BIG_B, c * d)
        Z = _big(zrows)
        O = IH.Buf(be, BIG_B, fwd.wo, fwd.ldo, 0)
        rc = hip.lib.ffh_dot_interaction_fwd(hip.ctx, Z.data_ptr(), BIG_LD, O.ptr, fwd.ldo, BIG_B, c, d, None)
        torch.cuda.synchronize()
        assert rc == capi.FFH_OK
        got = O.fetch().get()
        assert O.padding_intact(), "out: padding overwritten"
        assert got[:, :d].tobytes() == zrows[:, :d].tobytes(), "out: the pass-through columns are not z's row 0"
        nbad, where, worst, _, _ = IH.compare_slice(fwd, inp, got[:, d:], 0, BIG_B)
        IH.note_worst(fwd, worst)
        assert not nbad, f"{fwd!r}: {nbad} element(s) off; {where}"
        assert _gather(Z, c * d).tobytes() == zrows.tobytes() and _not_sentinel(Z) == BIG_B * c * d, "z was modified by the forward"
        # backward, on the same allocation of z
        inp = IH.make_inputs(bwd)
        zrows = inp["z"].reshape(BIG_B, c * d)
        Z[:BIG_B * BIG_LD].view(BIG_B, BIG_LD)[:, :c * d] = torch.from_numpy(zrows).to(DEV)
        ZG = _big(inp["old"].reshape(BIG_B, c * d))
        Gr = IH.Buf(be, BIG_B, bwd.wo, bwd.ldg, 0, inp["g"])
        rc = hip.lib.ffh_dot_interaction_bwd(hip.ctx, Z.data_ptr(), BIG_LD, Gr.ptr, bwd.ldg, ZG.data_ptr(), BIG_LD, BIG_B, c, d, bwd.flags, None)
        torch.cuda.synchronize()
        assert rc == capi.FFH_OK
        nbad, where, worst, _, _ = IH.compare_slice(bwd, inp, _gather(ZG, c * d), 0, BIG_B)
        IH.note_worst(bwd, worst)
        assert not nbad, f"{bwd!r}: {nbad} element(s) off; {where}"
        assert _not_sentinel(ZG) == BIG_B * c * d, "z_grad: padding overwritten, or a NaN sentinel stored as a result"
        assert _gather(Z, c * d).tobytes() == zrows.tobytes() and _not_sentinel(Z) == BIG_B * c * d, "z was modified by the backward"
        assert Gr.fetch().untouched(), "out_grad was modified"
    finally:
        Z = ZG = None
        torch.cuda.empty_cache()
    _report_worst()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: the return code, and nothing written.  The buffers are those of a 4 x 8 case with strides wide enough for 33 rows, so that the one
# argument named is the only thing wrong with the call.
def _refusal_case(kind):
    return Case("refusal", kind, 6, 4, 8, ldz=272, ldzg=276, ldo=540, ldg=544, overwrite=True)


REFUSALS = {
    # reason: (kinds, replaced arguments, buffers passed as null)
    "nrows-1": (("fwd", "bwd"), dict(nrows=1), ()),
    "nrows-33": (("fwd", "bwd"), dict(nrows=33), ()),
    "d-0": (("fwd", "bwd"), dict(d=0), ()),
    "batch-negative": (("fwd", "bwd"), dict(batch=-1), ()),
    "ldz-below-c-d": (("fwd", "bwd"), dict(ldz=31), ()),
    "ldzg-below-c-d": (("bwd",), dict(ldzg=31), ()),
    "ldo-below-row": (("fwd",), dict(ldo=13), ()),
    "ldg-below-row": (("bwd",), dict(ldg=13), ()),
    "null-z": (("fwd", "bwd"), {}, ("z",)),
    "null-out": (("fwd",), {}, ("out",)),
    "null-out_grad": (("bwd",), {}, ("out_grad",)),
    "null-z_grad": (("bwd",), {}, ("z_grad",)),
    "unknown-flag-bit": (("bwd",), dict(flags=3), ()),
}


@pytest.mark.parametrize("reason", list(REFUSALS))
def test_interaction_refusals_touch_nothing(hip, be, reason):
    kinds, args, null = REFUSALS[reason]
    for kind in kinds:
        case = _refusal_case(kind)
        served = IH.check(IH.run_case(hip, be, case))
        assert served.ok(), f"the case itself is not served: {served}"
        res = IH.run_case(hip, be, case, args=args, null=null)
        assert res.rc == capi.FFH_ERR_BAD_ARG, (reason, kind, res.rc, hip.lib.ffh_last_error_string(hip.ctx))
        for name, buf in res.buffers():
            assert buf.untouched(), f"{reason}: {name} was written by a refused {kind}"


def test_interaction_empty_batch_writes_nothing(hip, be):
    for kind in ("fwd", "bwd"):
        case = _refusal_case(kind)
        res = IH.run_case(hip, be, case, args=dict(batch=0), null=("z", "out", "out_grad", "z_grad"))
        assert res.rc == capi.FFH_OK, (kind, res.rc)
        res = IH.run_case(hip, be, case, args=dict(batch=0))
        assert res.rc == capi.FFH_OK, (kind, res.rc)
        for name, buf in res.buffers():
            assert buf.untouched(), f"{name} written by an empty {kind}"


def test_interaction_same_bits_twice(hip, be):
    """The kernels use no atomics: two launches of a case leave the same bytes (a race between a wave's samples would not)."""
    table = IH.edge_table(IH.num_cus(hip))
    cases = [c for c in table["lds-third-sample"] + table["grid-stride-9x128-G+7-uniform"] if c.dist == "uniform"]
    assert {c.kind for c in cases} == {"fwd", "bwd"} and len(cases) == 6
    for case in cases:
        inp = IH.make_inputs(case)
        runs = [IH.run_case(hip, be, case, inp=inp) for _ in range(2)]
        assert runs[0].rc == runs[1].rc == capi.FFH_OK
        (name, a), (_, b) = runs[0].outputs[0], runs[1].outputs[0]
        assert a.host.tobytes() == b.host.tobytes(), f"{case!r}: {name} differs between two launches"
        rep = IH.check(runs[1])
        assert rep.ok(), f"{case!r}\n{rep}"
