"""The gradient of per-sample bag weights (include/ffh_bag_weights_grad.h) through the C-ABI against ffmodel.bag_weights_grad_reference in float64.
Three tables of bag sizes (1, 3, 100) in one call -- both bag shapes -- read dY from columns [4, 4 + 3 D) of one strided buffer and write into
columns [4, 4 + 104) of another, whose every other element is a guard.  The bound is the header's, derived and not measured: a lane adds at most D
products with fmaf and the butterfly adds at most 6 more times, each rounding 2^-24 relative, so |got - exact| <= (D + 2) * 2^-23 * sum |terms|.
When accumulating, the value that was there is one more term of that sum (one more add)."""
import numpy as np
import pytest
import torch

import bf16_helpers as B
import pad_helpers as PH
from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
BAGS, ROWS, OFF = (1, 3, 100), (300, 3, 5000), (0, 1, 4)
LDG = sum(BAGS) + 8
BAD, UNSUPPORTED = capi.FFH_ERR_BAD_ARG, capi.FFH_ERR_UNSUPPORTED


def dev(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(PH.DEV)


def case(D, batch, bf16):
    rng = np.random.default_rng([PH.SEED, D, batch])
    W = [(rng.standard_normal((r, D)) * 0.1).astype(np.float32) for r in ROWS]
    W = [B.rne(w) for w in W] if bf16 else W
    ids = [PH.apply_pattern(rng.integers(0, r, (batch, L)), "mask", t, len(BAGS)).astype(np.int64) for t, (r, L) in enumerate(zip(ROWS, BAGS))]
    for i in ids[:3 * (batch > 1)]:
        i[1, :] = PH.PAD      # one bag of only pads
    return W, ids, rng.standard_normal((batch, len(BAGS) * D + 8)).astype(np.float32), rng.standard_normal((batch, LDG)).astype(np.float32)


def launch(hip, W, ids, dY, out, D, batch, bf16, accumulate=False, over=()):
    """One call on device copies; `over` replaces single arguments (gw, gw_ld, dims, nt, D, batch, flags).  Returns the status code."""
    nt, ld = len(BAGS), dY.shape[1]
    keep = [dev(w) for w in W], [dev(i) for i in ids], dev(dY)
    ent = [(keep[1][t], keep[0][t], keep[2].data_ptr() + 4 * (4 + t * D), ROWS[t], ld) for t in range(nt)]
    tabs = capi.bf16_api(hip).tables([e + (10 + t, 0) for t, e in enumerate(ent)]) if bf16 else hip.emb_tables(ent)
    a = dict(gw=[out.data_ptr() + 4 * (4 + o) for o in OFF], gw_ld=[LDG] * nt, dims=BAGS, nt=nt, D=D, batch=batch, flags=None)
    a.update(dict(over))
    dims = None if a["dims"] is None else capi.bags_api(hip).in_dims(a["dims"])
    code = capi.bag_weights_grad_api(hip).grad_rc(tabs, a["gw"], a["gw_ld"], dims, a["nt"], a["D"], a["batch"], accumulate=accumulate, bf16=bf16, flags=a["flags"])
    torch.cuda.synchronize()
    return code


# D: one lane, a part group in the 4-byte form, a part group, a full group at the model's width, a looped row.  batch: 1; one bag past what a
# workgroup takes per trip; and, at D = 260 (16 / 8 bags per workgroup and trip), enough to take the grid past its cap
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,batch", [(4, 1025), (6, 161), (16, 1), (16, 257), (128, 33), (260, 17), (260, 12301)])
def test_kernel_equals_the_float64_reference(hip, D, batch, bf16, accumulate):
    if batch > 10000:
        assert 2 * -(-batch // 16) + -(-batch // 8) > capi.bag_weights_grad_api(hip).grid_cap()
    W, ids, dY, g0 = case(D, batch, bf16)
    start = g0 if accumulate else np.full_like(g0, 7.0)
    runs = []
    for _ in range(2):
        out = dev(start)
        assert launch(hip, W, ids, dY, out, D, batch, bf16, accumulate) == 0, hip.lib.ffh_last_error_string(hip.ctx).decode()
        runs.append(out.cpu().numpy())
    got = runs[0]
    assert got.tobytes() == runs[1].tobytes(), "two launches differ"
    want, bound = start.astype(np.float64), np.zeros(start.shape)
    for t, (L, o) in enumerate(zip(BAGS, OFF)):
        Wt, g, cols = (B.widen(W[t]) if bf16 else W[t]).astype(np.float64), dY[:, 4 + t * D:4 + (t + 1) * D], slice(4 + o, 4 + o + L)
        bound[:, cols] = (D + 2) * 2.0 ** -23 * (ffmodel.bag_weights_grad_reference(np.abs(Wt), ids[t], np.abs(g)) + (np.abs(want[:, cols]) if accumulate else 0.0))
        want[:, cols] = ffmodel.bag_weights_grad_reference(Wt, ids[t], g) + (want[:, cols] if accumulate else 0.0)
        assert accumulate or not got[:, cols][ids[t] < 0].view(np.uint32).any(), "a pad is not +0"
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) - bound).max())      # (bound 0 outside the slices: the guard keeps its bits)


def test_bad_arguments_launch_nothing(hip):
    D, batch = 16, 9
    W, ids, dY, g0 = case(D, batch, False)
    out = dev(np.full_like(g0, 7.0))
    ok = [out.data_ptr() + 4 * (4 + o) for o in OFF]
    run = lambda **over: launch(hip, W, ids, dY, out, D, batch, False, over=over)
    for over in [dict(nt=-1), dict(nt=capi.MAX_TABLES + 1), dict(D=0), dict(batch=-1), dict(flags=2), dict(gw=None), dict(gw_ld=None), dict(dims=None),
                 dict(dims=(1, 0, 100)), dict(gw_ld=[LDG, 2, LDG]), dict(gw=[ok[0], None, ok[2]]), dict(gw=[ok[0], ok[1] + 2, ok[2]]), dict(gw=[ok[0], ok[2], ok[2]]), dict(D=64)]:
        assert run(**over) == BAD, over
    assert run(dims=(1, 3, 65536)) == UNSUPPORTED and run(gw_ld=[LDG, 2 ** 31, LDG]) == UNSUPPORTED
    assert run(batch=0) == 0 and run(nt=0) == 0
    wide = 1028                                             # five vectors a lane: past what a lane keeps of dY
    assert launch(hip, [np.zeros((r, wide), np.float32) for r in ROWS], ids, np.zeros((batch, 3 * wide + 8), np.float32), out, wide, batch, False) == UNSUPPORTED
    assert (out.cpu().numpy() == 7.0).all()
