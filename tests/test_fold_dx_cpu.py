"""CPU statement of the data-gradient half of the fold (include/ff_hip_fold.h, ABI 3): the update of a folded table is
E_t[r] = fmaf(-lr, G_t[r] W[:, cols_t], E_t[r]) with G_t the segmented sum of dy in the canonical order -- restated in float32 numpy in the orders the
header documents and held against the unfolded formula E_t[r] - lr sum_hits dy[b] W[:, cols_t] in float64, at 1e-5 lr (term mass of the unfolded sum over
hits and o) + 2 ulp(w).  Tables of 1, 3, 63 and 1543 rows, batch 4096, out 256, D 128, bags of 1 and 2.  No GPU, no library: what the kernels must
compute, and that the bound the GPU tests hold them to is met by the documented orders."""
import numpy as np
import pytest

import fold_dx_helpers as XH

OUT = XH.OUTS[0]


@pytest.mark.parametrize("bag", [1, 2])
def test_folded_update_meets_the_bound_of_the_unfolded_sum(bag):
    dy, w, ids, E = XH.inputs(bag, OUT)
    G = XH.canonical_G(bag, OUT)
    refs = XH.references(bag, OUT)
    for t, r in enumerate(XH.ROWS):
        got = XH.update_f32(G[t], XH.w_block(w, t), E[t], XH.LR)
        ref, mass = refs[t]
        XH.assert_update_within(got, ref, mass, E[t], XH.LR, f"folded update, {r} rows, bag {bag}")
        assert np.abs(got.astype(np.float64) - E[t]).max() > 0, "nothing moved"


@pytest.mark.parametrize("bag", [1, 2])
def test_a_row_nobody_hit_keeps_its_bits(bag):
    dy, w, ids, E = XH.inputs(bag, OUT)
    G = XH.canonical_G(bag, OUT)
    seen = 0
    for t, r in enumerate(XH.ROWS):
        un = XH.unhit(t, bag, OUT)
        if not un.any():
            continue
        seen += int(un.sum())
        assert not G[t][un].any(), "G of a row nobody hit is not exactly 0"
        Et = E[t].copy()
        Et[un, 0] = -0.0      # a signed zero survives fmaf(-lr, 0, -0.0) as well
        got = XH.update_f32(G[t], XH.w_block(w, t), Et, XH.LR)
        assert got[un].tobytes() == Et[un].tobytes(), f"{r} rows: a row nobody hit changed"
        assert got[~un].tobytes() != Et[~un].tobytes()
    assert seen >= 2


def test_model_batch_rule():
    """The model test's batch on a 256-CU device: 123 row tiles -- 984 tiles fill four rounds of 256 to 96 % (40 idle tiles: less than one k-tile per
    workgroup), the 615 kept tiles fill three rounds to 80.08 %; one row tile fewer and the kept tiles fall below 80 %."""
    assert XH.model_batch(256) == 15744
