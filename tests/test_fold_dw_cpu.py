"""CPU test of the algebra behind the weight-gradient fold (include/ff_hip_fold.h, ABI 2): at the seeded inputs of the GPU kernel
tests (tests/test_gpu_fold_dw.py), the FOLDED formula restated in float32 numpy -- G_t summed in the canonical 32 / 1024 block order of the fused table
update, then G_t^T E_t with the rows cut into the kernel's chunks -- lies within the project's bound of the UNFOLDED float64 dy^T X_t, the term mass
taken over the full unfolded sum |dy|^T |X_t|.  So an fp32 G alone, whatever the kernels do, fits the bound at these inputs."""
import numpy as np
import pytest

import fold_helpers as FH
import fold_dw_helpers as DH


@pytest.mark.parametrize("kind", DH.KINDS)
@pytest.mark.parametrize("bag", [1, 2])
def test_folded_formula_in_float32_meets_the_bound_of_the_unfolded_sum(bag, kind):
    dy, ids, E = DH.segment_inputs(bag, kind)
    d64 = dy.astype(np.float64)
    for t, rows in enumerate(DH.ROWS):
        G = DH.segment_sum_canonical_f32(ids[t], dy, rows)
        G64, Gmass = DH.segment_sum_f64(ids[t], dy, rows)
        FH.assert_within(G, G64, Gmass, f"G of the {rows}-row table, bag {bag}, ids {kind}")
        hit = np.zeros(rows, bool); hit[ids[t].reshape(-1)] = True
        assert not G[~hit].any()
        x = DH.gathered(E[t], ids[t])                         # [batch][D], float64
        ref, mass = d64.T @ x, np.abs(d64).T @ np.abs(x)      # the unfolded dW block and its term mass
        FH.assert_within(DH.product_f32(G, E[t]), ref, mass, f"G^T E of the {rows}-row table, bag {bag}, ids {kind}")
