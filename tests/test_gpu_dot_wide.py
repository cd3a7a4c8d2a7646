"""GPU tests (-m gpu) of the pairwise-dot interaction for up to 128 feature vectors (include/ffh_dot_wide.h, csrc/interaction_wide.hip).

The float64 reference, the input distributions, the sentinel buffers and the derived bound |got - ref| <= (k + 2) 2^-23 mass + k tiny32 are those of
tests/interaction_helpers.py (nothing in them depends on c <= 32), the calls its run_wide_case.  `integer` inputs make every fp32 operation exact:
the result has to equal the reference.  tests/test_gpu_dot_wide_sweep.py is the sweep of every kernel form; these are the shapes of the models.
"""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import interaction_helpers as IH
from interaction_helpers import Case

pytestmark = pytest.mark.gpu

# (batch, c, d); batch None: G + 3 with G the launch's grid size, so that some workgroup takes a second sample
SHAPES = [(3, 33, 128), (2, 64, 128), (2, 65, 36), (1, 97, 130), (2, 128, 128), (5, 40, 4), (7, 31, 128), (None, 33, 8)]
OFFSET = dict(z_off=1, out_off=1, g_off=1, zg_off=1)      # buffers 4 bytes off their 16-byte aligned allocations


@pytest.fixture(scope="module")
def be():
    return IH.TorchBackend()


@pytest.fixture(scope="module")
def wide(hip):
    return capi.dot_wide_api(hip)


def run(wide, be, case, args=None):
    """interaction_helpers.run_wide_case; `args` replaces arguments of the call without changing what is allocated."""
    return IH.run_wide_case(wide, be, case, args)


@pytest.mark.parametrize("dist", ["uniform", "integer"])
@pytest.mark.parametrize("kind,overwrite", [("fwd", False), ("bwd", False), ("bwd", True)])
@pytest.mark.parametrize("batch,c,d,kw", [s + ({},) for s in SHAPES] + [SHAPES[0] + (OFFSET,)])
def test_wide_kernels_match_float64(hip, wide, be, batch, c, d, kw, kind, overwrite, dist):
    """Forward, and backward both ways, against float64 within the derived bound (exactly, for integers); padding sentinels intact, inputs
    unmodified (IH.check), and a second launch gives the same bytes."""
    if batch is None:
        batch = wide.grid(IH.num_cus(hip), 1 << 30, c, backward=kind == "bwd") + 3
    case = Case(f"wide B={batch} c={c} d={d}", kind, batch, c, d, overwrite=overwrite, dist=dist, seed=7 * c + d, **kw)
    assert len({case.ldz, case.ldzg, case.ldo, case.ldg}) == 4
    res = run(wide, be, case)
    rep = IH.check(res)
    print(repr(case), "worst |got - ref| / bound:", rep.worst)
    assert rep.ok(), f"{case!r}\n{rep}"
    again = run(wide, be, case)
    assert again.outputs[0][1].host.tobytes() == res.outputs[0][1].host.tobytes()


# 40 rows in buffers whose strides would hold 129: the row count (or the one named argument) is all that is wrong with a call
WIDE_LD = dict(ldz=129 * 8 + 4, ldzg=129 * 8 + 8, ldo=8 + 129 * 64 + 4, ldg=8 + 129 * 64 + 7)
REFUSAL = Case("refusal", "fwd", 3, 40, 8, **WIDE_LD)


@pytest.mark.parametrize("kind,args", [("fwd", dict(nrows=129)), ("bwd", dict(nrows=129)), ("fwd", dict(nrows=1)), ("bwd", dict(nrows=1)),
                                       ("fwd", dict(ldo=REFUSAL.wo - 1)), ("bwd", dict(flags=2))],
                         ids=["fwd-nrows129", "bwd-nrows129", "fwd-nrows1", "bwd-nrows1", "fwd-ldo-one-short", "bwd-flag-bit-2"])
def test_wide_refusals_touch_nothing(wide, be, kind, args):
    """FFH_ERR_BAD_ARG, and every buffer as it was uploaded (ldo is the forward's argument, the flags are the backward's)."""
    case = Case("refusal", kind, REFUSAL.batch, REFUSAL.c, REFUSAL.d, **WIDE_LD)
    res = run(wide, be, case, args)
    assert res.rc == capi.FFH_ERR_BAD_ARG
    for name, buf in res.buffers():
        assert buf.untouched(), name


def _two_steps(interaction):
    T, D = 40, 16
    C = T + 1
    args = ["--backend", capi.HIP_LIB_PATH, "-b", "64", "--arch-sparse-feature-size", str(D), "--arch-embedding-size", "-".join(["100"] * T),
            "--arch-mlp-bot", "13-32-16", "--arch-mlp-top", f"{D + C * (C - 1) // 2}-64-1", "--arch-interaction-op", interaction, "--data-size", "64"]
    app = ffmodel.DLRM(args)
    m = app.model
    app.warmup()
    app.train_steps(2)
    m.sync()
    top0 = [i for i in range(m.num_layers) if m.layer_name(i).startswith("Dense")][2]      # behind the bottom MLP's two layers
    out = {"pred": m.layer_output(m.num_layers - 1).get(), "top0/w": m.parameter(top0, 0).get_weights(), "launches": m.counter("dot_wide_launches")}
    app.close()
    return out


def test_a_40_table_model_trains_through_the_wide_kernels(hip):
    """41 feature vectors: dot-tril (one launch each way) against dot-tril-ops (the operator chain) from the same seed, two training steps, within
    the tolerance of tests/test_gpu_model.py's dot-tril comparisons (rtol 2e-5, atol 2e-6)."""
    fused, chain = _two_steps("dot-tril"), _two_steps("dot-tril-ops")
    assert fused["launches"] > 0 and chain["launches"] == 0
    for k in ("pred", "top0/w"):
        np.testing.assert_allclose(fused[k], chain[k], rtol=2e-5, atol=2e-6, err_msg=k)
