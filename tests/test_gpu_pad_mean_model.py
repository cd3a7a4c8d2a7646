"""GPU tests (-m gpu) of mean pooling under --embedding-padding in the host model and the driver (include/ff_hip_pad_mean.h): the small model of
tests/bags_helpers.py built with AGGR_MODE_AVG and pads in its id tensors against a float64 model with the mean over the lookups that are
there; the driver's --embedding-pooling mean with synthetic pads, with and without --early-sort, fill 1 against the run without padding;
eval_batch()."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import bags_helpers as BH
import dlrm_helpers as H
import pad_helpers as PH
import pad_mean_helpers as PM

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
DET = ["--deterministic", "--no-trace"]
MEAN = ["--embedding-pooling", "mean"]
PADDED = ["--embedding-padding", "--synthetic-bag-fill", "0.5"]
COUNTERS = ("pad_mean_gather_launches", "pad_mean_update_launches", "pad_gather_launches", "pad_update_launches", "ragged_gather_launches",
            "ragged_update_launches", "ragged_early_sorts", "early_sorts")


# ---- the Python API ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trace", [False, True], ids=["eager", "traced"])
def test_small_model_equals_the_float64_model_with_the_mean_over_the_present_lookups(hip, trace):
    """Three steps at the bound of tests/test_gpu_pad_model.py.  The ids hold an empty bag, a bag with one pad, and a table whose whole batch is pads."""
    data = PH.model_data(BH.SMALL)
    assert (data["sparse0"][0] < 0).all() and (data["sparse2"] < 0).all() and (data["sparse1"] >= 0).any()
    m, h = PM.build_pad_mean_model(HIP, BH.SMALL, data)
    recs = H.run_steps(m, h, steps=3, trace=trace)
    assert m.counter("pad_mean_gather_launches") > 0 and m.counter("pad_mean_update_launches") > 0
    assert m.counter("pad_gather_launches") == 0 and m.counter("pad_update_launches") == 0
    assert m.counter("ragged_gather_launches") == 0 and m.counter("ragged_update_launches") == 0
    m.close()
    ref = PM.mean_reference(h, 3)
    for step, (g, r) in enumerate(zip(recs, ref)):
        assert g.keys() == r.keys()
        for k in g:
            np.testing.assert_allclose(g[k], r[k], rtol=2e-5, atol=2e-6, err_msg=f"{k} step {step} trace={trace}")
    np.testing.assert_array_equal(recs[-1]["emb.2.weight"], h["init"]["emb.2.weight"])      # only pads touched it
    assert not np.array_equal(recs[-1]["emb.1.weight"], h["init"]["emb.1.weight"])
    # the mean is not the sum: the float64 model with the pads masked out and a SUM lies outside the bound
    summed = PH.masked_reference(h, 1)[0]
    assert not np.allclose(recs[0]["emb.1.weight"], summed["emb.1.weight"], rtol=2e-5, atol=2e-6)


def test_eval_batch_runs_the_mean_gather(hip):
    data = PH.model_data(BH.SMALL)
    m, h = PM.build_pad_mean_model(HIP, BH.SMALL, data)
    H.run_steps(m, h, steps=1)
    before = m.counter("pad_mean_gather_launches")
    updates = m.counter("pad_mean_update_launches")
    m.eval_batch()
    m.sync()
    assert m.counter("pad_mean_gather_launches") > before and m.counter("pad_mean_update_launches") == updates
    assert m.counter("pad_gather_launches") == 0
    assert m.eval_metrics()["samples"] == BH.SMALL["B"]
    m.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: {what}"


@pytest.mark.parametrize("bags", [BH.DRIVER_BAGS, "3-3-3-3"], ids=["mixed", "one-bag-size"])
def test_padding_at_fill_one_changes_no_bit_of_the_mean(hip, bags):
    """Fill 1: no pad anywhere, every count is L_t.  The run moves from the existing AVG paths to the mean forms of the pad entries (the small-table
    fold off in both runs: --embedding-padding turns it off)."""
    args = list(BH.DRIVER_ARGS)
    args[args.index("--embedding-bag-sizes") + 1] = bags
    args += DET + ["--no-fold-small-tables"] + MEAN
    a, ca = BH.trajectory(HIP, args + ["--embedding-padding"], 3, trace=False, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, args, 3, trace=False, counters=COUNTERS)
    assert ca["pad_mean_gather_launches"] > 0 and ca["pad_mean_update_launches"] > 0 and ca["pad_gather_launches"] == 0 and ca["pad_update_launches"] == 0
    assert cb["pad_mean_gather_launches"] == 0 and cb["pad_mean_update_launches"] == 0
    _same_bits(a, b, f"--embedding-padding at fill 1 changed the bits of the mean (bags {bags})")
    plain = BH.trajectory(HIP, args[:-2], 3, trace=False)
    assert any(a[k].tobytes() != plain[k].tobytes() for k in a), "--embedding-pooling mean changed nothing"


def test_synthetic_pads_with_and_without_the_early_sort_and_against_the_sum(hip):
    a, ca = BH.trajectory(HIP, BH.DRIVER_ARGS + DET + PADDED + MEAN, 3, trace=False, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, BH.DRIVER_ARGS + DET + PADDED + MEAN + ["--early-sort"], 3, trace=False, counters=COUNTERS)
    for c in (ca, cb):
        assert c["pad_mean_gather_launches"] > 0 and c["pad_mean_update_launches"] > 0
        assert c["pad_gather_launches"] == 0 and c["pad_update_launches"] == 0
        assert c["ragged_gather_launches"] == 0 and c["ragged_update_launches"] == 0
    assert ca["ragged_early_sorts"] == 0 and ca["early_sorts"] == 0
    assert cb["ragged_early_sorts"] > 0 and cb["early_sorts"] == cb["ragged_early_sorts"]
    _same_bits(a, b, "the early pad sort changed the bits of the mean update")
    summed = BH.trajectory(HIP, BH.DRIVER_ARGS + DET + PADDED, 3, trace=False)
    assert any(a[k].tobytes() != summed[k].tobytes() for k in a), "mean pooling over the pads equals sum pooling"


def test_the_application_object_reports_the_pooling(hip):
    app = ffmodel.DLRM(["--backend", HIP] + BH.DRIVER_ARGS + PADDED + ["--embedding-pooling=mean"])
    assert app.embedding_pooling == "mean" and app.bag_fill == 0.5
    app.close()
