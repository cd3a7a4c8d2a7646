"""GPU tests (-m gpu) of --embedding-padding in the host model and the driver: the small model of tests/bags_helpers.py with
pads in its id tensors against the float64 model with the pads masked out; the driver with synthetic pads (--synthetic-bag-fill) with and without
--early-sort, fill 1 against the run without the flag, bf16 tables under row-wise Adagrad against the numpy rule; an HDF5 file that holds -1; a
checkpoint across the flag."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import bags_helpers as BH
import bf16_helpers as B16
import dlrm_helpers as H
import pad_helpers as PH
import shuffle_helpers as SH

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
PADDED = ["--embedding-padding", "--synthetic-bag-fill", "0.5"]
COUNTERS = ("pad_gather_launches", "pad_update_launches", "ragged_gather_launches", "ragged_update_launches", "ragged_early_sorts", "early_sorts",
            "folded_tables", "folded_dw_tables", "folded_dx_tables")


# ---- the Python API ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trace", [False, True], ids=["eager", "traced"])
def test_small_model_equals_the_float64_model_with_the_pads_masked_out(hip, trace):
    """Three steps at the bound of tests/test_gpu_bags_model.py.  The ids hold an empty bag, a bag with one pad, and a table whose whole batch is pads."""
    data = PH.model_data(BH.SMALL)
    assert (data["sparse0"][0] < 0).all() and (data["sparse2"] < 0).all() and (data["sparse1"] >= 0).any()
    m, h = PH.build_pad_model(HIP, BH.SMALL, data)
    recs = H.run_steps(m, h, steps=3, trace=trace)
    assert m.counter("pad_gather_launches") > 0 and m.counter("pad_update_launches") > 0
    assert m.counter("ragged_gather_launches") == 0 and m.counter("ragged_update_launches") == 0
    m.close()
    ref = PH.masked_reference(h, 3)
    for step, (g, r) in enumerate(zip(recs, ref)):
        assert g.keys() == r.keys()
        for k in g:
            np.testing.assert_allclose(g[k], r[k], rtol=2e-5, atol=2e-6, err_msg=f"{k} step {step} trace={trace}")
    np.testing.assert_array_equal(recs[-1]["emb.2.weight"], h["init"]["emb.2.weight"])      # only pads touched it
    assert not np.array_equal(recs[-1]["emb.1.weight"], h["init"]["emb.1.weight"])


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
DET = ["--deterministic", "--no-trace"]


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: {what}"


def test_synthetic_pads_with_and_without_the_early_sort(hip):
    a, ca = BH.trajectory(HIP, BH.DRIVER_ARGS + DET + PADDED, 3, trace=False, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, BH.DRIVER_ARGS + DET + PADDED + ["--early-sort"], 3, trace=False, counters=COUNTERS)
    for c in (ca, cb):
        assert c["pad_gather_launches"] > 0 and c["pad_update_launches"] > 0
        assert c["ragged_gather_launches"] == 0 and c["ragged_update_launches"] == 0
        assert (c["folded_tables"], c["folded_dw_tables"], c["folded_dx_tables"]) == (0, 0, 0)
    assert ca["ragged_early_sorts"] == 0 and ca["early_sorts"] == 0
    assert cb["ragged_early_sorts"] > 0 and cb["early_sorts"] == cb["ragged_early_sorts"]
    _same_bits(a, b, "the early pad sort changed the bits")
    plain = BH.trajectory(HIP, BH.DRIVER_ARGS + DET, 3, trace=False)
    assert any(a[k].tobytes() != plain[k].tobytes() for k in a), "the pads changed nothing"


@pytest.mark.parametrize("bags", [BH.DRIVER_BAGS, "3-3-3-3"], ids=["mixed", "one-bag-size"])
def test_the_flag_alone_changes_no_bit(hip, bags):
    """Fill 1: no pad anywhere.  A mixed model moves from the ragged entries to their pad forms; a model of one bag size from the uniform entries to the
    pad forms with equal bag sizes (its small-table fold off in both runs: the flag turns it off)."""
    args = list(BH.DRIVER_ARGS)
    args[args.index("--embedding-bag-sizes") + 1] = bags
    args += DET + ["--no-fold-small-tables"]
    a, ca = BH.trajectory(HIP, args + ["--embedding-padding"], 3, trace=False, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, args, 3, trace=False, counters=COUNTERS)
    assert ca["pad_gather_launches"] > 0 and ca["pad_update_launches"] > 0 and cb["pad_gather_launches"] == 0 and cb["pad_update_launches"] == 0
    assert (cb["ragged_gather_launches"] > 0) == (bags == BH.DRIVER_BAGS)
    _same_bits(a, b, f"--embedding-padding at fill 1 changed the bits (bags {bags})")


def test_bf16_tables_under_rowwise_adagrad_follow_the_numpy_rule_on_the_touched_rows(hip):
    """One step from fresh tables (S = 0) at fill 0.5, rounding to nearest.  A row's gradient is the sum of the output-gradient rows of the samples
    whose bags hold it, a pad holding nothing; the rule is ffmodel.rowwise_adagrad_reference in fp32.  The bound: the device adds a row's gradients
    in the order of its sorted list and numpy in sample order, so the fp32 pre-rounding values agree to a few 1e-7 relative and their bf16 roundings to
    one unit of the bf16 result (2^-8 relative) where a value sits at a rounding boundary.  Rows no lookup touches keep their bits."""
    lr = 0.05
    app = ffmodel.DLRM(["--backend", HIP] + BH.DRIVER_ARGS + DET + PADDED + ["--embedding-dtype", "bf16", "--embedding-rounding", "nearest", "--optimizer", "adagrad",
                                                                           "--adagrad-rowwise", "--lr", str(lr), "--synthetic-labels", "logistic"])      # (logistic labels: a step loads its batch itself)
    m = app.model
    tables = [li for li in range(m.num_layers) if m.layer_num_weights(li) == 1 and m.parameter(li, 0).data_type == ffmodel.DT_BF16]
    assert len(tables) == 4
    before = [m.parameter(li, 0).get_weights() for li in tables]
    app.train_steps(1, trace=False)
    m.sync()
    ids = [app.sparse_input(t).get(np.int64) for t in range(4)]
    assert app.bag_fill == 0.5 and all(0.3 < (i < 0).mean() < 0.7 for i in ids[1:])
    touched = 0
    for t, li in enumerate(tables):
        after = m.parameter(li, 0).get_weights()
        dy = m.layer_output(li).get_grad()
        R, D = before[t].shape
        g = np.zeros((R, D), np.float32)
        i = ids[t].reshape(dy.shape[0], -1)
        for j in range(i.shape[1]):
            live = i[:, j] >= 0
            np.add.at(g, i[live, j], dy[live])
        hit = np.zeros(R, bool)
        hit[i[i >= 0]] = True
        want, _ = ffmodel.rowwise_adagrad_reference(before[t][hit], g[hit], np.zeros(int(hit.sum()), np.float32), lr, 1e-10)
        want = B16.widen(B16.rne(want))
        ulp = np.abs(want) * 2.0 ** -7 + 1e-30      # one unit of a bf16 value is at most 2^-7 of it
        worst = float(np.max(np.abs(after[hit] - want) / ulp))
        print(f"table {t}: {int(hit.sum())} touched rows, worst |got - rule| = {worst:.3f} bf16 units")
        assert worst <= 1.0, (t, worst)
        assert float(np.mean(after[hit] == want)) > 0.9
        np.testing.assert_array_equal(after[~hit], before[t][~hit], err_msg=f"table {t}: an untouched row moved")
        assert not np.array_equal(after[hit], before[t][hit])
        touched += int(hit.sum())
    assert touched > 100
    app.close()


# ---- HDF5 ------------------------------------------------------------------------------------------------------------------------------------
def _file_with_pads(tmp_path):
    rows, bags, B, nb = (50, 7, 300), (2, 1, 5), 16, 4
    n = nb * B
    rng = np.random.default_rng(1)
    cat = np.concatenate([rng.integers(0, r, (n, L)) for r, L in zip(rows, bags)], 1).astype(np.int64)
    cat[rng.random(cat.shape) < 0.4] = PH.PAD
    cat[3, :] = PH.PAD                                             # a sample without any lookup
    data = {"X_int": rng.uniform(0.0, 4.0, (n, 13)).astype(np.float32), "X_cat": cat, "y": np.arange(n, dtype=np.float32)}
    return SH.write_hdf5(str(tmp_path / "pads.h5"), data), data, bags, B, nb


def test_hdf5_file_with_pads_loads_shuffles_and_trains(hip, tmp_path):
    path, data, bags, B, nb = _file_with_pads(tmp_path)
    seed, n = 5, nb * B
    app = ffmodel.DLRM(["--backend", HIP] + H.HDF5_ARGS + ["--dataset", path, "--embedding-bag-sizes", "-".join(map(str, bags)), "--seed", str(seed),
                                                            "--lr", "0.01", "--data-randomize", "total", "--embedding-padding"])
    order = ffmodel.shuffle_indices(seed, 0, n).reshape(nb, B)
    w0 = app.model.parameter(app.model.num_layers - 1, 0).get_weights()
    for k in range(nb):
        app.train_steps(1, trace=False)
        app.model.sync()
        idx = app.label_input().get().reshape(-1).astype(np.int64)
        assert np.array_equal(idx, order[k]), (k, idx[:8], order[k][:8])
        c0 = 0
        for t, L in enumerate(bags):      # the pads arrive where the permutation says
            assert np.array_equal(app.sparse_input(t).get(np.int64).reshape(B, L), data["X_cat"][idx, c0:c0 + L]), (k, t)
            c0 += L
    assert app.model.counter("pad_gather_launches") >= nb and app.model.counter("pad_update_launches") >= nb
    w1 = app.model.parameter(app.model.num_layers - 1, 0).get_weights()
    assert np.isfinite(w1).all() and not np.array_equal(w0, w1)
    app.close()


def test_hdf5_file_with_pads_is_refused_without_the_flag(hip, tmp_path):
    path, _, bags, _, _ = _file_with_pads(tmp_path)
    r = subprocess.run([EXE, "--backend", HIP] + H.HDF5_ARGS + ["--dataset", path, "--embedding-bag-sizes", "-".join(map(str, bags)), "--epochs", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout
    assert "= -1 is outside table" in r.stderr and "--embedding-padding" in r.stderr, r.stderr[-2000:]


def test_other_negative_ids_stay_an_error_with_the_flag(hip, tmp_path):
    rng = np.random.default_rng(2)
    cat = rng.integers(0, 7, (64, 3)).astype(np.int64)
    cat[5, 1] = -2
    path = SH.write_hdf5(str(tmp_path / "bad.h5"), {"X_int": rng.random((64, 13), dtype=np.float32), "X_cat": cat, "y": np.zeros(64, np.float32)})
    r = subprocess.run([EXE, "--backend", HIP] + H.HDF5_ARGS + ["--dataset", path, "--epochs", "1", "--embedding-padding"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "X_cat[5][1] = -2 is outside table 1" in r.stderr, r.stderr[-2000:]


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_saved_without_the_flag_loads_with_it(hip, tmp_path):
    """Tables and states keep their shapes: nothing in a checkpoint knows about the flag."""
    args = ["--backend", HIP] + BH.DRIVER_ARGS + DET + ["--optimizer", "adagrad"]
    a = ffmodel.DLRM(args)
    a.warmup()
    a.train_steps(2, trace=False)
    a.model.save_checkpoint(str(tmp_path), 1)
    digest = a.model.state_digest()
    a.close()
    b = ffmodel.DLRM(args + PADDED)
    assert b.model.load_checkpoint(str(tmp_path)) == {"epochs_done": 1}
    assert b.model.state_digest() == digest
    b.warmup()
    b.model.sync()
    assert b.model.counter("pad_update_launches") > 0 and b.model.state_digest() != digest
    b.close()
