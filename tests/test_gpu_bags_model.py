"""GPU tests (-m gpu) of per-table embedding bag sizes in the host model: the driver with --embedding-bag-sizes 1-3-2-7 (4 tables,
D = 16, batch 256, small MLPs) against the same host code on the CPU oracle, the one-launch ragged gather against --no-ragged-gather bit for bit under
--deterministic (eager and replayed, bf16 tables, row-wise Adagrad, the DCNv2 interaction), a shuffled HDF5 file of mixed bags, and the fold counters."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import bags_helpers as BH
import dlrm_helpers as H
import fold_helpers as FH
import shuffle_helpers as SH

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
COUNTERS = ("ragged_gather_launches", "graph_replays", "folded_tables", "folded_dw_tables", "folded_dx_tables", "early_sorts")


@pytest.fixture(scope="module")
def oracle_run():
    """The oracle backend's trajectory of the mixed driver model: computed once."""
    return BH.trajectory(H.oracle_backend(), BH.DRIVER_ARGS, 3, trace=False)


@pytest.mark.parametrize("flags", [[], ["--no-ragged-gather"]], ids=["ragged", "per-bag-size"])
def test_driver_mixed_bags_hip_equals_oracle_backend(hip, oracle_run, flags):
    """1 warm-up + 3 steps, at the bound of test_driver_config1_hip_equals_oracle_backend."""
    for trace in (False, True):
        g = BH.trajectory(HIP, BH.DRIVER_ARGS + flags, 3, trace=trace)
        assert g.keys() == oracle_run.keys()
        for k in g:
            np.testing.assert_allclose(g[k], oracle_run[k], rtol=2e-5, atol=2e-6, err_msg=f"{k} trace={trace}")


def _ragged_equals_split(extra, trace):
    det = ["--deterministic"] + (["--always-replay"] if trace else ["--no-trace"])
    a, ca = BH.trajectory(HIP, BH.DRIVER_ARGS + det + extra, 3, trace=trace, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, BH.DRIVER_ARGS + det + extra + ["--no-ragged-gather"], 3, trace=trace, counters=COUNTERS)
    assert ca["ragged_gather_launches"] > 0 and cb["ragged_gather_launches"] == 0
    if trace:
        assert ca["graph_replays"] >= 2 and cb["graph_replays"] >= 2
    assert ca["early_sorts"] == 0 and cb["early_sorts"] == 0          # mixed bag sizes: the sort stays in front of its apply
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: the ragged gather and the gather per bag size differ ({extra}, trace={trace})"
    return a


@pytest.mark.parametrize("trace", [False, True], ids=["eager", "traced"])
def test_ragged_gather_equals_the_gather_per_bag_size_bit_for_bit(hip, trace):
    _ragged_equals_split([], trace)


@pytest.mark.parametrize("extra", [["--embedding-dtype", "bf16", "--embedding-rounding", "nearest"],
                                   ["--optimizer", "adagrad", "--adagrad-rowwise"],
                                   ["--arch-interaction-op", "dcn", "--dcn-num-layers", "2", "--dcn-low-rank-dim", "8"]],
                         ids=["bf16-tables", "rowwise-adagrad", "dcn"])
def test_ragged_equals_split_with_other_features(hip, extra):
    _ragged_equals_split(extra, trace=False)


def test_shuffled_hdf5_file_of_mixed_bags(hip, tmp_path):
    """--data-randomize total: each loaded batch is the numpy gather of the file's rows by ffmodel.shuffle_indices, table t's ids from its own
    column block of X_cat."""
    rows, bags, B, nb, seed = (50, 7, 300), (2, 1, 5), 16, 4, 5
    n = nb * B
    rng = np.random.default_rng(1)
    data = {"X_int": rng.uniform(0.0, 4.0, (n, 13)).astype(np.float32),
            "X_cat": np.concatenate([rng.integers(0, r, (n, L)) for r, L in zip(rows, bags)], 1).astype(np.int64),
            "y": np.arange(n, dtype=np.float32)}
    path = SH.write_hdf5(str(tmp_path / "mixed.h5"), data)
    app = ffmodel.DLRM(["--backend", HIP] + H.HDF5_ARGS + ["--dataset", path, "--embedding-bag-sizes", "-".join(map(str, bags)), "--seed", str(seed),
                                                            "--lr", "1e-6", "--data-randomize", "total"])
    order = ffmodel.shuffle_indices(seed, 0, n).reshape(nb, B)
    for k in range(nb):
        app.train_steps(1, trace=False)
        app.model.sync()
        idx = app.label_input().get().reshape(-1).astype(np.int64)
        assert np.array_equal(idx, order[k]), (k, idx[:8], order[k][:8])
        assert np.array_equal(app.dense_input().get(), data["X_int"][idx])
        c0 = 0
        for t, L in enumerate(bags):
            assert np.array_equal(app.sparse_input(t).get(np.int64).reshape(B, L), data["X_cat"][idx, c0:c0 + L]), (k, t)
            c0 += L
    assert app.model.counter("ragged_gather_launches") > 0
    app.close()


def test_fold_counters(hip):
    """Mixed bag sizes: no table is folded.  The uniform model of tests/test_gpu_fold_model.py folds as before, given the one size or a list of it."""
    def counters(extra):
        app = ffmodel.DLRM(["--backend", HIP, "--lr", "0.01"] + FH.model_args(extra))
        app.warmup()
        app.train_steps(1, trace=False)
        app.model.sync()
        c = {k: app.model.counter(k) for k in COUNTERS}
        app.close()
        return c
    uniform = counters([])
    listed = counters(["--embedding-bag-sizes", "-".join(["1"] * len(FH.MODEL_ROWS))])
    mixed = counters(["--embedding-bag-sizes", "1-2-1-3-1-1"])
    assert uniform["folded_tables"] == 4 and uniform["ragged_gather_launches"] == 0
    assert listed == uniform
    assert (mixed["folded_tables"], mixed["folded_dw_tables"], mixed["folded_dx_tables"]) == (0, 0, 0)
    assert mixed["ragged_gather_launches"] > 0
