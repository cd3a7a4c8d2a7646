"""GPU tests (-m gpu) of the ragged table update in the host model: the driver model of tests/test_gpu_bags_model.py (4 tables of
bag sizes 1, 3, 2, 7; D = 16) with --ragged-update against --no-ragged-update, bit for bit under --deterministic.  Batch 256 is the small form
(the largest table has 1,792 entries); batch 512 the sorted form (bag 7: 3,584 entries).  Both flags are always given explicitly."""
import os

import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import bags_helpers as BH
import checkpoint_helpers as K
import dlrm_helpers as H

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
COUNTERS = ("ragged_update_launches", "ragged_gather_launches", "graph_replays", "early_sorts")
SMALL = list(BH.DRIVER_ARGS)
SORTED = [{"256": "512"}.get(a, a) for a in BH.DRIVER_ARGS]      # -b 512 --data-size 512
assert SORTED[SORTED.index("-b") + 1] == "512" and SORTED[SORTED.index("--data-size") + 1] == "512"
SHAPES = {"small": SMALL, "sorted": SORTED}


def _ragged_equals_split(args, extra, trace):
    det = ["--deterministic"] + (["--always-replay"] if trace else ["--no-trace"])
    a, ca = BH.trajectory(HIP, args + det + extra + ["--ragged-update"], 3, trace=trace, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, args + det + extra + ["--no-ragged-update"], 3, trace=trace, counters=COUNTERS)
    assert ca["ragged_update_launches"] > 0 and cb["ragged_update_launches"] == 0, (ca, cb)
    if trace:
        assert ca["graph_replays"] >= 2 and cb["graph_replays"] >= 2
    assert ca["early_sorts"] == 0 and cb["early_sorts"] == 0          # mixed bag sizes: the sort stays in front of its apply
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: the ragged update and the update per bag size differ ({extra}, trace={trace})"
    return a


@pytest.mark.parametrize("trace", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_update_equals_the_update_per_bag_size_bit_for_bit(hip, shape, trace):
    _ragged_equals_split(SHAPES[shape], [], trace)


@pytest.mark.parametrize("extra", [["--embedding-dtype", "bf16", "--embedding-rounding", "stochastic"],
                                   ["--optimizer", "adagrad", "--adagrad-rowwise"],
                                   ["--optimizer", "adam", "--sparse-embedding-optimizer", "--device-lr", "--lr-num-warmup-steps", "3"]],
                         ids=["bf16-stochastic", "rowwise-adagrad", "adam-device-lr-warmup"])
def test_ragged_equals_split_with_other_features(hip, extra):
    _ragged_equals_split(SORTED, extra, trace=False)


# 34 bf16 tables under Adam: the stateful bf16 entries take 32 tables a call, so the group is cut into tables 0 .. 31 (bag sizes 2, 1, 3 in rotation: the
# ragged call) and tables 32, 33 (both bag size 3: the uniform call, whose bag size is its own tables', not the group's first)
CUT_BAGS = [(2, 1, 3)[t % 3] for t in range(32)] + [3, 3]
CUT = ["-b", "256", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "-".join(str(40 + 7 * t) for t in range(34)), "--arch-mlp-bot", "13-32-8",
       "--arch-mlp-top", f"{8 + 34 * 8}-32-1", "--data-size", "256", "--embedding-bag-sizes", "-".join(map(str, CUT_BAGS)),
       "--embedding-dtype", "bf16", "--optimizer", "adam", "--sparse-embedding-optimizer"]


def test_a_cut_group_whose_last_call_has_one_bag_size(hip):
    assert CUT_BAGS[0] != CUT_BAGS[32] == CUT_BAGS[33]
    _ragged_equals_split(CUT, [], trace=False)
    on = K.run_driver(None, *CUT, "--epochs", "1", "--ragged-update", exe=os.path.join(K.ROOT, "dlrm_flexflow_amd", "host", "dlrm"))
    assert "[DLRM] embedding update: ragged, 2 calls per step (1 of them over one bag size)" in on.stdout, on.stdout


def test_the_later_flag_wins(hip):
    for flags, ran in ((["--ragged-update", "--no-ragged-update"], False), (["--no-ragged-update", "--ragged-update"], True)):
        _, c = BH.trajectory(HIP, SMALL + ["--no-trace"] + flags, 1, trace=False, counters=COUNTERS)
        assert (c["ragged_update_launches"] > 0) == ran, (flags, c)


@pytest.mark.parametrize("flag", ["--ragged-update", "--no-ragged-update"])
def test_a_uniform_model_makes_no_ragged_call(hip, flag):
    args = [a for a in SMALL if a not in ("--embedding-bag-sizes", BH.DRIVER_BAGS)] + ["--embedding-bag-size", "3", "--no-trace", flag]
    _, c = BH.trajectory(HIP, args, 1, trace=False, counters=COUNTERS)
    assert c["ragged_update_launches"] == 0 and c["ragged_gather_launches"] == 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_update_on_hip_equals_the_oracle_backend(hip, shape):
    """1 warm-up + 3 steps, at the bound of tests/test_gpu_bags_model.py for this model."""
    ref = BH.trajectory(H.oracle_backend(), SHAPES[shape], 3, trace=False)
    g, c = BH.trajectory(HIP, SHAPES[shape] + ["--ragged-update"], 3, trace=False, counters=COUNTERS)
    assert c["ragged_update_launches"] > 0 and g.keys() == ref.keys()
    for k in g:
        np.testing.assert_allclose(g[k], ref[k], rtol=2e-5, atol=2e-6, err_msg=k)


def test_driver_says_how_it_updates(hip):
    on = K.run_driver(None, *SMALL, "--epochs", "1", "--ragged-update", exe=os.path.join(K.ROOT, "dlrm_flexflow_amd", "host", "dlrm"))
    off = K.run_driver(None, *SMALL, "--epochs", "1", "--no-ragged-update", exe=os.path.join(K.ROOT, "dlrm_flexflow_amd", "host", "dlrm"))
    assert "[DLRM] embedding update: ragged, 1 call per step" in on.stdout, on.stdout
    assert "[DLRM] embedding update: per bag size, 4 calls per step (--no-ragged-update)" in off.stdout, off.stdout
    for r in (on, off):
        assert "[DLRM] embedding gather: ragged, one launch per group (1 launch)" in r.stdout


def test_checkpoint_resume_with_the_ragged_update(hip, tmp_path):
    """Save after 1 epoch (2 steps) with the ragged update, load in a new process, continue to 2 epochs: the straight run's bits."""
    flags = list(SORTED)
    flags[flags.index("--data-size") + 1] = "1024"      # batch 512: 2 batches an epoch
    flags += ["--deterministic", "--ragged-update", "--optimizer", "adagrad", "--adagrad-rowwise"]
    (ra, rb, rc), (a, b, c) = K.abc(None, tmp_path, flags, epochs=2, split=1)
    assert "[DLRM] embedding update: ragged" in rc.stdout and f"[DLRM] checkpoint: loaded {b}" in rc.stdout
    K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))
