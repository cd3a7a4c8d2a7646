"""GPU tests (-m gpu) of the early sort of a model of mixed bag sizes (include/ff_hip_bags_sort.h): the driver model of
tests/bags_helpers.py (4 tables of bag sizes 1, 3, 2, 7; D = 16) with --ragged-update --early-sort against --ragged-update --no-early-sort, bit for
bit under --deterministic.  Batch 256 is the small route (every table has at most 1,792 entries: the sort call is empty, the apply kernel sorts);
batch 512 the sorted route (bag 7: 3,584 entries).  The flags are always given explicitly."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import bags_helpers as BH
import checkpoint_helpers as K
import test_gpu_bags_update_model as M

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
COUNTERS = ("ragged_early_sorts", "early_sorts", "ragged_update_launches", "graph_replays")
SMALL, SORTED, SHAPES = M.SMALL, M.SORTED, M.SHAPES


def _early_equals_front(args, extra, trace, steps=3):
    det = ["--deterministic", "--ragged-update"] + (["--always-replay"] if trace else ["--no-trace"])
    a, ca = BH.trajectory(HIP, args + det + extra + ["--early-sort"], steps, trace=trace, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, args + det + extra + ["--no-early-sort"], steps, trace=trace, counters=COUNTERS)
    assert ca["ragged_early_sorts"] > 0 and ca["early_sorts"] > 0, ca
    assert cb["ragged_early_sorts"] == 0 and cb["early_sorts"] == 0, cb
    assert ca["ragged_update_launches"] > 0 and cb["ragged_update_launches"] > 0, (ca, cb)
    if trace:
        assert ca["graph_replays"] >= 2 and cb["graph_replays"] >= 2, (ca, cb)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: the sort behind the gather and the sort in front of the apply differ ({extra}, trace={trace})"
    return a


@pytest.mark.parametrize("trace", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_early_sort_equals_the_sort_in_front_bit_for_bit(hip, shape, trace):
    _early_equals_front(SHAPES[shape], [], trace)


@pytest.mark.parametrize("extra", [["--embedding-dtype", "bf16", "--embedding-rounding", "stochastic"],
                                   ["--optimizer", "adagrad", "--adagrad-rowwise"],
                                   ["--optimizer", "adam", "--sparse-embedding-optimizer", "--device-lr", "--lr-num-warmup-steps", "3"],
                                   ["--fp32-split-bf16x3"]],
                         ids=["bf16-stochastic", "rowwise-adagrad", "adam-device-lr-warmup", "split-mode"])
def test_early_sort_with_other_features(hip, extra):
    _early_equals_front(SORTED, extra, trace=False)


# ---- where the sort stays in front --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,extra", [(SORTED, ["--ragged-update", "--early-sort", "--no-ragged-update"]),
                                        (M.CUT, ["--ragged-update", "--early-sort"]),
                                        (SORTED, ["--ragged-update", "--early-sort", "--no-overlap"])],
                         ids=["no-ragged-update", "cut-group-of-34-tables", "no-overlap"])
def test_the_sort_stays_in_front(hip, args, extra):
    """--early-sort is a wish: without the ragged update, with a group that is cut into two calls (one note per ctx) and without the side stream
    the model trains as it does without the flag."""
    a, ca = BH.trajectory(HIP, args + ["--deterministic", "--no-trace"] + extra, 2, trace=False, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, args + ["--deterministic", "--no-trace"] + [f for f in extra if f != "--early-sort"] + ["--no-early-sort"], 2, trace=False, counters=COUNTERS)
    assert ca["ragged_early_sorts"] == 0 and cb["ragged_early_sorts"] == 0, (ca, cb)
    assert ca["ragged_update_launches"] == cb["ragged_update_launches"]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
        assert np.isfinite(a[k]).all(), k
    init = BH.trajectory(HIP, args + ["--deterministic", "--no-trace"] + extra, 0, trace=False)
    assert any(a[k].tobytes() != init[k].tobytes() for k in a if k != "pred"), "the model did not train"


def test_a_uniform_model_keeps_the_uniform_sort_calls(hip):
    args = [a for a in SORTED if a not in ("--embedding-bag-sizes", BH.DRIVER_BAGS)] + ["--embedding-bag-size", "3", "--no-trace", "--ragged-update"]
    _, on = BH.trajectory(HIP, args + ["--early-sort"], 2, trace=False, counters=COUNTERS)
    _, off = BH.trajectory(HIP, args + ["--no-early-sort"], 2, trace=False, counters=COUNTERS)
    assert on["early_sorts"] > 0 and on["ragged_early_sorts"] == 0 and on["ragged_update_launches"] == 0, on
    assert off["early_sorts"] == 0 and off["ragged_early_sorts"] == 0, off


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_says_where_it_sorts(hip):
    on = K.run_driver(None, *SORTED, "--epochs", "1", "--ragged-update", "--early-sort", exe=EXE)
    off = K.run_driver(None, *SORTED, "--epochs", "1", "--ragged-update", exe=EXE)
    no = K.run_driver(None, *SORTED, "--epochs", "1", "--ragged-update", "--no-early-sort", exe=EXE)
    split = K.run_driver(None, *SORTED, "--epochs", "1", "--no-ragged-update", "--early-sort", exe=EXE)
    assert "[DLRM] embedding update: ragged, 1 call per step, sorted behind the gather\n" in on.stdout, on.stdout
    for r in (off, no):
        assert "[DLRM] embedding update: ragged, 1 call per step\n" in r.stdout, r.stdout
    assert "[DLRM] embedding update: per bag size, 4 calls per step (--no-ragged-update)\n" in split.stdout, split.stdout
    assert "sorted behind the gather" not in off.stdout + no.stdout + split.stdout


def test_run_dlrm_passes_the_flag_through(hip):
    r = subprocess.run(["python", os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py"), *SORTED, "--epochs", "1", "--ragged-update", "--early-sort"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "[DLRM] embedding update: ragged, 1 call per step, sorted behind the gather\n" in r.stdout, r.stdout


def test_checkpoint_resume_with_the_early_sort(hip, tmp_path):
    """Save after 1 epoch (2 steps) with the early sort, load in a new process, continue to 2 epochs: the straight run's bits."""
    flags = list(SORTED)
    flags[flags.index("--data-size") + 1] = "1024"      # batch 512: 2 batches an epoch
    flags += ["--deterministic", "--ragged-update", "--early-sort", "--optimizer", "adagrad", "--adagrad-rowwise"]
    (ra, rb, rc), (a, b, c) = K.abc(None, tmp_path, flags, epochs=2, split=1)
    for r in (ra, rb, rc):
        assert "[DLRM] embedding update: ragged, 1 call per step, sorted behind the gather" in r.stdout, r.stdout
    assert f"[DLRM] checkpoint: loaded {b}" in rc.stdout
    K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))


# ---- the exchange path: two ranks sharing the GPU -----------------------------------------------------------------------------------------
def _run_ranks(tmp_path, flag):
    worker = os.path.join(ROOT, "tests", "_dist_worker_bags_sort.py")
    out = tmp_path / flag.strip("-")
    out.mkdir()
    port = str(29950 + os.getpid() % 40 + (0 if flag == "--early-sort" else 45))
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(out), flag], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(out, f"rank{r}.npz")) for r in range(2)]


def test_two_ranks_on_the_exchange_path(hip, tmp_path):
    """Mixed bags, table-wise, each rank owning two tables of differing bag sizes: --early-sort against --no-early-sort under --deterministic,
    every rank's parameters byte for byte, and the ragged sort ran on each rank."""
    on, off = _run_ranks(tmp_path, "--early-sort"), _run_ranks(tmp_path, "--no-early-sort")
    for r in range(2):
        assert int(on[r]["ragged_early_sorts"]) > 0 and int(on[r]["early_sorts"]) > 0, r
        assert int(off[r]["ragged_early_sorts"]) == 0 and int(off[r]["early_sorts"]) == 0, r
        assert int(on[r]["ragged_update_launches"]) > 0 and int(off[r]["ragged_update_launches"]) > 0, r
        assert sorted(on[r].files) == sorted(off[r].files) and sum(k.startswith("emb.") for k in on[r].files) == 2
        for k in on[r].files:
            if k not in COUNTERS:
                assert on[r][k].tobytes() == off[r][k].tobytes(), f"rank {r}: {k}"
        assert any(on[r][k].tobytes() != on[r]["init/" + k].tobytes() for k in on[r].files if k.startswith("emb."))
