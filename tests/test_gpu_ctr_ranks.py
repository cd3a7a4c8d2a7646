"""GPU test (-m gpu): evaluation metrics over several ranks (include/ff_hip_ctr.h).  Each rank evaluates its slice of the batch;
FFModel.eval_metrics() sums counts and histograms over the ranks exactly (16-bit pieces through the fp32 all-reduce of ffcomm)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import ctr_helpers as CH

pytestmark = pytest.mark.gpu

HIP = capi.HIP_LIB_PATH


def _run_ranks(tmp_path, world, train_steps):
    worker = os.path.join(ROOT, "tests", "_dist_worker_ctr.py")
    port = str(29850 + os.getpid() % 100)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(tmp_path), str(train_steps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("train_steps", [0, 2])
def test_two_ranks_sharing_the_gpu_report_the_one_rank_evaluation(hip, tmp_path, train_steps):
    """Two ranks sharing the GPU (host-staged test transport, as tests/test_gpu_model.py): the global histograms and counts every rank
    reports equal the one-rank run's exactly, the AUC is equal, the log-loss sum within 1e-5 relative; before training and after two
    --deterministic steps."""
    z = _run_ranks(tmp_path, 2, train_steps)
    m, h = CH.build_bce_dlrm(HIP, overlap=False, extra_argv=["--deterministic"])
    ref = CH.train_then_evaluate(m, train_steps)
    pred = m.layer_output(h["final"]).get()
    m.close()
    B = int(h["g"]["B"])
    assert ref["counts"][0] == 2 * B and ref["counts"][3] == 0
    assert 0 < ref["counts"][1] < 2 * B and int(ref["hist_pos"].sum() + ref["hist_neg"].sum()) == 2 * B
    for r in range(2):
        print(f"rank {r}: max |pred - one-rank pred| = {np.abs(z[r]['pred'] - pred[r * B // 2:(r + 1) * B // 2]).max():.3e}")
        assert z[r]["counts"].tolist() == ref["counts"].tolist()
        assert np.array_equal(z[r]["hist_pos"], ref["hist_pos"]) and np.array_equal(z[r]["hist_neg"], ref["hist_neg"])
        assert float(z[r]["auc"]) == float(ref["auc"])
        assert abs(float(z[r]["logloss_sum"]) - float(ref["logloss_sum"])) <= 1e-5 * float(ref["logloss_sum"])
