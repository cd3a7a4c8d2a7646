"""GPU test (-m gpu): --eval-embedding-dtype int8 over two ranks that share the GPU, tables placed table-wise, the gather writing the exchange
buffers (the pattern of tests/test_gpu_ctr_ranks.py).  The global evaluation equals the one-rank int8 evaluation."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import ctr_helpers as CH

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
INT8 = ["--eval-batches", "1", "--eval-embedding-dtype", "int8"]


def _run_ranks(tmp_path, world, train_steps):
    worker = os.path.join(ROOT, "tests", "_dist_worker_q8.py")
    port = str(29950 + os.getpid() % 40)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(tmp_path), str(train_steps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("train_steps", [0, 2])
def test_two_ranks_report_the_one_rank_int8_evaluation(hip, tmp_path, train_steps):
    """Counts, both histograms and the AUC equal the one-rank run's exactly; the log-loss sum, an fp32 sum taken in another order over two ranks,
    within the 1e-5 relative of tests/test_gpu_ctr_ranks.py.  Every rank quantized its own tables once (one group) and gathered them from the
    images in both eval_batch() calls; the fp32 evaluation of the same model gives other histograms (the flag did something)."""
    z = _run_ranks(tmp_path, 2, train_steps)
    m, h = CH.build_bce_dlrm(HIP, overlap=False, extra_argv=["--deterministic"] + INT8)
    ref = CH.train_then_evaluate(m, train_steps)
    assert m.counter("q8_quantize_launches") == 1 and m.counter("q8_gather_launches") == 2
    m.close()
    m, h = CH.build_bce_dlrm(HIP, overlap=False, extra_argv=["--deterministic"])
    plain = CH.train_then_evaluate(m, train_steps)
    m.close()
    assert float(plain["logloss_sum"]) != float(ref["logloss_sum"])
    B = int(h["g"]["B"])
    assert ref["counts"][0] == 2 * B and ref["counts"][3] == 0
    for r in range(2):
        assert z[r]["q8"].tolist() == [1, 2], z[r]["q8"]
        assert z[r]["counts"].tolist() == ref["counts"].tolist()
        assert np.array_equal(z[r]["hist_pos"], ref["hist_pos"]) and np.array_equal(z[r]["hist_neg"], ref["hist_neg"])
        assert float(z[r]["auc"]) == float(ref["auc"])
        assert abs(float(z[r]["logloss_sum"]) - float(ref["logloss_sum"])) <= 1e-5 * float(ref["logloss_sum"])
