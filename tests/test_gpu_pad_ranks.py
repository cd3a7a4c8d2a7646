"""GPU test (-m gpu): --embedding-padding over two ranks that share the GPU, tables placed table-wise, ids with pads at fill 0.5 (the pattern of
tests/test_gpu_q8_ranks.py).  Table-wise placement needs nothing new -- ids cross the exchange as they are -- so the two-rank parameters equal the
one-rank run's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import dlrm_helpers as H
import pad_helpers as PH
from _dist_worker_pad import CFG, COUNTERS

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH


def _run_ranks(tmp_path, world):
    worker = os.path.join(ROOT, "tests", "_dist_worker_pad.py")
    port = str(29950 + os.getpid() % 40)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


def test_two_ranks_train_the_one_rank_parameters(hip, tmp_path):
    """Three steps.  The bound: what differs between the runs is the order of fp32 sums (the MLP gradients' all-reduce over two halves of the batch), a
    few 1e-7 relative per step on sums of at most 512 terms -- rtol 1e-5 (the relative bound of tests/test_gpu_q8_ranks.py) with atol 1e-6 for the
    parameters near zero."""
    z = _run_ranks(tmp_path, 2)
    m, h = PH.build_pad_model(HIP, CFG, PH.model_data(CFG, seed=11), extra_argv=["--deterministic"])
    ref = H.run_steps(m, h, steps=3)[-1]
    assert m.counter("pad_gather_launches") > 0 and m.counter("pad_update_launches") > 0
    m.close()
    B, seen = CFG["B"], set()
    for r in range(2):
        assert int(z[r]["pad_gather_launches"]) > 0 and int(z[r]["pad_update_launches"]) > 0, r
        assert int(z[r]["ragged_gather_launches"]) == 0 and int(z[r]["ragged_update_launches"]) == 0, r
        for k in z[r].files:
            if k in COUNTERS:
                continue
            want = ref[k][r * B // 2:(r + 1) * B // 2] if k == "pred" else ref[k]
            np.testing.assert_allclose(z[r][k], want, rtol=1e-5, atol=1e-6, err_msg=f"rank {r}: {k}")
            seen.add(k)
    assert {f"emb.{t}.weight" for t in range(len(CFG["rows"]))} <= seen      # every table on one of the two ranks
    last = f"emb.{len(CFG['rows']) - 1}.weight"                              # its whole batch is pads: no row moved
    np.testing.assert_array_equal(ref[last], h["init"][last])
