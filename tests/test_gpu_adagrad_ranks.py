"""GPU test (-m gpu): --optimizer adagrad over two ranks sharing the GPU (host-staged test transport, a fresh child process per rank, as
tests/test_gpu_ctr_ranks.py): table-wise tables keep their accumulator on the owner and take the fused update there, a replicated table lives in
the dense slab under ffh_adagrad_update with an all-reduced gradient; the result is the one-rank run on the global batch."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import adagrad_helpers as A
import dlrm_helpers as H

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH


def _run_ranks(tmp_path, world, *args):
    worker = os.path.join(ROOT, "tests", "_dist_worker_adagrad.py")
    port = str(29750 + os.getpid() % 90)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(tmp_path), *map(str, args)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("wd,acc,extra", [(0.0, 0.0, ()), (1e-3, 0.1, ())], ids=["fused_tables", "wd_dense_tables"])
def test_two_ranks_sharing_the_gpu_equal_one_rank(hip, tmp_path, wd, acc, extra):
    """Golden DLRM, rows (7, 50, 3, 20): the 3-row table replicated, the others table-wise (rank 0 owns two, rank 1 one).  Three steps; predictions,
    the top MLP and every table a rank holds equal the one-rank run within the bound of the any-optimizer ranks test (rtol 2e-5, atol 2e-6).  Without
    weight decay the owners run the fused update, with it the owner-local dense path."""
    z = _run_ranks(tmp_path, 2, wd, acc, *extra)
    g = H.golden("dlrm_step_torch")
    m, h = A.build_dlrm(HIP, g, dict(lr=0.02, weight_decay=wd, epsilon=1e-10, initial_accumulator=acc))
    ref = H.run_steps(m, h, 3)
    m.close()
    B, rows = int(g["B"]), list(g["rows"])
    holders = {t: [r for r in range(2) if f"s2/emb.{t}.weight" in z[r].files] for t in range(len(rows))}
    assert holders[2] == [0, 1] and all(len(holders[t]) == 1 for t in (0, 1, 3)), holders          # replicated / table-wise
    assert {holders[t][0] for t in (0, 1, 3)} == {0, 1}                                                # each rank owns a table
    for r in range(2):
        assert int(z[r]["allreduce_calls"]) >= 3 and int(z[r]["alltoall_calls"]) >= 3
        sl = slice(r * B // 2, (r + 1) * B // 2)
        for step in range(3):
            np.testing.assert_allclose(z[r][f"s{step}/pred"], ref[step]["pred"][sl], rtol=2e-5, atol=2e-6, err_msg=f"pred rank {r} step {step}")
            for k in ref[step]:
                if k != "pred" and f"s{step}/{k}" in z[r].files:
                    np.testing.assert_allclose(z[r][f"s{step}/{k}"], ref[step][k], rtol=2e-5, atol=2e-6, err_msg=f"{k} rank {r} step {step}")
    assert not np.array_equal(ref[2]["emb.2.weight"], g["init/emb.2.weight"])
