"""GPU test (-m gpu): --adagrad-rowwise over two ranks sharing the GPU (host-staged test transport, a fresh child process per rank, arranged as
tests/test_gpu_adagrad_ranks.py arranges its ranks): table-wise tables keep their row state on the owner and take the fused update there; the
result is the one-rank run on the global batch."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import adagrad_helpers as A
import dlrm_helpers as H
import rowwise_helpers as R

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH


def _run_ranks(tmp_path, world, *args):
    worker = os.path.join(ROOT, "tests", "_dist_worker_rowwise.py")
    port = str(29850 + os.getpid() % 90)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(["python", worker, str(tmp_path), *map(str, args)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("acc", [0.0, 0.1])
def test_two_ranks_sharing_the_gpu_equal_one_rank(hip, tmp_path, acc):
    """Golden DLRM, rows (7, 50, 3, 20), every table table-wise (each rank owns two), --deterministic, three steps.  Each table and its row state
    on the rank that holds it, and the predictions, equal the one-rank run.  Not bit for bit: a rank sums the dense gradients of its half of the
    batch and the all-reduce adds the halves, another order than the one-rank sum over the whole batch, so the MLPs and through them the tables
    differ in the last bits from the second step on -- the bound is that of tests/test_gpu_adagrad_ranks.py (rtol 2e-5, atol 2e-6), on the
    tables and on the row states alike."""
    z = _run_ranks(tmp_path, 2, acc)
    g = H.golden("dlrm_step_torch")
    m, h = A.build_dlrm(HIP, g, dict(lr=0.02, weight_decay=0.0, epsilon=1e-10, initial_accumulator=acc, rowwise=True), argv=["--deterministic"])
    ref = H.run_steps(m, h, 3)[-1]
    ref_S = R.row_states(m, tmp_path / "one")
    emb_names = {f"emb.{t}": m.layer_name(h["names"][f"emb.{t}"]) for t in range(len(g["rows"]))}
    m.close()
    B, rows = int(g["B"]), list(g["rows"])
    assert sorted(ref_S) == sorted(emb_names.values()) and all(ref_S[emb_names[f"emb.{t}"]].shape == (rows[t],) for t in range(len(rows)))
    holders = {t: [r for r in range(2) if f"emb.{t}.weight" in z[r].files] for t in range(len(rows))}
    assert all(len(holders[t]) == 1 for t in holders) and {holders[t][0] for t in holders} == {0, 1}, holders
    for r in range(2):
        assert int(z[r]["alltoall_calls"]) >= 3
        np.testing.assert_allclose(z[r]["pred"], ref["pred"][r * B // 2:(r + 1) * B // 2], rtol=2e-5, atol=2e-6, err_msg=f"pred rank {r}")
    for t, (r,) in holders.items():
        name = emb_names[f"emb.{t}"]
        np.testing.assert_allclose(z[r][f"emb.{t}.weight"], ref[f"emb.{t}.weight"], rtol=2e-5, atol=2e-6, err_msg=f"table {t} on rank {r}")
        np.testing.assert_allclose(z[r]["S/" + name], ref_S[name], rtol=2e-5, atol=2e-6, err_msg=f"row state of table {t} on rank {r}")
        assert float(ref_S[name].max()) > acc and not np.array_equal(ref[f"emb.{t}.weight"], g[f"init/emb.{t}.weight"])
