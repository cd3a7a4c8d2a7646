"""One rank of two sharing ONE GPU (launched by tests/test_gpu_rowwise_ranks.py): the golden DLRM under AdagradOptimizer(rowwise=True) over the
host-staged test transport, every table table-wise on its owner, --deterministic."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dlrm_flexflow_amd import capi  # noqa: E402
from host_staged_comm import HostStagedComm  # noqa: E402
import adagrad_helpers as A  # noqa: E402
import dlrm_helpers as H  # noqa: E402
import rowwise_helpers as R  # noqa: E402


def main():
    outdir, acc = sys.argv[1], float(sys.argv[2])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    comm = HostStagedComm()
    hp = dict(lr=0.02, weight_decay=0.0, epsilon=1e-10, initial_accumulator=acc, rowwise=True)
    m, h = A.build_dlrm(capi.HIP_LIB_PATH, H.golden("dlrm_step_torch"), hp, overlap=True, comm=comm.struct,
                        argv=["--device", "0", "--force-exchange", "--deterministic"])
    out = {}
    for k, v in H.run_steps(m, h, 3)[-1].items():
        out[k] = v
    for name, S in R.row_states(m, os.path.join(outdir, f"ck{dist.get_rank()}")).items():
        out["S/" + name] = S
    out["alltoall_calls"] = np.array(comm.calls["alltoall"])
    np.savez(os.path.join(outdir, f"rank{dist.get_rank()}.npz"), **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
