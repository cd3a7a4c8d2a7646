"""One rank of two sharing ONE GPU (launched by tests/test_gpu_adagrad_ranks.py): the golden DLRM under AdagradOptimizer over the host-staged
test transport, the table of 3 rows replicated (data-parallel, in the dense slab), the other three table-wise on their owners."""
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


def main():
    outdir, wd, acc, extra = sys.argv[1], float(sys.argv[2]), float(sys.argv[3]), sys.argv[4:]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    comm = HostStagedComm()
    hp = dict(lr=0.02, weight_decay=wd, epsilon=1e-10, initial_accumulator=acc)
    m, h = A.build_dlrm(capi.HIP_LIB_PATH, H.golden("dlrm_step_torch"), hp, overlap=True, comm=comm.struct,
                        argv=["--device", "0", "--force-exchange", "--replicate-embedding-rows", "3"] + extra)
    out = {}
    for step, rec in enumerate(H.run_steps(m, h, 3)):
        for k, v in rec.items():
            out[f"s{step}/{k}"] = v
    out["allreduce_calls"] = np.array(comm.calls["allreduce"])
    out["alltoall_calls"] = np.array(comm.calls["alltoall"])
    np.savez(os.path.join(outdir, f"rank{dist.get_rank()}.npz"), **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
