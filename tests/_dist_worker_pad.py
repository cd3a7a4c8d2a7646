"""One rank of two sharing ONE GPU (launched by tests/test_gpu_pad_ranks.py): the padded DLRM of tests/pad_helpers.py over the host-staged test
transport, every table table-wise on its owner, --deterministic.  The ids cross the exchange as they are: a pad is the id -1 on every rank.
Writes this rank's parameters after three steps, its predictions and the pad counters."""
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
import dlrm_helpers as H  # noqa: E402
import pad_helpers as PH  # noqa: E402

# global batch 512: the table of bag size 7 has 3,584 entries on its owner (the sorted route), the others ride beside it or take the small route
CFG = dict(B=512, D=8, rows=(1000, 37, 500, 2000), bags=(1, 3, 2, 7), bot=(13, 32, 8), top=(40, 32, 1), lr=0.05)
COUNTERS = ("pad_gather_launches", "pad_update_launches", "ragged_gather_launches", "ragged_update_launches")


def main():
    outdir = sys.argv[1]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    rank, world = dist.get_rank(), dist.get_world_size()
    comm = HostStagedComm()
    m, h = PH.build_pad_model(capi.HIP_LIB_PATH, CFG, PH.model_data(CFG, seed=11), extra_argv=["--device", "0", "--force-exchange", "--deterministic"],
                              comm=comm.struct, rank=rank, world=world)
    out = H.run_steps(m, h, steps=3)[-1]
    for name in COUNTERS:
        out[name] = np.array(m.counter(name))
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
