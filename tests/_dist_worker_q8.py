"""One rank of several sharing ONE GPU (launched by tests/test_gpu_q8_ranks.py): the golden DLRM with the BCE loss over the host-staged test
transport, its tables placed table-wise, evaluated with --eval-embedding-dtype int8 through the exchange buffers."""
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
import ctr_helpers as CH  # noqa: E402


def main():
    outdir, train_steps = sys.argv[1], int(sys.argv[2])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    comm = HostStagedComm()
    m, h = CH.build_bce_dlrm(capi.HIP_LIB_PATH, comm=comm.struct, overlap=True, force_exchange=True,
                             extra_argv=["--device", "0", "--deterministic", "--eval-batches", "1", "--eval-embedding-dtype", "int8"])
    out = CH.train_then_evaluate(m, train_steps)
    out["q8"] = np.array([m.counter("q8_quantize_launches"), m.counter("q8_gather_launches")])
    np.savez(os.path.join(outdir, f"rank{dist.get_rank()}.npz"), **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
