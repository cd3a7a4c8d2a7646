"""One of two ranks that share the GPU (launched by tests/test_gpu_cross.py): the DCNv2 model of tests/cross_helpers.py on the product
kernels, global batch 128, collectives through the host-staged test transport over gloo (RCCL refuses two ranks on one device).
Writes this rank's parameters and prediction after two optimizer steps to <outdir>/rank<r>.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dlrm_flexflow_amd import capi, ffmodel  # noqa: E402
from host_staged_comm import HostStagedComm  # noqa: E402
import cross_helpers as X  # noqa: E402


def main():
    outdir, L, R = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    comm = HostStagedComm()
    app = ffmodel.DLRM(X.dcn_args(capi.HIP_LIB_PATH, L, R, ["--device", "0", *sys.argv[4:]]), comm=comm.struct)
    m = app.model
    app.warmup()
    app.train_steps(1, trace=False)
    m.sync()
    out = {"pred": m.layer_output(m.num_layers - 1).get()}
    for l in range(m.num_layers):
        for i in range(m.layer_num_weights(l)):
            if m.parameter(l, i).is_local:
                out[f"{m.layer_name(l)}/{i}"] = m.parameter(l, i).get_weights()
    out["allreduce_calls"] = np.array(comm.calls["allreduce"] + comm.calls.get("allreduce_buckets", 0))
    np.savez(os.path.join(outdir, f"rank{dist.get_rank()}.npz"), **out)
    app.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
