"""One rank of the two-rank checkpoint tests (launched by tests/test_checkpoint_cpu.py and tests/test_gpu_checkpoint.py):
    _dist_worker_checkpoint.py <cpu|gpu> <save|load> <outdir> <checkpoint dir> [more driver flags]
cpu: kernels from the CPU oracle, the product's TorchComm over gloo.  gpu: the HIP kernels, both ranks on one GPU, the host-staged test
transport (tests/host_staged_comm.py).  save: one epoch of the tiny model through the driver object, --save-checkpoint; load: a new pair of
ranks with --load-checkpoint (nothing left to train).  Either writes <outdir>/<mode>-rank<r>.npz: the model's state digest and the epoch."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dlrm_flexflow_amd import ffmodel  # noqa: E402
from dlrm_flexflow_amd.comm import TorchComm  # noqa: E402
import checkpoint_helpers as K  # noqa: E402
import dlrm_helpers as H  # noqa: E402


def main():
    where, mode, outdir, ckdir = sys.argv[1:5]
    if where == "gpu":
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    if where == "gpu":
        from host_staged_comm import HostStagedComm
        comm, backend = HostStagedComm(), ["--device", "0"]
    else:
        comm, backend = TorchComm(on_gpu=False), ["--backend", H.oracle_backend()]
    flags = backend + K.MODEL + ["--optimizer", "sgd-momentum", "--epochs", "1"]
    flags += ["--save-checkpoint", ckdir] if mode == "save" else ["--load-checkpoint", ckdir]
    flags += sys.argv[5:]                  # a placement, or a later --epochs / --save-checkpoint (the last one given holds)
    app = ffmodel.DLRM(flags, comm=comm.struct)
    app.run_epochs()
    out = {"digest": np.array(app.model.state_digest(), dtype=np.uint64), "epochs_done": np.array(app.start_epoch if mode == "load" else 1)}
    np.savez(os.path.join(outdir, f"{mode}-rank{dist.get_rank()}.npz"), **out)
    app.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
