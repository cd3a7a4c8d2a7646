"""One rank of several sharing ONE GPU (launched by tests/test_gpu_shuffle.py): the DLRM driver object on a data set with
--data-randomize total over the host-staged test transport; records what every step of one epoch trained on -- this rank's labels and
dense rows, and the ids of every table whose input this rank holds."""
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


def main():
    outdir, dataset, steps, flags = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4:]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    comm = HostStagedComm()
    app = ffmodel.DLRM(["--backend", capi.HIP_LIB_PATH] + flags + ["--dataset", dataset, "--device", "0", "--force-exchange", "--deterministic"],
                       comm=comm.struct)
    held = [t for t in range(app.num_tables) if app.sparse_input(t).is_local]
    rec = {"label": [], "dense": [], **{f"sparse{t}": [] for t in held}}
    for _ in range(steps):
        app.train_steps(1, trace=False)
        app.model.sync()
        rec["label"].append(app.label_input().get().reshape(-1))
        rec["dense"].append(app.dense_input().get())
        for t in held:
            rec[f"sparse{t}"].append(app.sparse_input(t).get(np.int64).reshape(-1))
    np.savez(os.path.join(outdir, f"rank{dist.get_rank()}.npz"), **{k: np.stack(v) for k, v in rec.items()})
    app.close()
    sys.stdout.flush()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
