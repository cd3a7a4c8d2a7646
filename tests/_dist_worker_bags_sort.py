"""One rank of two sharing ONE GPU (launched by tests/test_gpu_bags_sort_model.py): a DLRM of mixed bag sizes over the host-staged test
transport, every table table-wise on its owner (each rank owns two tables of differing bag sizes), --deterministic, with the flag given on the
command line (--early-sort / --no-early-sort).  Writes this rank's parameters before and after three steps, and the sort counters."""
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

# global batch 512: the table of bag size 7 has 3,584 entries on its owner (the sorted route), the others ride the small route or beside it
CFG = dict(B=512, D=8, rows=(1000, 37, 500, 2000), bags=(1, 3, 2, 7), bot=(13, 32, 8), top=(40, 32, 1), lr=0.05)
COUNTERS = ("ragged_early_sorts", "early_sorts", "ragged_update_launches")


def main():
    outdir, flag = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://{os.environ['MASTER_ADDR']}:{os.environ['MASTER_PORT']}",
                            rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    rank, world = dist.get_rank(), dist.get_world_size()
    comm = HostStagedComm()
    B, D, rows, bags, bot, top = (CFG[k] for k in ("B", "D", "rows", "bags", "bot", "top"))
    c = ffmodel.FFConfig(argv=["-b", str(B), "--device", "0", "--force-exchange", "--deterministic", "--ragged-update", flag],
                         backend=capi.HIP_LIB_PATH, comm=comm.struct)
    c.set(enable_graph=False, overlap_embedding=True, dense_embedding_update=False)
    m = ffmodel.FFModel(c)
    sparse = [m.create_tensor([B, L], ffmodel.DT_INT64) for L in bags]
    dense = m.create_tensor([B, bot[0]], ffmodel.DT_FLOAT)
    x = dense
    for i in range(len(bot) - 1):
        x = m.dense(x, bot[i + 1], capi.AC_MODE_RELU)
    ly = [m.embedding(s, r, D, capi.AGGR_MODE_SUM) for s, r in zip(sparse, rows)]
    z = m.concat([x] + ly, 1)
    for i in range(len(top) - 1):
        z = m.dense(z, top[i + 1], capi.AC_MODE_SIGMOID if i == len(top) - 2 else capi.AC_MODE_RELU)
    m.set_sgd_optimizer(lr=CFG["lr"])
    m.compile()
    m.init_layers()
    rng = np.random.default_rng(11)      # the same data on both ranks and in both legs
    data = {"dense": rng.random((B, bot[0]), dtype=np.float32), "label": rng.integers(0, 2, (B, 1)).astype(np.float32)}
    for t, (r, L) in enumerate(zip(rows, bags)):
        data[f"sparse{t}"] = rng.integers(0, r, (B, L)).astype(np.int64)
    sl = slice(rank * B // world, (rank + 1) * B // world)
    dense.set(data["dense"][sl])
    m.label_tensor.set(data["label"][sl])
    for t, s in enumerate(sparse):
        if s.is_local:
            s.set(data[f"sparse{t}"])
    emb0 = len(bot) - 1
    layers = {f"bot.{i}": i for i in range(len(bot) - 1)}
    layers.update({f"emb.{t}": emb0 + t for t in range(len(rows))})
    layers.update({f"top.{i}": emb0 + len(rows) + 1 + i for i in range(len(top) - 1)})

    def params(prefix=""):
        rec = {}
        for k, li in layers.items():
            p = m.parameter(li, 0)
            if p.is_local:
                rec[prefix + k + ".weight"] = p.get_weights()
            if not k.startswith("emb"):
                rec[prefix + k + ".bias"] = m.parameter(li, 1).get_weights()
        return rec

    out = params("init/")
    for _ in range(3):
        m.forward(); m.zero_gradients(); m.backward(); m.update()
    m.sync()
    out.update(params())
    out["pred"] = m.layer_output(m.num_layers - 1).get()
    for name in COUNTERS:
        out[name] = np.array(m.counter(name))
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
