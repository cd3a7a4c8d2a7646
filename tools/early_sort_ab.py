#!/usr/bin/env python3
"""The step of a model of mixed bag sizes with its sort behind the gather (--early-sort) against the sort in front of the apply (--no-early-sort):
the measurement behind DESIGN section 19, "The early sort of a mixed model".

  python tools/early_sort_ab.py [--runs 5] [--steps 300] [--modes exact,split,tensor,exchange]

The MLPerf DLRM-DCNv2 shape through the DLRM application object, as bench.py drives it: 26 tables with the Terabyte row counts, D = 128, the 26
bag sizes, --arch-interaction-op dcn, bottom MLP 13-512-256-128, top MLP 3456-1024-1024-512-256-1, --ragged-update; 8192 samples on one GPU in
exact fp32 (`exact`), --fp32-split-bf16x3 (`split`) and --allow-tensor-op-math-conversion (`tensor`); `exchange` is the 4096-sample per-rank
shape with --force-exchange on one RCCL rank, exact fp32.  Every run is a fresh child process (one leg, one mode: 30 untimed steps, then --steps
timed ones, hipGraph replay where the step can be captured); the two legs alternate, --runs each.  Prints every run, each leg's min / median / max,
the counters that say which sort ran, and for each mode whether the legs differ by more than their own run-to-run spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = {"exact": (8192, []), "split": (8192, ["--fp32-split-bf16x3"]), "tensor": (8192, ["--allow-tensor-op-math-conversion"]),
         "exchange": (4096, ["--force-exchange"])}


def leg(mode, flag, steps):
    import torch
    import bags_helpers
    import bench as B
    from dlrm_flexflow_amd import ffmodel
    batch, extra = MODES[mode]
    torch.cuda.set_device(0)
    comm = None
    if mode == "exchange":
        import torch.distributed as dist
        from dlrm_flexflow_amd.comm import RcclComm, TorchComm
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29537")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        comm = RcclComm(TorchComm(on_gpu=True))
    w = dict(B.workload("terabyte", batch), extra=["--arch-interaction-op", "dcn"])
    flags = B.flags_of(w, ["--device", "0", "--embedding-bag-sizes", "-".join(map(str, bags_helpers.MLPERF_BAGS)), "--ragged-update", flag] + extra)
    app = ffmodel.DLRM(flags, comm=comm.struct if comm else None)
    app.warmup()
    trace = comm is None
    app.train_steps(30, trace=trace)
    app.model.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    app.train_steps(steps, trace=trace)
    app.model.sync()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {"ms": ms, "graph_replays": app.model.counter("graph_replays")}
    out.update({c: app.model.counter(c) for c in ("early_sorts", "ragged_early_sorts", "ragged_update_launches")})
    app.close()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--modes", default="exact,split,tensor,exchange")
    ap.add_argument("--leg", nargs=2, metavar=("MODE", "FLAG"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg[0], "--" + a.leg[1], a.steps)
    import numpy as np
    legs = ("--early-sort", "--no-early-sort")
    for mode in a.modes.split(","):
        ms = {f: [] for f in legs}
        for r in range(a.runs):
            for f in (legs if r % 2 == 0 else legs[::-1]):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--leg", mode, f[2:]], capture_output=True, text=True, timeout=600)
                line = [x for x in p.stdout.splitlines() if x.startswith("LEG ")]
                if p.returncode != 0 or not line:
                    sys.exit(f"{mode} {f}: run {r} failed (exit status {p.returncode})\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
                d = json.loads(line[0][4:])
                ms[f].append(d["ms"])
                print(f"{mode:9s} run {r} {f:16s} {d['ms']:.4f} ms per step  early_sorts {d['early_sorts']} ragged_early_sorts {d['ragged_early_sorts']} "
                      f"ragged_update_launches {d['ragged_update_launches']} graph_replays {d['graph_replays']}", flush=True)
        v = {f: np.array(ms[f]) for f in legs}
        for f in legs:
            print(f"{mode:9s} {f:16s} min {v[f].min():.4f} median {np.median(v[f]):.4f} max {v[f].max():.4f} ms per step ({MODES[mode][0]} samples)")
        e, n = v[legs[0]], v[legs[1]]
        spread = max(e.max() - e.min(), n.max() - n.min())
        diff = float(np.median(e) - np.median(n))
        verdict = "level with" if abs(diff) <= spread else ("faster than" if diff < 0 else "slower than")
        print(f"{mode:9s} the early sort is {verdict} --no-early-sort: medians differ by {diff * 1e3:+.1f} us ({100 * diff / np.median(n):+.2f} %), "
              f"the wider leg's run-to-run spread is {spread * 1e3:.1f} us", flush=True)


if __name__ == "__main__":
    main()
