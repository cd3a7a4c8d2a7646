#!/usr/bin/env python3
"""Timings behind DESIGN section 13 (--data-randomize total), on the stream with HIP events:

  python tools/shuffle_bench.py gather            the batch load alone: one ffh_batch_gather launch against the copies DataLoader::load_batch
                                                  issues (one ffh_memcpy_d2d per table, one for the dense features, one for the labels),
                                                  at the Kaggle shape (2048 x 26 tables) and the Terabyte shape (32768 x 26 tables)
  python tools/shuffle_bench.py driver [shape]    the driver's step with --data-randomize total against none on one
                                                  --synthetic-labels logistic run, interleaved, three runs per side (kaggle | terabyte)
"""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES, DENSE = 26, 13


def gather_bench():
    """DataLoader::next_batch alone, issued back to back from C++ (flexflow_dlrm_time_kernel 12: HIP events on the compute stream around 200
    loads): the 28 copies of file order against the one gather launch.  The tables are small (their size does not matter to the load), the
    data set is 64 batches, so consecutive loads read different rows."""
    from dlrm_flexflow_amd import ffmodel
    for name, B, D, bot, top in (("kaggle 2048 x 26", 2048, 16, "13-512-256-64-16", "432-512-256-1"),
                                 ("terabyte 32768 x 26", 32768, 128, "13-512-256-128", "3456-1024-1024-512-256-1")):
        flags = ["-b", str(B), "--arch-sparse-feature-size", str(D), "--arch-embedding-size", "-".join(["100000"] * TABLES), "--arch-mlp-bot", bot,
                 "--arch-mlp-top", top, "--data-size", str(B * 64), "--synthetic-labels", "logistic"]
        moved = B * (TABLES * 8 + DENSE * 4 + 4)
        for rep in range(2):
            for mode in ("none", "total"):
                app = ffmodel.DLRM(flags + ["--data-randomize", mode])
                us = [app.time_kernel(12, 200) * 1e3 for _ in range(3)]
                app.close()
                print(f"{name} rep {rep} --data-randomize {mode:5s} ({'28 copies' if mode == 'none' else '1 gather '}): "
                      f"{' '.join(f'{u:6.1f}' for u in us)} us per load  ({moved / 1e6:.2f} MB, {moved / min(us) / 1e3:.0f} GB/s at the best)", flush=True)


def driver_bench(shape):
    sys.path.insert(0, ROOT)
    import bench
    w = bench.workload(shape, bench.DEFAULT_BATCH[shape])
    B = w["B"]
    flags = ["-b", str(B), "--arch-sparse-feature-size", str(w["D"]), "--arch-embedding-size", w["rows"], "--arch-mlp-bot", w["bot"],
             "--arch-mlp-top", w["top"], "--data-size", str(B * 64), "--synthetic-labels", "logistic", "--epochs", "4"]
    exe = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
    out = {"none": [], "total": []}
    for rep in range(3):
        for mode in ("none", "total"):
            r = subprocess.run([exe, *flags, "--data-randomize", mode], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"driver failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
            m = re.search(r"THROUGHPUT = ([0-9.]+) samples/s", r.stdout)
            us = B / float(m.group(1)) * 1e6
            out[mode].append(us)
            print(f"{shape} run {rep} --data-randomize {mode:5s}: {us:9.1f} us per step (4 epochs of 64 steps, eager first epoch included)", flush=True)
    for mode, t in out.items():
        print(f"{shape} --data-randomize {mode:5s}: min {min(t):9.1f}  median {float(np.median(t)):9.1f}  max {max(t):9.1f} us per step")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "gather":
        gather_bench()
    elif len(sys.argv) > 1 and sys.argv[1] == "driver":
        driver_bench(sys.argv[2] if len(sys.argv) > 2 else "kaggle")
    else:
        sys.exit(__doc__)
