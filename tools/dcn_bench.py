#!/usr/bin/env python3
"""Timings behind DESIGN section 14 (--arch-interaction-op dcn), on the stream with HIP events:

  python tools/dcn_bench.py kernels          ffh_cross_fwd / ffh_cross_bwd alone through the C-ABI at (32768, 3456) and (4096, 3456), tight strides
                                             (the 16-byte path), against the bytes the contract moves: 16 B D forward, 12 ... 32 B D backward by mode.
                                             Back-to-back launches rotate over buffer sets that together exceed the 256 MiB Infinity Cache, so that
                                             no launch finds the operands of the one before in it.
  python tools/dcn_bench.py driver [batch]   the driver's step for the DCNv2 shape: Terabyte tables, --arch-sparse-feature-size 128, bottom MLP
                                             13-512-256-128, --arch-interaction-op dcn (3 layers, rank 512), top MLP 3456-1024-1024-512-256-1,
                                             batch 32768; next to the same shape with --arch-interaction-op cat; three interleaved runs per side
"""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SKIP, STORE, ADD = 0, 1, 2
NAMES = {SKIP: "skip", STORE: "store", ADD: "add"}


def bwd_bytes(mode_x0, mode_xl, same):
    """bytes per element of ffh_cross_bwd (include/ff_hip_cross.h): dy, x0 read and dv written always; v read and dx0 written unless skipped, its old
    value read when added to; likewise dxl (dx0 == dxl: one write under mode_x0)"""
    b = 12
    if mode_x0 != SKIP:
        b += 8 + (4 if mode_x0 == ADD else 0)
    if not same and mode_xl != SKIP:
        b += 4 + (4 if mode_xl == ADD else 0)
    return b


def time_launches(fn, sets, min_seconds=0.3):
    import torch
    for k in range(len(sets)):
        fn(k)                                   # every buffer set once: code objects loaded, pages touched
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, out = 8 * len(sets), []
    while True:                                 # size the window: at least min_seconds of launches
        e0.record()
        for i in range(n):
            fn(i % len(sets))
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_seconds * 1e3:
            break
        n = int(n * max(2.0, 1.2 * min_seconds * 1e3 / max(ms, 1e-3)))
    for _ in range(3):
        e0.record()
        for i in range(n):
            fn(i % len(sets))
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / n)
    return out, n


def kernels_bench():
    import torch
    from dlrm_flexflow_amd import capi
    hip = capi.load_hip(0)
    cross = capi.cross_api(hip)
    s = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; launches on one stream, HIP events around the window, us per launch (three windows)")
    for B, D in ((32768, 3456), (4096, 3456)):
        elems = B * D
        nsets = max(2, int(np.ceil(3 * (256 << 20) / (7 * 4 * elems))))      # 7 operands per set; the sets together: >= 3 x the cache
        sets = [[torch.randn(B, D, device="cuda:0") for _ in range(7)] for _ in range(nsets)]
        print(f"({B}, {D}): {nsets} buffer sets of 7 x {4 * elems / 1e6:.0f} MB")

        def fwd(k):
            y, x0, v, xl = sets[k][:4]
            cross.call("ffh_cross_fwd", y, D, x0, D, v, D, xl, D, B, D, s)
        us, n = time_launches(fwd, sets)
        print(f"  fwd                      {16 * elems / 1e6:8.1f} MB  {' '.join(f'{u:8.1f}' for u in us)} us  ({n} launches)  {16 * elems / min(us) / 1e6:6.2f} TB/s at the best", flush=True)
        cases = [(m0, ml, False) for m0 in (SKIP, STORE, ADD) for ml in (SKIP, STORE, ADD)] + [(STORE, STORE, True), (ADD, ADD, True)]
        for m0, ml, same in cases:
            def bwd(k, m0=m0, ml=ml, same=same):
                dy, x0, v, dv, dx0, dxl = sets[k][:6]
                cross.call("ffh_cross_bwd", dy, D, x0, D, v, D, dv, D, dx0, D, m0, dx0 if same else dxl, D, ml, B, D, s)
            us, n = time_launches(bwd, sets)
            nbytes = bwd_bytes(m0, ml, same) * elems
            tag = f"bwd x0={NAMES[m0]} xl={NAMES[ml]}" + (" (one buffer)" if same else "")
            print(f"  {tag:32s} {nbytes / 1e6:8.1f} MB  {' '.join(f'{u:8.1f}' for u in us)} us  ({n} launches)  {nbytes / min(us) / 1e6:6.2f} TB/s at the best", flush=True)
        del sets
        torch.cuda.empty_cache()


def driver_bench(batch):
    import bench
    w = bench.workload("terabyte", batch)
    base = ["-b", str(batch), "--arch-sparse-feature-size", "128", "--arch-embedding-size", w["rows"], "--arch-mlp-bot", "13-512-256-128",
            "--arch-mlp-top", "3456-1024-1024-512-256-1", "--data-size", str(batch * 8), "--epochs", "6"]
    sides = {"cat": ["--arch-interaction-op", "cat"], "dcn": ["--arch-interaction-op", "dcn", "--dcn-num-layers", "3", "--dcn-low-rank-dim", "512"]}
    exe = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
    out = {k: [] for k in sides}
    for rep in range(3):
        for name, flags in sides.items():
            r = subprocess.run([exe, *base, *flags], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"driver failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
            m = re.search(r"THROUGHPUT = ([0-9.]+) samples/s", r.stdout)
            us = batch / float(m.group(1)) * 1e6
            out[name].append(us)
            print(f"batch {batch} run {rep} --arch-interaction-op {name}: {us:9.1f} us per step (6 epochs of 8 steps, eager first epoch included)", flush=True)
    for name, t in out.items():
        print(f"batch {batch} --arch-interaction-op {name}: min {min(t):9.1f}  median {float(np.median(t)):9.1f}  max {max(t):9.1f} us per step")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "kernels":
        kernels_bench()
    elif len(sys.argv) > 1 and sys.argv[1] == "driver":
        driver_bench(int(sys.argv[2]) if len(sys.argv) > 2 else 32768)
    else:
        sys.exit(__doc__)
