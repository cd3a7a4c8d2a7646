#!/usr/bin/env python3
"""Timings behind the gradient of per-sample bag weights (include/ffh_bag_weights_grad.h): one launch of ffh_bag_weights_grad[_bf16] against the
weighted gather of the same ids, through the C-ABI:

  (a) weighted gather   ffh_embedding_fwd_multi_bags_weighted[_bf16] (include/ffh_bag_weights.h): the yardstick -- it reads the same table rows
  (b) weights' gradient  gw[b][l] = dY[b] . W[idx[b][l]], stored

  python tools/bag_weights_grad_bench.py [--batch B] [--dim D] [--rows r-r-...] [--fills F,F] [--dtype fp32|bf16|both] [--shapes mlperf,terabyte] [--out FILE]

Shapes: the table row counts of bench.py's MLPerf workload with the 26 pooling sizes of the DCNv2 recipe ("mlperf"), and the same tables with one
lookup per bag ("terabyte"); D = 128, 8192 samples.  Protocol, as tools/bag_weights_bench.py: the legs run INTERLEAVED on one device (seven windows
each, every window at least 0.2 s of back-to-back launches between two HIP events), after every id set of every leg has run once; the launches
rotate over four id sets.

Bytes, with N real lookups, B bags and R the bytes of a row (4 D, bf16 rows 2 D):
  (a) moves N * (8 + 4 + R) in (id, weight, row) and B * 4 D out;
  (b) moves N * (8 + R) in (id, row), B * 4 D in (the dY row, once per bag) and N * 4 out.
The two sums are equal: by bytes (b) / (a) is 1.000 at every shape.  --out appends the report to a file."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pad_bench as PB      # say, window, windows_of: one protocol for the tools

A, G = "(a) gather", "(b) gradient"


def bench(hip, dtype, shape, rows, bags, D, batch, fills):
    import torch
    from dlrm_flexflow_amd import capi
    bags_api, b16, pd, bw, bg = capi.bags_api(hip), capi.bf16_api(hip), capi.pad_api(hip), capi.bag_weights_api(hip), capi.bag_weights_grad_api(hip)
    dev, nt, bf16 = "cuda:0", len(bags), dtype == "bf16"
    W = []
    for t, R in enumerate(rows):
        if bf16:
            w = torch.empty(R * D, dtype=torch.int16, device=dev)
            b16.call("ffh_init_uniform_bf16", w, R * D, 100 + t, -0.05, 0.05, None)
        else:
            w = torch.empty(R * D, dtype=torch.float32, device=dev)
            hip.call("ffh_init_uniform", w, R * D, 100 + t, -0.05, 0.05, None)
        W.append(w)
    ld = nt * D
    out = torch.zeros(batch, ld, device=dev)
    dY = torch.empty(batch, ld, device=dev).uniform_(-1e-3, 1e-3)
    gw = [torch.zeros(batch * L, device=dev) for L in bags]
    make = b16.tables if bf16 else hip.emb_tables
    dims = bags_api.in_dims(bags)
    SUM = capi.AGGR_MODE_SUM
    for fill in fills:
        ids, wts = [], []
        for s in range(PB.NSETS):
            p = []
            for t, (R, L) in enumerate(zip(rows, bags)):
                i = torch.empty(batch * L, dtype=torch.int64, device=dev)
                hip.call("ffh_gen_indices", i, batch * L, (0x9E3779B97F4A7C15 * (s + 1) + t) & (2**64 - 1), 0, R, None)
                pd.mask(i, batch * L, 1000 * s + t, 0, fill)
                p.append(i)
            ids.append(p)
            wts.append([torch.empty(batch * L, device=dev).uniform_(0.5, 1.5) for L in bags])
        tabs = lambda s, io: make([(ids[s][t], W[t], io.data_ptr() + 4 * D * t, rows[t], ld) for t in range(nt)])
        fwd_arr = [tabs(s, out) for s in range(PB.NSETS)]
        bwd_arr = [tabs(s, dY) for s in range(PB.NSETS)]
        legs = {A: lambda s: bw.fwd(fwd_arr[s], wts[s], dims, nt, D, batch, SUM, bf16=bf16),
                G: lambda s: bg.grad(bwd_arr[s], gw, list(bags), dims, nt, D, batch, bf16=bf16)}
        for s in range(PB.NSETS):
            for fn in legs.values():
                fn(s)
        torch.cuda.synchronize()
        live = sum(int((m >= 0).sum()) for m in ids[0])
        row = 2 * D if bf16 else 4 * D
        mb = (live * (12 + row) + batch * nt * 4 * D) / 1e6
        PB.say(f"{shape}, {dtype} rows: {nt} tables, D {D}, batch {batch}, {sum(bags)} slots per sample, fill {fill} ({live} real lookups in set 0), "
               f"{mb:.1f} MB per launch either way, {PB.WINDOWS} interleaved windows per leg")
        med = {}
        for name, (n, v) in PB.windows_of(legs).items():
            med[name] = float(np.median(v))
            PB.say(f"  fill {fill:<4g} {name:14s} us: {' '.join(f'{u:8.1f}' for u in v)} | median {med[name]:8.1f} | spread {100 * (v.max() - v.min()) / med[name]:4.1f} % | "
                   f"{mb / med[name]:6.2f} TB/s   ({n} per window)")
        PB.say(f"  fill {fill:<4g} (b) / (a) = {med[G] / med[A]:.3f}    (by bytes: 1.000)")
        del ids, wts, fwd_arr, bwd_arr
    del W, out, dY, gw
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", default=None, help="table row counts r-r-... (default: bench.py's MLPerf workload)")
    ap.add_argument("--fills", default="1", help="the fills to run, comma-separated")
    ap.add_argument("--dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--shapes", default="mlperf,terabyte")
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    if a.rows is None:
        import bench as B
        a.rows = B.TERABYTE_ROWS
    rows = [int(x) for x in a.rows.split("-")]
    shapes = {"mlperf": [int(x) for x in PB.MLPERF_BAGS.split("-")], "terabyte": [1] * len(rows)}
    import torch
    import _lab
    hip = _lab.load_hip(0)                      # FFH_TOOLS_LIB=<libffhip.so of another build> measures that build
    PB.say(f"device: {torch.cuda.get_device_name(0)}; launches on the null stream, HIP events around each window")
    for shape in a.shapes.split(","):
        bags = shapes[shape]
        if len(rows) != len(bags):
            sys.exit(f"--rows has {len(rows)} entries, the shape {len(bags)} bag sizes")
        for dtype in (["fp32", "bf16"] if a.dtype == "both" else [a.dtype]):
            bench(hip, dtype, shape, rows, bags, a.dim, a.batch, [float(f) for f in a.fills.split(",")])
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(PB.LINES) + "\n")


if __name__ == "__main__":
    main()
