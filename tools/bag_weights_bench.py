#!/usr/bin/env python3
"""Timings behind per-sample weights on embedding bags (include/ffh_bag_weights.h): the gather and the plain-SGD fused update of one set of
tables, through the C-ABI, at two fills:

  (a) pad, sum          the pad entries of include/ff_hip_pad.h in SUM mode: code the weighted forms leave as it was, and their yardstick
  (b) weighted          the weighted entries on the same ids, with a weight per slot uniform in [0.5, 1.5)

  python tools/bag_weights_bench.py [--batch B] [--dim D] [--rows r-r-...] [--fills F,F] [--dtype fp32|bf16|both] [--out FILE]

Shape and protocol, as tools/pad_bench.py: the table row counts of bench.py's MLPerf workload, the 26 pooling sizes of the DCNv2 recipe, D = 128,
8192 samples; the legs run INTERLEAVED on one device (seven windows each, every window at least 0.2 s of back-to-back launches between two HIP
events), after every id set of every leg has run once; the launches rotate over four id sets.  The update legs keep adding to the tables: the
timings do not depend on the values.  The expectation printed beside each ratio is the bytes a lookup moves, (12 + 4 D) / (8 + 4 D) for fp32 rows
and (12 + 2 D) / (8 + 2 D) for bf16 rows.  Before timing, the weighted gather with every weight 1 is compared bit for bit with the pad gather.
--out appends the report to a file."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pad_bench as PB      # say, window, windows_of: one protocol for both tools

A, Bw = "(a) pad, sum", "(b) weighted"


def report(what, fill, res, expect):
    med = {}
    for name, (n, v) in res.items():
        med[name] = float(np.median(v))
        PB.say(f"  {what:7s} fill {fill:<4g} {name:14s} us: {' '.join(f'{u:8.1f}' for u in v)} | median {med[name]:8.1f} | spread {100 * (v.max() - v.min()) / med[name]:4.1f} %   ({n} per window)")
    PB.say(f"  {what:7s} fill {fill:<4g} (b) / (a) = {med[Bw] / med[A]:.3f}    (bytes per lookup: {expect:.3f})")


def bench(hip, dtype, rows, bags, D, batch, fills):
    import torch
    from dlrm_flexflow_amd import capi
    bags_api, b16, bu, pd, bw = capi.bags_api(hip), capi.bf16_api(hip), capi.bags_update_api(hip), capi.pad_api(hip), capi.bag_weights_api(hip)
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
    out = {k: torch.zeros(batch, ld, device=dev) for k in (A, Bw)}
    grad = torch.empty(batch, ld, device=dev).uniform_(-1e-3, 1e-3)
    make = b16.tables if bf16 else hip.emb_tables
    dims = bags_api.in_dims(bags)
    SUM = capi.AGGR_MODE_SUM
    ws_bytes = bu.workspace_bytes(bags, D, batch) + 256
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    hip.set_workspace(ws, ws_bytes)
    rnd = b16.rounding(capi.BF16_ROUND_NEAREST) if bf16 else None
    row = 2 * D if bf16 else 4 * D
    expect = (12 + row) / (8 + row)
    ones = [torch.ones(batch * L, device=dev) for L in bags]
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
        fwd_arr = {k: [tabs(s, out[k]) for s in range(PB.NSETS)] for k in (A, Bw)}
        gather = {A: lambda s: pd.fwd(fwd_arr[A][s], dims, nt, D, batch, SUM, bf16=bf16),
                  Bw: lambda s: bw.fwd(fwd_arr[Bw][s], wts[s], dims, nt, D, batch, SUM, bf16=bf16)}
        for s in range(PB.NSETS):
            gather[A](s)
            bw.fwd(fwd_arr[Bw][s], ones, dims, nt, D, batch, SUM, bf16=bf16)      # reference 1 of the header
            torch.cuda.synchronize()
            if not out[A].view(torch.int32).equal(out[Bw].view(torch.int32)):
                sys.exit(f"fill {fill}, id set {s}: with every weight 1 the weighted gather is not the pad gather")
            gather[Bw](s)
        plain = [capi.BagsUpdateApi.descriptor(in_dims=bags, out_dim=D, batch=batch, aggr=SUM, lr=1e-3, rounding=rnd,
                                               **{"tables_bf16" if bf16 else "tables": tabs(s, grad)}) for s in range(PB.NSETS)]
        weighted = [bw.descriptor(capi.BagsUpdateApi.descriptor(in_dims=bags, out_dim=D, batch=batch, aggr=SUM, lr=1e-3, rounding=rnd,
                                                                **{"tables_bf16" if bf16 else "tables": tabs(s, grad)}), wts[s]) for s in range(PB.NSETS)]
        update = {A: lambda s: pd.fused(plain[s]), Bw: lambda s: bw.fused(weighted[s])}
        for s in range(PB.NSETS):
            for fn in update.values():
                fn(s)
        torch.cuda.synchronize()
        npad = sum(int((m < 0).sum()) for m in ids[0])
        PB.say(f"{dtype} rows: {nt} tables, D {D}, batch {batch}, {sum(bags)} slots per sample, fill {fill} ({npad / (batch * sum(bags)):.3f} of set 0's slots are pads), "
               f"{PB.WINDOWS} interleaved windows per leg")
        report("gather", fill, PB.windows_of(gather), expect)
        report("update", fill, PB.windows_of(update), expect)
        del ids, wts, fwd_arr, plain, weighted
    del W, out, grad, ws
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", default=None, help="table row counts r-r-... (default: bench.py's MLPerf workload)")
    ap.add_argument("--fills", default="0.5,1", help="the fills to run, comma-separated")
    ap.add_argument("--dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    if a.rows is None:
        import bench as B
        a.rows = B.TERABYTE_ROWS
    rows = [int(x) for x in a.rows.split("-")]
    bags = [int(x) for x in PB.MLPERF_BAGS.split("-")]
    if len(rows) != len(bags):
        sys.exit(f"--rows has {len(rows)} entries, the MLPerf shape {len(bags)} bag sizes")
    import torch
    import _lab
    hip = _lab.load_hip(0)                      # FFH_TOOLS_LIB=<libffhip.so of another build> measures that build
    PB.say(f"device: {torch.cuda.get_device_name(0)}; launches on the null stream, HIP events around each window")
    for dtype in (["fp32", "bf16"] if a.dtype == "both" else [a.dtype]):
        bench(hip, dtype, rows, bags, a.dim, a.batch, [float(f) for f in a.fills.split(",")])
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(PB.LINES) + "\n")


if __name__ == "__main__":
    main()
