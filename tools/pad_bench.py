#!/usr/bin/env python3
"""Timings behind DESIGN section 21 (variable-length embedding bags, include/ff_hip_pad.h): the gather and the plain-SGD fused update of one set of
tables, through the C-ABI, four ways:

  (a) ragged, full      ffh_embedding_fwd_multi_bags / ffh_embedding_bwd_fused_multi_bags, no pads: the yardstick of (b)
  (b) pad, full         the pad entries on the same ids (no pad among them): what the flag costs a model that has no pads
  (c) zero row, 0.5     the existing entries on tables with a zero row appended, every pad pointed at it: the workaround, the yardstick of (d)
  (d) pad, 0.5          the pad entries on the same ids with the pads left as -1 (ffh_pad_mask_indices at fill 0.5)

  python tools/pad_bench.py [--batch B] [--dim D] [--rows r-r-...] [--fill F] [--dtype fp32|bf16|both] [--out FILE]

Shape, as tools/bags_bench.py: the table row counts of bench.py's MLPerf workload, the 26 pooling sizes of the DCNv2 recipe, D = 128, 8192 samples.
The legs run INTERLEAVED on one device (seven windows each, every window at least 0.2 s of back-to-back launches between two HIP events), after
every id set of every leg has run once; the launches rotate over four id sets.  Every table is allocated with R + 1 rows: legs (a), (b), (d) pass
num_entries = R, leg (c) R + 1.  The update legs keep adding to the tables (and leg (c) to its zero row): the timings do not depend on the values.
Before timing, (b) is compared with (a) and (d) with (c) bit for bit on the gather.  --out appends the report to a file."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MLPERF_BAGS = "3-2-1-2-6-1-1-1-1-7-3-8-1-6-9-5-1-1-1-12-100-27-10-3-1-1"
NSETS, WINDOWS, MIN_SECONDS = 4, 7, 0.2
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def window(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i % NSETS)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def windows_of(legs):
    """Interleaved windows of every leg (name -> fn), each leg's window count sized on itself; returns name -> (launches per window, us per launch)."""
    n = {}
    for name, fn in legs.items():
        k = 16
        while True:
            us = window(fn, k)
            if us * k >= MIN_SECONDS * 1e6:
                break
            k = int(k * max(2.0, 1.2 * MIN_SECONDS * 1e6 / (us * k)))
        n[name] = k
    t = {name: [] for name in legs}
    for _ in range(WINDOWS):
        for name, fn in legs.items():
            t[name].append(window(fn, n[name]))
    return {name: (n[name], np.array(v)) for name, v in t.items()}


def report(what, res):
    med = {}
    for name, (n, v) in res.items():
        med[name] = float(np.median(v))
        say(f"  {what:7s} {name:18s} us: {' '.join(f'{u:8.1f}' for u in v)} | median {med[name]:8.1f} | spread {100 * (v.max() - v.min()) / med[name]:4.1f} %   ({n} per window)")
    say(f"  {what:7s} (b) / (a) = {med['(b) pad, full'] / med['(a) ragged, full']:.3f}    (d) / (c) = {med['(d) pad, fill'] / med['(c) zero row, fill']:.3f}")


def bench(hip, dtype, rows, bags, D, batch, fill):
    import torch
    from dlrm_flexflow_amd import capi
    bags_api, b16, bu, pd = capi.bags_api(hip), capi.bf16_api(hip), capi.bags_update_api(hip), capi.pad_api(hip)
    dev, nt, bf16 = "cuda:0", len(bags), dtype == "bf16"
    W = []
    for t, R in enumerate(rows):
        if bf16:
            w = torch.empty((R + 1) * D, dtype=torch.int16, device=dev)
            b16.call("ffh_init_uniform_bf16", w, R * D, 100 + t, -0.05, 0.05, None)
        else:
            w = torch.empty((R + 1) * D, dtype=torch.float32, device=dev)
            hip.call("ffh_init_uniform", w, R * D, 100 + t, -0.05, 0.05, None)
        w[R * D:] = 0
        W.append(w)
    full, padded, zero_row = [], [], []
    for s in range(NSETS):
        f, p, z = [], [], []
        for t, (R, L) in enumerate(zip(rows, bags)):
            i = torch.empty(batch * L, dtype=torch.int64, device=dev)
            hip.call("ffh_gen_indices", i, batch * L, (0x9E3779B97F4A7C15 * (s + 1) + t) & (2**64 - 1), 0, R, None)
            m = i.clone()
            pd.mask(m, batch * L, 1000 * s + t, 0, fill)
            f.append(i); p.append(m); z.append(torch.where(m < 0, torch.full_like(m, R), m))
        full.append(f); padded.append(p); zero_row.append(z)
    ld = nt * D
    names = ["(a) ragged, full", "(b) pad, full", "(c) zero row, fill", "(d) pad, fill"]
    ids_of = dict(zip(names, (full, full, zero_row, padded)))
    out = {k: torch.zeros(batch, ld, device=dev) for k in names}
    grad = torch.empty(batch, ld, device=dev).uniform_(-1e-3, 1e-3)
    make = b16.tables if bf16 else hip.emb_tables
    tabs = lambda k, s, io: make([(ids_of[k][s][t], W[t], io.data_ptr() + 4 * D * t, rows[t] + (1 if k.startswith("(c)") else 0), ld) for t in range(nt)])
    dims = bags_api.in_dims(bags)
    SUM = capi.AGGR_MODE_SUM
    fwd_arr = {k: [tabs(k, s, out[k]) for s in range(NSETS)] for k in names}
    plain_fwd = "ffh_embedding_fwd_multi_bags_bf16" if bf16 else "ffh_embedding_fwd_multi_bags"
    gather = {k: ((lambda s, k=k: pd.fwd(fwd_arr[k][s], dims, nt, D, batch, SUM, bf16=bf16)) if "pad" in k else
                  (lambda s, k=k: bags_api.call(plain_fwd, fwd_arr[k][s], dims, nt, D, batch, SUM))) for k in names}
    for s in range(NSETS):
        for fn in gather.values():
            fn(s)
        torch.cuda.synchronize()
        for x, y in ((names[1], names[0]), (names[3], names[2])):
            if not out[x].view(torch.int32).equal(out[y].view(torch.int32)):
                sys.exit(f"id set {s}: the gathers of {x} and {y} differ")
    ws_bytes = bu.workspace_bytes(bags, D, batch) + 256
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    hip.set_workspace(ws, ws_bytes)
    rnd = b16.rounding(capi.BF16_ROUND_NEAREST) if bf16 else None
    desc = {k: [capi.BagsUpdateApi.descriptor(in_dims=bags, out_dim=D, batch=batch, aggr=SUM, lr=1e-3, rounding=rnd,
                                              **{"tables_bf16" if bf16 else "tables": tabs(k, s, grad)}) for s in range(NSETS)] for k in names}
    update = {k: ((lambda s, k=k: pd.fused(desc[k][s])) if "pad" in k else (lambda s, k=k: bu.call(desc[k][s]))) for k in names}
    for s in range(NSETS):
        for fn in update.values():
            fn(s)
    torch.cuda.synchronize()
    npad = sum(int((m < 0).sum()) for m in padded[0])
    say(f"{dtype} rows: {nt} tables, D {D}, batch {batch}, {sum(bags)} slots per sample, fill {fill} ({npad / (batch * sum(bags)):.3f} of set 0's slots are pads), "
        f"{WINDOWS} interleaved windows per leg")
    report("gather", windows_of(gather))
    report("update", windows_of(update))
    del W, full, padded, zero_row, out, grad, ws
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", default=None, help="table row counts r-r-... (default: bench.py's MLPerf workload)")
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    if a.rows is None:
        import bench as B
        a.rows = B.TERABYTE_ROWS
    rows = [int(x) for x in a.rows.split("-")]
    bags = [int(x) for x in MLPERF_BAGS.split("-")]
    if len(rows) != len(bags):
        sys.exit(f"--rows has {len(rows)} entries, the MLPerf shape {len(bags)} bag sizes")
    import torch
    import _lab
    hip = _lab.load_hip(0)                      # FFH_TOOLS_LIB=<libffhip.so of another build> measures that build
    say(f"device: {torch.cuda.get_device_name(0)}; launches on the null stream, HIP events around each window")
    for dtype in (["fp32", "bf16"] if a.dtype == "both" else [a.dtype]):
        bench(hip, dtype, rows, bags, a.dim, a.batch, a.fill)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
