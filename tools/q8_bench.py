#!/usr/bin/env python3
"""Timings behind DESIGN section 20 (8-bit embedding rows for evaluation, include/ff_hip_q8.h): the gather of one set of ids from the same tables
stored four ways, through the C-ABI, and the quantizer that makes the 8-bit rows:

  fp32     ffh_embedding_fwd_multi[_bags]            the yardstick: the gather every evaluation ran before
  bf16     ffh_embedding_fwd_multi[_bags]_bf16
  int8     ffh_embedding_fwd_multi[_bags]_q8          rows of D + 8 bytes (the default, fbgemm's layout)
  int8/16  the same from rows of D + 8 rounded up to 16 bytes (no row straddles a 16-byte boundary; an A/B, not the default)
  quantize ffh_embedding_quantize_q8                  every table in one launch, fp32 source

  python tools/q8_bench.py [--shape terabyte|mlperf|both] [--batch B] [--dim D] [--rows r-r-...]

Shapes, as tools/bags_bench.py: the table row counts of bench.py's MLPerf workload, 26 tables, D = 128, 8192 samples; "terabyte" looks up one id per
bag (the uniform entries), "mlperf" the 26 pooling sizes of the DCNv2 recipe (the ragged entries).  The legs run INTERLEAVED on one device (seven
windows each, every window at least 0.2 s of back-to-back launches between two HIP events), after every id set of every leg has run once; the launches
rotate over four id sets.  Each leg is priced as a fraction of the HBM rate (8 TB/s) by its algorithmic bytes, summed over the tables:
batch * (L_t * (8 + row bytes) + 4 * D), row bytes = 4 D, 2 D, D + 8 or the padded size; the quantizer by rows * (4 D + row bytes).  The int8 legs'
outputs are compared with each other bit for bit (that they equal the fp32 gather of the dequantized table is tests/test_gpu_q8.py)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MLPERF_BAGS = "3-2-1-2-6-1-1-1-1-7-3-8-1-6-9-5-1-1-1-12-100-27-10-3-1-1"
HBM_PEAK = 8.0e12
NSETS, WINDOWS, MIN_SECONDS = 4, 7, 0.2


def gather_bytes(batch, bags, D, row_bytes):
    return sum(batch * (L * (8 + row_bytes) + 4 * D) for L in bags)


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


def report(name, what, n, v, nbytes, base=None):
    med = float(np.median(v))
    rel = "" if base is None else f" | {med / base:.3f} of fp32"
    print(f"  {name:9s} {what:34s} {nbytes / 1e6:8.1f} MB | us: {' '.join(f'{u:7.1f}' for u in v)} | median {med:7.1f} | spread "
          f"{100 * (v.max() - v.min()) / med:4.1f} % | {nbytes / med / 1e6 / (HBM_PEAK / 1e12):.3f} of 8 TB/s{rel}   ({n} per window)", flush=True)
    return med


def bench(hip, q8, bags_api, b16, rows, bags, D, batch, shape):
    import torch
    from dlrm_flexflow_amd import capi
    dev, nt = "cuda:0", len(bags)
    rb = {"int8": q8.row_bytes(D), "int8/16": (D + 8 + 15) // 16 * 16}
    w32, w16, img = [], [], {k: [] for k in rb}
    for t, R in enumerate(rows):
        w = torch.empty(R * D, dtype=torch.float32, device=dev)
        hip.call("ffh_init_uniform", w, R * D, 100 + t, -0.05, 0.05, None)
        h = torch.empty(R * D, dtype=torch.int16, device=dev)
        b16.call("ffh_init_uniform_bf16", h, R * D, 100 + t, -0.05, 0.05, None)
        w32.append(w); w16.append(h)
        for k in rb:
            img[k].append(torch.empty(R * rb[k], dtype=torch.uint8, device=dev))
    src = {k: q8.sources([(w32[t], img[k][t], rows[t], rb[k], 0) for t in range(nt)]) for k in rb}
    for k in rb:
        q8.quantize(src[k], nt, D)
    ids = []
    for s in range(NSETS):
        per = []
        for t, (R, L) in enumerate(zip(rows, bags)):
            i = torch.empty(batch * L, dtype=torch.int64, device=dev)
            hip.call("ffh_gen_indices", i, batch * L, (0x9E3779B97F4A7C15 * (s + 1) + t) & (2**64 - 1), 0, R, None)
            per.append(i)
        ids.append(per)
    ld = nt * D
    names = ["fp32", "bf16", "int8", "int8/16"]
    out = {k: torch.zeros(batch, ld, device=dev) for k in names}
    io = lambda k, t: out[k].data_ptr() + 4 * D * t
    arr = {"fp32": [hip.emb_tables([(ids[s][t], w32[t], io("fp32", t), rows[t], ld) for t in range(nt)]) for s in range(NSETS)],
           "bf16": [b16.tables([(ids[s][t], w16[t], io("bf16", t), rows[t], ld) for t in range(nt)]) for s in range(NSETS)]}
    for k in rb:
        arr[k] = [q8.tables([(ids[s][t], img[k][t], io(k, t), rows[t], ld, rb[k]) for t in range(nt)]) for s in range(NSETS)]
    dims = bags_api.in_dims(bags)
    uniform = len(set(bags)) == 1
    SUM = capi.AGGR_MODE_SUM
    if uniform:
        L = bags[0]
        legs = {"fp32": lambda s: hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, arr["fp32"][s], nt, L, D, batch, SUM, None), "fwd_multi"),
                "bf16": lambda s: b16.call("ffh_embedding_fwd_multi_bf16", arr["bf16"][s], nt, L, D, batch, SUM, None),
                "int8": lambda s: q8.fwd(arr["int8"][s], nt, L, D, batch, SUM),
                "int8/16": lambda s: q8.fwd(arr["int8/16"][s], nt, L, D, batch, SUM)}
    else:
        legs = {"fp32": lambda s: bags_api.call("ffh_embedding_fwd_multi_bags", arr["fp32"][s], dims, nt, D, batch, SUM),
                "bf16": lambda s: bags_api.call("ffh_embedding_fwd_multi_bags_bf16", arr["bf16"][s], dims, nt, D, batch, SUM),
                "int8": lambda s: q8.fwd_bags(arr["int8"][s], dims, nt, D, batch, SUM),
                "int8/16": lambda s: q8.fwd_bags(arr["int8/16"][s], dims, nt, D, batch, SUM)}
    for s in range(NSETS):                      # every id set of every leg once: code objects loaded, pages touched
        for fn in legs.values():
            fn(s)
        torch.cuda.synchronize()
        if not out["int8"].view(torch.int32).equal(out["int8/16"].view(torch.int32)):
            sys.exit(f"id set {s}: the two int8 legs differ")
        err = float((out["int8"] - out["fp32"]).abs().max())
        if not err <= max(bags) * 0.1 / 255.0:     # each element is off by at most half a step of its row's range (0.1) / 255
            sys.exit(f"id set {s}: int8 and fp32 gathers differ by {err}")
    print(f"{shape}: {nt} tables, D {D}, batch {batch}, {sum(bags)} lookups per sample ({'uniform' if uniform else 'ragged'} entries), "
          f"{WINDOWS} interleaved windows per leg")
    res = windows_of(legs)
    row_bytes = {"fp32": 4 * D, "bf16": 2 * D, **rb}
    med = {}
    for k in names:
        n, v = res[k]
        med[k] = report(k, f"gather, rows of {row_bytes[k]} bytes", n, v, gather_bytes(batch, bags, D, row_bytes[k]), med.get("fp32"))
    print(f"  bytes by the formula, int8 / fp32: {gather_bytes(batch, bags, D, rb['int8']) / gather_bytes(batch, bags, D, 4 * D):.3f}; "
          f"time at the medians, int8 / fp32: {med['int8'] / med['fp32']:.3f}, int8 / bf16: {med['int8'] / med['bf16']:.3f}, int8/16 / int8: {med['int8/16'] / med['int8']:.3f}")
    qres = windows_of({k: (lambda s, k=k: q8.quantize(src[k], nt, D)) for k in rb})
    for k in rb:
        n, v = qres[k]
        report(k, f"quantize fp32 -> rows of {rb[k]} bytes", n, v, sum(rows) * (4 * D + rb[k]))
    del w32, w16, img, ids, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="both", choices=["terabyte", "mlperf", "both"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", default=None, help="table row counts r-r-... (default: bench.py's MLPerf workload)")
    a = ap.parse_args()
    if a.rows is None:
        import bench as B
        a.rows = B.TERABYTE_ROWS
    rows = [int(x) for x in a.rows.split("-")]
    mlperf = [int(x) for x in MLPERF_BAGS.split("-")]
    if a.shape != "terabyte" and len(rows) != len(mlperf):
        sys.exit(f"--rows has {len(rows)} entries, the MLPerf shape {len(mlperf)} bag sizes")
    import torch
    import _lab
    from dlrm_flexflow_amd import capi
    hip = _lab.load_hip(0)                      # FFH_TOOLS_LIB=<libffhip.so of another build> measures that build
    q8, bags_api, b16 = capi.q8_api(hip), capi.bags_api(hip), capi.bf16_api(hip)
    print(f"device: {torch.cuda.get_device_name(0)}; launches on the null stream, HIP events around each window")
    for shape in (["terabyte", "mlperf"] if a.shape == "both" else [a.shape]):
        bench(hip, q8, bags_api, b16, rows, [1] * len(rows) if shape == "terabyte" else mlperf, a.dim, a.batch, shape)


if __name__ == "__main__":
    main()
