#!/usr/bin/env python3
"""Timings behind DESIGN section 19 (per-table embedding bag sizes): the gather of a model of mixed bag sizes, through the C-ABI, two ways:

  (a) ragged      ffh_embedding_fwd_multi_bags[_bf16] (include/ff_hip_bags.h): every table in ONE launch
  (b) per size    ffh_embedding_fwd_multi[_bf16] once per distinct bag size over the tables of that size: the only way without the extension,
                  and the baseline

  python tools/bags_bench.py [--bag-sizes a-b-c-...] [--batch B] [--dtype fp32|bf16|both] [--rows r-r-...] [--dim D]

Defaults: the MLPerf DLRM-DCNv2 shape -- the 26 pooling sizes 3-2-1-2-6-1-1-1-1-7-3-8-1-6-9-5-1-1-1-12-100-27-10-3-1-1, 8192 samples, D = 128, the
table row counts of bench.py's MLPerf workload -- for fp32 and for bf16 tables.  The two legs run INTERLEAVED on one device (window a, window b,
window a, ...: seven windows each, every window at least 0.2 s of back-to-back launches on one stream between two HIP events), after every id set
of both legs has run once.  The launches rotate over four id sets drawn with their own seeds, so that a launch does not find the rows of the one
before in the Infinity Cache.  Each leg is also priced as a fraction of the HBM rate (8 TB/s) by the algorithmic bytes of DESIGN section 3.1,
summed over the tables: batch * (L_t * (8 + w * D) + 4 * D) with w = 4 (fp32) or 2 (bf16) bytes per element.  Before timing, the two legs'
outputs are compared bit for bit."""
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


def algorithmic_bytes(batch, bags, D, wbytes):
    return sum(batch * (L * (8 + wbytes * D) + 4 * D) for L in bags)


def window(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i % NSETS)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench(hip, bags_api, b16, rows, bags, D, batch, bf16):
    import torch
    from dlrm_flexflow_amd import capi
    dev, nt = "cuda:0", len(bags)
    wbytes = 2 if bf16 else 4
    tables = []
    for t, R in enumerate(rows):
        if bf16:
            w = torch.empty(R * D, dtype=torch.int16, device=dev)
            b16.call("ffh_init_uniform_bf16", w, R * D, 100 + t, -0.05, 0.05, None)
        else:
            w = torch.empty(R * D, dtype=torch.float32, device=dev)
            hip.call("ffh_init_uniform", w, R * D, 100 + t, -0.05, 0.05, None)
        tables.append(w)
    ids = []
    for s in range(NSETS):
        per = []
        for t, (R, L) in enumerate(zip(rows, bags)):
            i = torch.empty(batch * L, dtype=torch.int64, device=dev)
            hip.call("ffh_gen_indices", i, batch * L, (0x9E3779B97F4A7C15 * (s + 1) + t) & (2**64 - 1), 0, R, None)
            per.append(i)
        ids.append(per)
    ld = nt * D
    out = {"a": torch.zeros(batch, ld, device=dev), "b": torch.zeros(batch, ld, device=dev)}
    make = (lambda e: b16.tables(e)) if bf16 else (lambda e: hip.emb_tables(e))
    entry = lambda leg, s, t: (ids[s][t], tables[t], out[leg].data_ptr() + 4 * D * t, rows[t], ld)
    dims = bags_api.in_dims(bags)
    ragged = [make([entry("a", s, t) for t in range(nt)]) for s in range(NSETS)]
    sizes = sorted(set(bags))
    split = [[(L, [t for t in range(nt) if bags[t] == L]) for L in sizes] for _ in range(NSETS)]
    split = [[(L, len(sel), make([entry("b", s, t) for t in sel])) for L, sel in split[s]] for s in range(NSETS)]
    name_a = "ffh_embedding_fwd_multi_bags_bf16" if bf16 else "ffh_embedding_fwd_multi_bags"
    fn_b = b16.lib.ffh_embedding_fwd_multi_bf16 if bf16 else hip.lib.ffh_embedding_fwd_multi

    def leg_a(s):
        bags_api.call(name_a, ragged[s], dims, nt, D, batch, capi.AGGR_MODE_SUM)

    def leg_b(s):
        for L, n, arr in split[s]:
            hip.check(fn_b(hip.ctx, arr, n, L, D, batch, capi.AGGR_MODE_SUM, None), "ffh_embedding_fwd_multi")

    for s in range(NSETS):                      # every id set of both legs once: code objects loaded, pages touched; and the same bits
        leg_a(s); leg_b(s)
        torch.cuda.synchronize()
        if not out["a"].view(torch.int32).equal(out["b"].view(torch.int32)):
            sys.exit(f"id set {s}: the ragged gather and the gather per bag size differ")
    n = 16
    while True:                                 # size the windows on the slower leg
        us = max(window(leg_a, n), window(leg_b, n))
        if us * n >= MIN_SECONDS * 1e6:
            break
        n = int(n * max(2.0, 1.2 * MIN_SECONDS * 1e6 / (us * n)))
    t = {"a": [], "b": []}
    for _ in range(WINDOWS):
        t["a"].append(window(leg_a, n))
        t["b"].append(window(leg_b, n))
    nbytes = algorithmic_bytes(batch, bags, D, wbytes)
    kind = "bf16" if bf16 else "fp32"
    print(f"{kind} tables: {nt} tables, D {D}, batch {batch}, {sum(bags)} lookups per sample, {nbytes / 1e6:.1f} MB per gather by the formula; "
          f"{n} gathers per window, {WINDOWS} interleaved windows per leg; outputs of the two legs: same bits")
    for leg, what in (("a", "(a) ragged, 1 launch"), ("b", f"(b) per bag size, {len(sizes)} launches")):
        v = np.array(t[leg])
        print(f"  {what:32s} us per gather: {' '.join(f'{u:7.1f}' for u in v)} | min {v.min():7.1f} median {np.median(v):7.1f} max {v.max():7.1f} "
              f"| spread {100 * (v.max() - v.min()) / np.median(v):4.1f} % | {nbytes / np.median(v) / 1e6 / (HBM_PEAK / 1e12):.3f} of 8 TB/s at the median", flush=True)
    ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
    print(f"  (a) / (b) at the medians: {ma / mb:.3f}")
    del tables, ids, out
    torch.cuda.empty_cache()
    return ma, mb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bag-sizes", default=MLPERF_BAGS, help="one bag size per table, a-b-c-...")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", default=None, help="table row counts r-r-... (default: bench.py's MLPerf workload)")
    ap.add_argument("--dtype", default="both", choices=["fp32", "bf16", "both"])
    a = ap.parse_args()
    bags = [int(x) for x in a.bag_sizes.split("-")]
    if a.rows is None:
        import bench as B
        a.rows = B.TERABYTE_ROWS
    rows = [int(x) for x in a.rows.split("-")]
    if len(rows) != len(bags) or min(bags) < 1:
        sys.exit(f"--bag-sizes has {len(bags)} entries for {len(rows)} tables (--rows), each >= 1")
    import torch
    import _lab
    from dlrm_flexflow_amd import capi
    hip = _lab.load_hip(0)                      # FFH_TOOLS_LIB=<libffhip.so of another build> measures that build
    bags_api, b16 = capi.bags_api(hip), capi.bf16_api(hip)
    print(f"device: {torch.cuda.get_device_name(0)}; launches on the null stream, HIP events around each window")
    for bf16 in ([False, True] if a.dtype == "both" else [a.dtype == "bf16"]):
        bench(hip, bags_api, b16, rows, bags, a.dim, a.batch, bf16)


if __name__ == "__main__":
    main()
