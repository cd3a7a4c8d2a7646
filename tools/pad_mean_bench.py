#!/usr/bin/env python3
"""Timings behind mean pooling over variable-length embedding bags (include/ff_hip_pad_mean.h): the gather and the plain-SGD fused update of one
set of tables, through the C-ABI, at two fills:

  (a) pad, sum          the pad entries of include/ff_hip_pad.h in SUM mode: code the mean forms leave as it was, and their yardstick
  (b) pad, mean         the mean entries on the same ids
  (c) ragged, avg       at fill 1 only: the existing ragged entries with FFH_AGGR_MODE_AVG on the same ids (no pad among them) -- the mean over the
                        L_t slots, which pays the same fp32 division per gradient element and the same scaling in the gather's epilogue, without counts

  python tools/pad_mean_bench.py [--batch B] [--dim D] [--rows r-r-...] [--fills F,F] [--dtype fp32|bf16|both] [--out FILE]

Shape and protocol, as tools/pad_bench.py: the table row counts of bench.py's MLPerf workload, the 26 pooling sizes of the DCNv2 recipe, D = 128,
8192 samples; the legs run INTERLEAVED on one device (seven windows each, every window at least 0.2 s of back-to-back launches between two HIP
events), after every id set of every leg has run once; the launches rotate over four id sets.  The update legs keep adding to the tables: the
timings do not depend on the values.  Before timing, the mean gather is compared bit for bit with the pad gather's sum times
float32(1) / float32(max(count, 1)) formed on the device.  --out appends the report to a file."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pad_bench as PB      # say, window, windows_of: one protocol for both tools

A, Bm, Cr = "(a) pad, sum", "(b) pad, mean", "(c) ragged, avg"


def report(what, fill, res):
    med = {}
    for name, (n, v) in res.items():
        med[name] = float(np.median(v))
        PB.say(f"  {what:7s} fill {fill:<4g} {name:14s} us: {' '.join(f'{u:8.1f}' for u in v)} | median {med[name]:8.1f} | spread {100 * (v.max() - v.min()) / med[name]:4.1f} %   ({n} per window)")
    PB.say(f"  {what:7s} fill {fill:<4g} (b) / (a) = {med[Bm] / med[A]:.3f}" + (f"    (b) / (c) = {med[Bm] / med[Cr]:.3f}" if Cr in med else ""))


def bench(hip, dtype, rows, bags, D, batch, fills):
    import torch
    from dlrm_flexflow_amd import capi
    bags_api, b16, bu, pd, pm = capi.bags_api(hip), capi.bf16_api(hip), capi.bags_update_api(hip), capi.pad_api(hip), capi.pad_mean_api(hip)
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
    out = {k: torch.zeros(batch, ld, device=dev) for k in (A, Bm, Cr)}
    grad = torch.empty(batch, ld, device=dev).uniform_(-1e-3, 1e-3)
    make = b16.tables if bf16 else hip.emb_tables
    dims = bags_api.in_dims(bags)
    SUM, AVG = capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG
    ws_bytes = pm.workspace_bytes(bags, D, batch) + 256
    assert ws_bytes > bu.workspace_bytes(bags, D, batch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    hip.set_workspace(ws, ws_bytes)
    rnd = b16.rounding(capi.BF16_ROUND_NEAREST) if bf16 else None
    for fill in fills:
        ids = []
        for s in range(PB.NSETS):
            p = []
            for t, (R, L) in enumerate(zip(rows, bags)):
                i = torch.empty(batch * L, dtype=torch.int64, device=dev)
                hip.call("ffh_gen_indices", i, batch * L, (0x9E3779B97F4A7C15 * (s + 1) + t) & (2**64 - 1), 0, R, None)
                pd.mask(i, batch * L, 1000 * s + t, 0, fill)
                p.append(i)
            ids.append(p)
        tabs = lambda s, io: make([(ids[s][t], W[t], io.data_ptr() + 4 * D * t, rows[t], ld) for t in range(nt)])
        legs = (A, Bm, Cr) if fill >= 1.0 else (A, Bm)
        fwd_arr = {k: [tabs(s, out[k]) for s in range(PB.NSETS)] for k in legs}
        plain_fwd = "ffh_embedding_fwd_multi_bags_bf16" if bf16 else "ffh_embedding_fwd_multi_bags"
        gather = {A: lambda s: pd.fwd(fwd_arr[A][s], dims, nt, D, batch, SUM, bf16=bf16),
                  Bm: lambda s: pm.fwd(fwd_arr[Bm][s], dims, nt, D, batch, AVG, bf16=bf16)}
        if Cr in legs:
            gather[Cr] = lambda s: bags_api.call(plain_fwd, fwd_arr[Cr][s], dims, nt, D, batch, AVG)
        for s in range(PB.NSETS):
            for fn in gather.values():
                fn(s)
            torch.cuda.synchronize()
            for t, L in enumerate(bags):      # identity 2 of the header, on the device: one fp32 reciprocal, one fp32 multiply
                cnt = (ids[s][t].view(batch, L) >= 0).sum(1).clamp(min=1).to(torch.float32)
                want = out[A][:, t * D:(t + 1) * D] * (1.0 / cnt)[:, None]
                if not want.view(torch.int32).equal(out[Bm][:, t * D:(t + 1) * D].view(torch.int32)):
                    sys.exit(f"fill {fill}, id set {s}, table {t}: the mean gather is not the pad gather's sum times 1 / max(count, 1)")
            if Cr in legs and not out[Cr].view(torch.int32).equal(out[Bm].view(torch.int32)):
                sys.exit(f"fill {fill}, id set {s}: without pads the mean gather is not the ragged AVG gather")
        desc = {k: [capi.BagsUpdateApi.descriptor(in_dims=bags, out_dim=D, batch=batch, aggr=SUM if k == A else AVG, lr=1e-3, rounding=rnd,
                                                  **{"tables_bf16" if bf16 else "tables": tabs(s, grad)}) for s in range(PB.NSETS)] for k in legs}
        update = {A: lambda s: pd.fused(desc[A][s]), Bm: lambda s: pm.fused(desc[Bm][s])}
        if Cr in legs:
            update[Cr] = lambda s: bu.call(desc[Cr][s])
        for s in range(PB.NSETS):
            for fn in update.values():
                fn(s)
        torch.cuda.synchronize()
        npad = sum(int((m < 0).sum()) for m in ids[0])
        PB.say(f"{dtype} rows: {nt} tables, D {D}, batch {batch}, {sum(bags)} slots per sample, fill {fill} ({npad / (batch * sum(bags)):.3f} of set 0's slots are pads), "
               f"{PB.WINDOWS} interleaved windows per leg")
        report("gather", fill, PB.windows_of(gather))
        report("update", fill, PB.windows_of(update))
        del ids, fwd_arr, desc
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
