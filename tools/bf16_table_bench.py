#!/usr/bin/env python3
"""fp32 vs bf16 embedding tables (include/ff_hip_bf16.h): the gather and the fused plain-SGD update alone, HIP events on the
launch stream, at three shapes.

  python tools/bf16_table_bench.py [terabyte-26] [terabyte-rank-of-8] [kaggle-26]

Algorithmic bytes per table (SURVEY.md 8(d) with the table element size e = 4 or 2):
  gather   B*(L*(8+e*D)+4D)        ids, table rows, output rows
  update   B*(8L+4D+L*2*e*D)       ids, gradient rows, each looked-up row read and written once
reported as a fraction of 8 TB/s.  The bf16 update uses stochastic rounding (the default), the counter advanced once per call.
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dlrm_flexflow_amd import capi

DEV = "cuda:0"
PEAK_HBM = 8.0e12
TERABYTE_ROWS = [39884406, 39043, 17289, 7420, 20263, 3, 7120, 1543, 63, 38532951, 2953546, 403346, 10, 2208, 11938, 155, 4, 976, 14,
                 39979771, 25641295, 39664984, 585935, 12972, 108, 36]
KAGGLE_ROWS = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10, 5652, 2173, 4,
               7046547, 18, 15, 286181, 105, 142572]
CASES = [("terabyte-26", 32768, 128, TERABYTE_ROWS),
         ("terabyte-rank-of-8", 32768, 128, [39884406, 39043, 38532951, 2953546]),
         ("kaggle-26", 2048, 16, KAGGLE_ROWS)]


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def run(hip, b16, name, B, D, rows, dtype):
    T = len(rows)
    e = 2 if dtype == "bf16" else 4
    W, I = [], []
    for t, R in enumerate(rows):
        if dtype == "bf16":
            w = torch.empty(R, D, dtype=torch.int16, device=DEV)
            b16.call("ffh_init_uniform_bf16", w, R * D, t, -0.01, 0.01, None)
        else:
            w = torch.empty(R, D, device=DEV)
            hip.call("ffh_init_uniform", w, R * D, t, -0.01, 0.01, None)
        i = torch.empty(B, 1, dtype=torch.int64, device=DEV)
        hip.call("ffh_gen_indices", i, B, 100 + t, 0, R, None)
        W.append(w); I.append(i)
    ld = T * D
    Z = torch.empty(B, ld, device=DEV)
    G = torch.empty(B, ld, device=DEV)
    hip.call("ffh_gen_uniform01", G, G.numel(), 5, 0, None)
    ws = torch.empty(hip.lib.ffh_embedding_bwd_workspace_bytes(T, 1, D, B) + 256, dtype=torch.uint8, device=DEV)
    hip.set_workspace(ws, ws.numel())
    if dtype == "bf16":
        counter = torch.zeros(1, dtype=torch.int64, device=DEV)
        rnd = b16.rounding(capi.BF16_ROUND_STOCHASTIC, 1, counter)
        fa = b16.tables([(I[t], W[t], Z[:, t * D:], rows[t], ld) for t in range(T)])
        ba = b16.tables([(I[t], W[t], G[:, t * D:], rows[t], ld) for t in range(T)])
        fwd = lambda: hip.check(b16.lib.ffh_embedding_fwd_multi_bf16(hip.ctx, fa, T, 1, D, B, capi.AGGR_MODE_SUM, None), "f")

        def bwd():
            hip.check(b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(hip.ctx, ba, T, 1, D, B, capi.AGGR_MODE_SUM, 1e-6, ctypes.byref(rnd), None), "b")
            hip.check(b16.lib.ffh_bf16_counter_advance(hip.ctx, capi.ptr(counter), None), "c")
    else:
        fa = hip.emb_tables([(I[t], W[t], Z[:, t * D:], rows[t], ld) for t in range(T)])
        ba = hip.emb_tables([(I[t], W[t], G[:, t * D:], rows[t], ld) for t in range(T)])
        fwd = lambda: hip.check(hip.lib.ffh_embedding_fwd_multi(hip.ctx, fa, T, 1, D, B, capi.AGGR_MODE_SUM, None), "f")
        bwd = lambda: hip.check(hip.lib.ffh_embedding_bwd_sgd_fused_multi(hip.ctx, ba, T, 1, D, B, capi.AGGR_MODE_SUM, 1e-6, None), "b")
    tf, tb = timeit(fwd), timeit(bwd)
    bf = T * B * (8 + e * D + 4 * D)
    bb = T * B * (8 + 4 * D + 2 * e * D)
    table_gb = sum(rows) * D * e / 1e9
    print(f"{name:20s} {dtype:5s} tables {table_gb:7.2f} GB | gather {tf*1e6:8.1f} us ({bf/tf/PEAK_HBM:5.3f} of 8 TB/s) | "
          f"fused update {tb*1e6:8.1f} us ({bb/tb/PEAK_HBM:5.3f})", flush=True)
    del W, I, Z, G, ws
    torch.cuda.empty_cache()
    return tf, tb


def main():
    hip = capi.load_hip(0)
    b16 = capi.bf16_api(hip)
    only = sys.argv[1:]
    print(hip.device_info().name.decode(), hip.device_info().compute_units, "CUs")
    for name, B, D, rows in CASES:
        if only and name not in only:
            continue
        f32 = run(hip, b16, name, B, D, rows, "fp32")
        h16 = run(hip, b16, name, B, D, rows, "bf16")
        print(f"{name:20s} bf16 / fp32 time: gather {h16[0]/f32[0]:.3f}  fused update {h16[1]/f32[1]:.3f}", flush=True)


if __name__ == "__main__":
    main()
