#!/usr/bin/env python3
"""Adagrad (include/ff_hip_adagrad.h) beside the rules it shares a path with: the fused table update under plain SGD, momentum SGD, Adagrad and
row-wise Adagrad (include/ff_hip_rowwise.h) on fp32 and bf16 tables, the dense launch on the Terabyte shape's MLP slab, and the driver's whole
step on the Terabyte shape under --optimizer adagrad with and without --adagrad-rowwise.  HIP events on the launch stream (the step: wall clock
around a synchronised run of steps).

  python tools/adagrad_bench.py [terabyte-26] [4x32768] [26x4096] [dense] [step] [--out profiles/adagrad_measurements.txt]

Algorithmic bytes per table update (e = 4 or 2 bytes per table element, s = state rows per touched row: 0 plain SGD, 1 momentum / Adagrad):
  B*(8 + 4D + 2*e*D + s*2*4*D)      ids, gradient rows, each looked-up row and its state row read and written once
  row-wise Adagrad: s = 0 and 8 more bytes per row (the row's one float read and written)
reported as a fraction of 8 TB/s.  Momentum and Adagrad move the same bytes: momentum's time in the same run is Adagrad's yardstick, and
Adagrad's is row-wise Adagrad's.  Every table figure is the median of three timings of 20 calls; "spread" is (max - min) / median of the three.
"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dlrm_flexflow_amd import capi

DEV = "cuda:0"
PEAK_HBM = 8.0e12
TERABYTE_ROWS = [39884406, 39043, 17289, 7420, 20263, 3, 7120, 1543, 63, 38532951, 2953546, 403346, 10, 2208, 11938, 155, 4, 976, 14,
                 39979771, 25641295, 39664984, 585935, 12972, 108, 36]
CASES = [("terabyte-26", 32768, 128, TERABYTE_ROWS),
         ("4x32768", 32768, 128, [32768] * 4),
         ("26x4096", 32768, 128, [4096] * 26)]
# bottom 13-512-256-128 and top 479-1024-1024-512-256-1 of the Terabyte (MLPerf) shape, weights + biases
SLAB = sum(a * b + b for a, b in zip([13, 512, 256, 479, 1024, 1024, 512, 256], [512, 256, 128, 1024, 1024, 512, 256, 1]))
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


def opt_of(kind):
    o = capi.SparseOpt()
    o.kind, o.lr, o.epsilon = kind, 1e-6, 1e-10
    o.momentum = 0.9 if kind == capi.SPARSE_OPT_SGD_MOMENTUM else 0.0
    return o


def tables(hip, b16, name, B, D, rows, dtype):
    T = len(rows)
    e = 2 if dtype == "bf16" else 4
    W, I, S = [], [], []
    for t, R in enumerate(rows):
        if dtype == "bf16":
            w = torch.empty(R, D, dtype=torch.int16, device=DEV)
            b16.call("ffh_init_uniform_bf16", w, R * D, t, -0.01, 0.01, None)
        else:
            w = torch.empty(R, D, device=DEV)
            hip.call("ffh_init_uniform", w, R * D, t, -0.01, 0.01, None)
        i = torch.empty(B, 1, dtype=torch.int64, device=DEV)
        hip.call("ffh_gen_indices", i, B, 100 + t, 0, R, None)
        W.append(w); I.append(i); S.append(torch.zeros(R, D, device=DEV))      # one state buffer: momentum's V, then Adagrad's S
    Srow = [torch.zeros(R, device=DEV) for R in rows]                          # row-wise Adagrad's: one float per row
    ld = T * D
    G = torch.empty(B, ld, device=DEV)
    hip.call("ffh_gen_uniform01", G, G.numel(), 5, 0, None)
    ws = torch.empty(hip.lib.ffh_embedding_bwd_workspace_bytes(T, 1, D, B) + 256, dtype=torch.uint8, device=DEV)
    hip.set_workspace(ws, ws.numel())
    st_full, st_row = hip.emb_states([(S[t], None) for t in range(T)]), hip.emb_states([(Srow[t], None) for t in range(T)])
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    rnd = b16.rounding(capi.BF16_ROUND_STOCHASTIC, 1, counter)
    out = {}
    for rule, kind, s in (("sgd", capi.SPARSE_OPT_SGD, 0), ("momentum", capi.SPARSE_OPT_SGD_MOMENTUM, 1), ("adagrad", capi.SPARSE_OPT_ADAGRAD, 1),
                          ("rowwise", capi.SPARSE_OPT_ROWWISE_ADAGRAD, 0)):
        opt = opt_of(kind)
        st = st_row if rule == "rowwise" else st_full
        if dtype == "bf16":
            ba = b16.tables([(I[t], W[t], G[:, t * D:], rows[t], ld) for t in range(T)])
            per = 32 if kind == capi.SPARSE_OPT_SGD_MOMENTUM else 64      # FFH_BF16_MAX_STATEFUL_TABLES is momentum's limit, not Adagrad's

            def step():
                for b in range(0, T, per):
                    n = min(per, T - b)
                    part = ctypes.cast(ctypes.byref(ba, b * ctypes.sizeof(capi.EmbTableBf16)), ctypes.POINTER(capi.EmbTableBf16))
                    sp = ctypes.cast(ctypes.byref(st, b * ctypes.sizeof(capi.EmbState)), ctypes.POINTER(capi.EmbState))
                    hip.check(b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(hip.ctx, part, sp, n, 1, D, B, capi.AGGR_MODE_SUM, ctypes.byref(opt),
                                                                            ctypes.byref(rnd), None), "b16")
                hip.check(b16.lib.ffh_bf16_counter_advance(hip.ctx, capi.ptr(counter), None), "c")
        else:
            ba = hip.emb_tables([(I[t], W[t], G[:, t * D:], rows[t], ld) for t in range(T)])
            step = lambda: hip.check(hip.lib.ffh_embedding_bwd_opt_fused_multi(hip.ctx, ba, st, T, 1, D, B, capi.AGGR_MODE_SUM, ctypes.byref(opt), None), "b")
        ts = sorted(timeit(step) for _ in range(3))
        t = ts[1]
        bytes_ = T * B * (8 + 4 * D + 2 * e * D + s * 8 * D + (8 if rule == "rowwise" else 0))
        out[rule] = t
        say(f"{name:12s} {dtype:5s} {rule:9s} fused update {t*1e6:8.1f} us (spread {(ts[2]-ts[0])/t:5.3f}; {bytes_/t/PEAK_HBM:5.3f} of 8 TB/s, "
            f"route {hip.lib.ffh_embedding_last_route(hip.ctx).decode()})")
    say(f"{name:12s} {dtype:5s} adagrad / momentum time {out['adagrad']/out['momentum']:.3f}   adagrad / sgd {out['adagrad']/out['sgd']:.3f}   "
        f"accumulator {sum(rows)*D*4/1e9:.2f} GB beside {sum(rows)*D*e/1e9:.2f} GB of tables")
    say(f"{name:12s} {dtype:5s} rowwise / adagrad time {out['rowwise']/out['adagrad']:.3f}   rowwise / sgd {out['rowwise']/out['sgd']:.3f}   "
        f"accumulator {sum(rows)*4/1e9:.3f} GB beside {sum(rows)*D*e/1e9:.2f} GB of tables")
    del W, I, S, Srow, G, ws
    torch.cuda.empty_cache()


def dense(hip, ag):
    n = SLAB // 4 * 4
    w, g, s, v = (torch.zeros(n, device=DEV) for _ in range(4))
    hip.call("ffh_init_uniform", w, n, 1, -0.1, 0.1, None)
    hip.call("ffh_gen_uniform01", g, n, 2, 0, None)
    res = {
        "sgd": (timeit(lambda: hip.call("ffh_sgd_update_ex", w, g, None, n, 1e-6, 0.0, 0.0, 0, 0, None), 200, 20), 12),
        "adam": (timeit(lambda: hip.call("ffh_adam_update", w, g, s, v, n, 1e-6, 0.9, 0.999, 0.0, 1e-8, 0, None), 200, 20), 28),
        "adagrad": (timeit(lambda: ag.call("ffh_adagrad_update", w, g, s, n, 1e-6, 1e-10, 0.0, 0, None), 200, 20), 20),
    }
    for k, (t, b) in res.items():
        say(f"dense slab   n={n} {k:8s} {t*1e6:7.2f} us ({b*n/t/PEAK_HBM:5.3f} of 8 TB/s at {b} bytes per element; the slab fits the caches)")


def whole_step():
    """The driver's model at the Terabyte shape (the flagship workload of bench.py: 26 tables x 128, batch 32768, concat interaction) for 3 x 20 steps
    behind the warm-up step, element-wise and row-wise, fp32 and bf16 tables; the start-up line gives the accumulator's bytes."""
    from dlrm_flexflow_amd import ffmodel
    flags = ["-b", "32768", "--arch-sparse-feature-size", "128", "--arch-embedding-size", "-".join(map(str, TERABYTE_ROWS)), "--arch-mlp-bot",
             "13-512-256-128", "--arch-mlp-top", "3456-1024-1024-512-256-1", "--data-size", "32768", "--optimizer", "adagrad"]
    for dtype in ("fp32", "bf16"):
        res = {}
        for rule, extra in (("adagrad", []), ("rowwise", ["--adagrad-rowwise"])):
            app = ffmodel.DLRM(flags + extra + (["--embedding-dtype", "bf16"] if dtype == "bf16" else []))
            try:
                app.warmup()
                app.train_steps(5)
                app.model.sync()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    app.train_steps(20)
                    app.model.sync()
                    ts.append((time.perf_counter() - t0) / 20)
                ts.sort()
                res[rule] = ts[1]
                say(f"step terabyte {dtype:5s} {rule:9s} {ts[1]*1e3:7.3f} ms per step (spread {(ts[2]-ts[0])/ts[1]:5.3f}), {32768/ts[1]:9.0f} samples/s")
            finally:
                app.close()
        say(f"step terabyte {dtype:5s} rowwise / adagrad time {res['rowwise']/res['adagrad']:.3f}")


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        args = [a for a in args if a not in ("--out", out)]
    hip = capi.load_hip(0)
    b16, ag = capi.bf16_api(hip), capi.adagrad_api(hip)
    say(f"{hip.device_info().name.decode()} {hip.device_info().compute_units} CUs; tools/adagrad_bench.py {' '.join(args)}".rstrip())
    for name, B, D, rows in CASES:
        if args and name not in args:
            continue
        for dtype in ("fp32", "bf16"):
            tables(hip, b16, name, B, D, rows, dtype)
    if not args or "dense" in args:
        dense(hip, ag)
    if not args or "step" in args:
        whole_step()
    if out:
        with open(out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
