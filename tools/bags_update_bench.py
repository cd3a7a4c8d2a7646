#!/usr/bin/env python3
"""Timings behind DESIGN section 19 (per-table embedding bag sizes): the fused table update of a model of mixed bag sizes, through the C-ABI, two ways:

  (a) ragged      ffh_embedding_bwd_fused_multi_bags (include/ff_hip_bags_update.h): every table in ONE call
  (b) per size    ffh_embedding_bwd_{sgd,opt}_fused_multi[_bf16] once per distinct bag size over the tables of that size: what --no-ragged-update
                  runs, the only way without the extension, and the baseline

  python tools/bags_update_bench.py [--bag-sizes a-b-c-...] [--batch B] [--dtype fp32|bf16|both] [--rule sgd|rowwise|both] [--rows r-r-...] [--dim D]
                                    [--legs update|pair|both]

Defaults: the MLPerf DLRM-DCNv2 shape -- the 26 pooling sizes 3-2-1-2-6-1-1-1-1-7-3-8-1-6-9-5-1-1-1-12-100-27-10-3-1-1, 8192 samples, D = 128, the
table row counts of bench.py's MLPerf workload -- for fp32 and for bf16 tables (stochastic rounding, the update counter held still), plain SGD and
row-wise Adagrad.  The two legs run INTERLEAVED on one device (window a, window b, window a, ...: seven windows each, every window at least 0.2 s of
back-to-back updates on one stream between two HIP events), after every id set of both legs has run once.  The updates rotate over four id sets
drawn with their own seeds.  Each leg is also priced as a fraction of the HBM rate (8 TB/s) by the algorithmic bytes of DESIGN section 3.2, summed
over the tables: batch * (8 L_t + 4 D + L_t * 2 * w * D) with w = 4 (fp32) or 2 (bf16) bytes per element.  The launches of one update are counted
off the route every call reports (ffh_embedding_last_route: one-launch form 1, bucket form 3, LSD form 2 passes + 1).

Before any timing the two legs are compared bit for bit: from the same start (the tables are re-initialised from their seeds in between) each leg
runs one update per id set; after each, the rows the update touched (and their optimizer state) are read back, and a wrapping 64-bit sum over
every table's bits covers the rows it did not.

The pair leg (--legs pair | both; include/ff_hip_bags_sort.h) says how much of the ragged call an early sort can move off the step's serial chain:
  (s) sort     ffh_embedding_bwd_sort_multi_bags alone: the index-only part
  (p) apply    ffh_embedding_bwd_apply_multi_bags alone: what stays behind the output gradients
  (f) fused    ffh_embedding_bwd_fused_multi_bags, timed the same way
An apply needs a sort of its own (the pair is one-shot), so this leg cannot run applies back to back: every CALL sits between two HIP events of its
own ([e0] sort [e1] apply [e2], and [e0] fused [e1]) and a window's figure is the mean over its calls.  Windows of sort + apply and windows of the
fused call alternate; the pair is first compared with the fused call bit for bit, as above.  The per-call events leave the launch gaps in, so (f)
here reads higher than (a) above; (s) + (p) against (f) is the comparison."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bags_helpers  # noqa: E402  (tests/bags_helpers.py: the one list of the 26 MLPerf bag sizes)

MLPERF_BAGS = "-".join(map(str, bags_helpers.MLPERF_BAGS))
HBM_PEAK = 8.0e12
NSETS, WINDOWS, MIN_SECONDS = 4, 7, 0.2
LR, EPS, ACC0 = 0.01, 1e-10, 0.1


def algorithmic_bytes(batch, bags, D, wbytes):
    return sum(batch * (8 * L + 4 * D + L * 2 * wbytes * D) for L in bags)


def launches_of(route):
    if route.endswith("small"):
        return 1
    if "buckets" in route:
        return 3
    return 2 * int(re.search(r"passes=(\d+)", route).group(1)) + 1


def window(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i % NSETS)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench(hip, bu, b16, rows, bags, D, batch, bf16, rule, legs="update", bs=None):
    import torch
    from dlrm_flexflow_amd import capi
    dev, nt = "cuda:0", len(bags)
    wbytes = 2 if bf16 else 4
    rowwise = rule == "rowwise"
    tables = [torch.empty(R * D, dtype=torch.int16 if bf16 else torch.float32, device=dev) for R in rows]
    state = [torch.empty(R, dtype=torch.float32, device=dev) if rowwise else None for R in rows]

    def reset():
        for t, R in enumerate(rows):
            if bf16:
                b16.call("ffh_init_uniform_bf16", tables[t], R * D, 100 + t, -0.05, 0.05, None)
            else:
                hip.call("ffh_init_uniform", tables[t], R * D, 100 + t, -0.05, 0.05, None)
            if rowwise:
                state[t].fill_(ACC0)

    ids = []
    for s in range(NSETS):
        per = []
        for t, (R, L) in enumerate(zip(rows, bags)):
            i = torch.empty(batch * L, dtype=torch.int64, device=dev)
            hip.call("ffh_gen_indices", i, batch * L, (0x9E3779B97F4A7C15 * (s + 1) + t) & (2**64 - 1), 0, R, None)
            per.append(i)
        ids.append(per)
    ld = nt * D
    g = torch.randn(batch, ld, device=dev) * 0.01
    counter = torch.tensor([5], dtype=torch.int64, device=dev)
    rnd = b16.rounding(capi.BF16_ROUND_STOCHASTIC, 0xBA65, counter)
    opt = capi.SparseOpt()
    opt.kind, opt.lr, opt.epsilon = capi.SPARSE_OPT_ROWWISE_ADAGRAD, LR, EPS
    make = (lambda e: b16.tables(e)) if bf16 else (lambda e: hip.emb_tables(e))
    entry = lambda s, t: (ids[s][t], tables[t], g.data_ptr() + 4 * D * t, rows[t], ld) + ((t, 0) if bf16 else ())
    states = lambda sel: hip.emb_states([(state[t], None) for t in sel])
    sizes = sorted(set(bags))
    groups = [[t for t in range(nt) if bags[t] == L] for L in sizes]
    ragged = []
    for s in range(NSETS):
        kw = dict(in_dims=bags, out_dim=D, batch=batch, aggr=capi.AGGR_MODE_SUM, lr=LR)
        kw["tables_bf16" if bf16 else "tables"] = make([entry(s, t) for t in range(nt)])
        if bf16:
            kw["rounding"] = rnd
        if rowwise:
            kw["opt"], kw["states"] = opt, states(range(nt))
        ragged.append(bu.descriptor(**kw))
    split = [[(L, len(sel), make([entry(s, t) for t in sel]), states(sel)) for L, sel in zip(sizes, groups)] for s in range(NSETS)]
    need = max([bu.workspace_bytes(bags, D, batch)] + [int(hip.lib.ffh_embedding_bwd_workspace_bytes(len(sel), L, D, batch)) for L, sel in zip(sizes, groups)]) + 256
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    hip.set_workspace(ws, need)
    route = lambda: hip.lib.ffh_embedding_last_route(hip.ctx).decode()
    seen = {"a": [], "b": []}

    def leg_a(s, note=False):
        bu.call(ragged[s])
        if note:
            seen["a"].append(route())

    def leg_b(s, note=False):
        for L, n, arr, st in split[s]:
            if bf16 and rowwise:
                rc = b16.lib.ffh_embedding_bwd_opt_fused_multi_bf16(b16.ctx, arr, st, n, L, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), C.byref(rnd), None)
            elif bf16:
                rc = b16.lib.ffh_embedding_bwd_sgd_fused_multi_bf16(b16.ctx, arr, n, L, D, batch, capi.AGGR_MODE_SUM, LR, C.byref(rnd), None)
            elif rowwise:
                rc = hip.lib.ffh_embedding_bwd_opt_fused_multi(hip.ctx, arr, st, n, L, D, batch, capi.AGGR_MODE_SUM, C.byref(opt), None)
            else:
                rc = hip.lib.ffh_embedding_bwd_sgd_fused_multi(hip.ctx, arr, n, L, D, batch, capi.AGGR_MODE_SUM, LR, None)
            hip.check(rc, "the update per bag size")
            if note:
                seen["b"].append(route())

    # the same bits, before any timing: NSETS updates in a row from the same start on each leg
    def snapshot(leg):
        reset()
        out = []
        for s in range(NSETS):
            leg(s, note=(s == 0))
            for t in range(nt):
                out.append(tables[t].view(-1, D)[ids[s][t]].clone())
                if rowwise:
                    out.append(state[t][ids[s][t]].clone())
        for t in range(nt):
            out.append(tables[t].view(torch.int16 if bf16 else torch.int32).sum(dtype=torch.int64).reshape(1))
            if rowwise:
                out.append(state[t].view(torch.int32).sum(dtype=torch.int64).reshape(1))
        torch.cuda.synchronize()
        return out
    kind = ("bf16" if bf16 else "fp32") + " tables, " + ("row-wise Adagrad" if rowwise else "plain SGD")
    nbytes = algorithmic_bytes(batch, bags, D, wbytes)
    if legs != "update":
        def leg_pair(s, note=False):
            bs.sort(ragged[s])
            bs.apply(ragged[s])
        sa, sp = snapshot(leg_a), snapshot(leg_pair)
        for k, (x, y) in enumerate(zip(sa, sp)):
            if not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
                sys.exit(f"record {k}: sort + apply and the fused ragged call differ")
        del sa, sp

        def timed(calls, n):
            """n rounds of `calls` (each between two events of its own); the mean microseconds of every call"""
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)] for _ in range(n)]
            for i in range(n):
                ev[i][0].record()
                for k, fn in enumerate(calls):
                    fn(ragged[i % NSETS])
                    ev[i][k + 1].record()
            torch.cuda.synchronize()
            return [sum(ev[i][k].elapsed_time(ev[i][k + 1]) for i in range(n)) * 1e3 / n for k in range(len(calls))]
        n = 8
        while True:
            us = timed([bu.call], n)[0]
            if us * n >= MIN_SECONDS * 1e6:
                break
            n = int(n * max(2.0, 1.2 * MIN_SECONDS * 1e6 / (us * n)))
        t = {"s": [], "p": [], "f": []}
        for _ in range(WINDOWS):
            a, b = timed([bs.sort, bs.apply], n)
            t["s"].append(a); t["p"].append(b)
            t["f"].append(timed([bu.call], n)[0])
        print(f"{kind}: {nt} tables, D {D}, batch {batch}, {sum(bags)} lookups per sample; the pair leg: {n} calls per window, {WINDOWS} interleaved windows, "
              f"every call between two events of its own; sort + apply leave the fused call's bits; route {seen['a'][0]}")
        t["s+p"] = [x + y for x, y in zip(t["s"], t["p"])]
        for leg, what in (("s", "(s) sort call alone"), ("p", "(p) apply call alone"), ("s+p", "(s) + (p), window by window"), ("f", "(f) fused call")):
            v = np.array(t[leg])
            print(f"  {what:44s} us per call:   {' '.join(f'{u:7.1f}' for u in v)} | min {v.min():7.1f} median {np.median(v):7.1f} max {v.max():7.1f} "
                  f"| spread {100 * (v.max() - v.min()) / np.median(v):4.1f} %", flush=True)
        ms, mp, mf = (float(np.median(t[k])) for k in ("s", "p", "f"))
        print(f"  the sort is {ms / mf:.3f} of the fused call at the medians: what an early sort can move; (s) + (p) - (f) = {ms + mp - mf:+.1f} us "
              f"(the fused call's window spread: {max(t['f']) - min(t['f']):.1f} us)", flush=True)
    if legs == "pair":
        del tables, ids, g, ws, state
        torch.cuda.empty_cache()
        return None
    seen["a"].clear()
    sa, sb = snapshot(leg_a), snapshot(leg_b)
    for k, (x, y) in enumerate(zip(sa, sb)):
        if not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            sys.exit(f"record {k}: the ragged update and the update per bag size differ")
    del sa, sb
    n = 8
    while True:                                 # size the windows on the slower leg
        us = max(window(leg_a, n), window(leg_b, n))
        if us * n >= MIN_SECONDS * 1e6:
            break
        n = int(n * max(2.0, 1.2 * MIN_SECONDS * 1e6 / (us * n)))
    t = {"a": [], "b": []}
    for _ in range(WINDOWS):
        t["a"].append(window(leg_a, n))
        t["b"].append(window(leg_b, n))
    print(f"{kind}: {nt} tables, D {D}, batch {batch}, {sum(bags)} lookups per sample, {nbytes / 1e6:.1f} MB per update by the formula; "
          f"{n} updates per window, {WINDOWS} interleaved windows per leg; the two legs leave the same bits")
    la, lb = sum(map(launches_of, seen["a"])), sum(map(launches_of, seen["b"]))
    print(f"  routes: (a) {' '.join(seen['a'])} | (b) {' '.join(f'L={L}x{len(sel)}:{r}' for L, sel, r in zip(sizes, groups, seen['b']))}")
    for leg, what in (("a", f"(a) ragged, 1 call, {la} launches"), ("b", f"(b) per bag size, {len(sizes)} calls, {lb} launches")):
        v = np.array(t[leg])
        print(f"  {what:44s} us per update: {' '.join(f'{u:7.1f}' for u in v)} | min {v.min():7.1f} median {np.median(v):7.1f} max {v.max():7.1f} "
              f"| spread {100 * (v.max() - v.min()) / np.median(v):4.1f} % | {nbytes / np.median(v) / 1e6 / (HBM_PEAK / 1e12):.3f} of 8 TB/s at the median", flush=True)
    ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
    print(f"  (a) / (b) at the medians: {ma / mb:.3f}")
    del tables, ids, g, ws, state
    torch.cuda.empty_cache()
    return ma, mb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bag-sizes", default=MLPERF_BAGS, help="one bag size per table, a-b-c-...")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", default=None, help="table row counts r-r-... (default: bench.py's MLPerf workload)")
    ap.add_argument("--dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--rule", default="both", choices=["sgd", "rowwise", "both"])
    ap.add_argument("--legs", default="update", choices=["update", "pair", "both"], help="update: ragged against per bag size; pair: the sort call and the apply call alone")
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
    bu, b16 = capi.bags_update_api(hip), capi.bf16_api(hip)
    bs = capi.bags_sort_api(hip) if a.legs != "update" else None
    print(f"device: {torch.cuda.get_device_name(0)}; calls on the null stream, HIP events around each window")
    for bf16 in ([False, True] if a.dtype == "both" else [a.dtype == "bf16"]):
        for rule in (["sgd", "rowwise"] if a.rule == "both" else [a.rule]):
            bench(hip, bu, b16, rows, bags, a.dim, a.batch, bf16, rule, a.legs, bs)


if __name__ == "__main__":
    main()
