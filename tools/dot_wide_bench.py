#!/usr/bin/env python3
"""The wide dot interaction (include/ffh_dot_wide.h) beside the operator chain it replaces, on the GPU.
  python3 tools/dot_wide_bench.py [--batch 8192] [--d 128] [--c 33,64,128] [--rounds 7] [--out profiles/dot_wide_measurements.txt]

Per shape and direction: the one-launch kernel and the chain (--arch-interaction-op dot-tril-ops: transpose -> batch_matmul -> tril -> concat,
with the zeroing its accumulating backward needs), timed with device events in interleaved legs (kernel, chain, kernel, chain ...: `rounds`
windows of `iters` calls each after a warm-up of both), median and min..max of the windows, and the kernel's fraction of the HBM rate by the
algorithmic bytes 4 (c d + d + c (c - 1) / 2) forward, that plus 4 c d backward (stored, not accumulated).  The chain's tril stops at 64 rows:
beyond that there is no chain to time, and the line says so.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dlrm_flexflow_amd import capi  # noqa: E402
import _lab  # noqa: E402

HBM_BYTES_PER_S = 8.0e12      # MI355X: 8 TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--c", default="33,64,128")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dot_wide_measurements.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "dot_wide_bench.py measures on the GPU"
hip = _lab.load_hip(0)
wide = capi.dot_wide_api(hip)
s = torch.cuda.current_stream().cuda_stream
B, d = a.batch, a.d


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def legs(fns):
    """Interleaved legs: every round times each of `fns` once, in turn.  -> per fn (median, min, max) in us."""
    for fn in fns:
        window(fn, 5)
    t = [[] for _ in fns]
    for _ in range(a.rounds):
        for k, fn in enumerate(fns):
            t[k].append(window(fn, a.iters))
    return [(statistics.median(v), min(v), max(v)) for v in t]


lines = [f"# tools/dot_wide_bench.py --batch {B} --d {d} --c {a.c} --rounds {a.rounds} --iters {a.iters}   ({torch.cuda.get_device_name(0)})",
         "# us per call: median (min..max) of the windows; kernel and chain in interleaved legs; HBM fraction of the kernel at 8 TB/s"]
for c in [int(v) for v in a.c.split(",")]:
    P, wo = c * (c - 1) // 2, d + c * (c - 1) // 2
    z = torch.randn(B, c * d, device="cuda")
    out, g, zg = torch.empty(B, wo, device="cuda"), torch.randn(B, wo, device="cuda"), torch.zeros(B, c * d, device="cuda")
    fwd = lambda: wide.call("ffh_dot_interaction_wide_fwd", z, c * d, out, wo, B, c, d, s)
    bwd = lambda: wide.call("ffh_dot_interaction_wide_bwd", z, c * d, g, wo, zg, c * d, B, c, d, capi.DOT_BWD_OVERWRITE, s)
    fns = [fwd, bwd]
    if c <= 64:      # the chain on the same z: zt = z^T per sample, o = z zt, out = [z row 0 | tril(o)]
        zt, o = torch.empty(B, d * c, device="cuda"), torch.empty(B, c * c, device="cuda")
        ztg, og = torch.empty_like(zt), torch.empty_like(o)

        def chain_fwd():
            hip.transpose("ffh_transpose_fwd", zt, z, [B, c, d], [0, 2, 1], s)
            hip.call("ffh_bmm_fwd", o, z, zt, c, c, d, B, -1, -1, -1, s)
            hip.call("ffh_tril_fwd", out[:, d:], wo, o, B, c, s)
            hip.concat("ffh_concat_fwd", out, wo, [z], [d], [c * d], B, s)      # (the triangle is in place: row 0 is copied)

        def chain_bwd():
            hip.call("ffh_zero", og, og.numel() * 4, s)
            hip.call("ffh_zero", ztg, ztg.numel() * 4, s)
            hip.call("ffh_zero", zg, zg.numel() * 4, s)
            hip.concat("ffh_concat_bwd", g, wo, [zg], [d], [c * d], B, s)      # row 0's direct path
            hip.call("ffh_tril_bwd", og, g[:, d:], wo, B, c, s)
            hip.call("ffh_bmm_bwd", og, z, zg, zt, ztg, c, c, d, B, s)
            hip.transpose("ffh_transpose_bwd", zg, ztg, [B, c, d], [0, 2, 1], s)
        fns += [chain_fwd, chain_bwd]
    r = legs(fns)
    fb, bb = 4 * B * (c * d + d + P), 4 * B * (2 * c * d + d + P)
    for k, (name, nbytes) in enumerate((("fwd", fb), ("bwd", bb))):
        med, lo, hi = r[k]
        line = f"B={B} c={c} d={d} {name}: wide {med:.1f} ({lo:.1f}..{hi:.1f}) us, {nbytes / 1e6:.1f} MB, {nbytes / (med * 1e-6) / HBM_BYTES_PER_S:.2f} of HBM"
        if len(r) > 2:
            cm, cl, ch = r[2 + k]
            line += f"; chain {cm:.1f} ({cl:.1f}..{ch:.1f}) us, chain / wide = {cm / med:.2f}"
        else:
            line += "; chain: none (ffh_tril stops at 64 rows)"
        lines.append(line)
        print(line, flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
