#!/usr/bin/env python3
"""The int8 Linear forward (include/ffh_q8_linear.h) beside the exact-fp32 and the bf16 tensor-op forward of the same layer, on the GPU, and the
driver's held-out evaluation with fp32 and with int8 MLP layers from one checkpoint.
  python3 tools/q8_linear_bench.py [--batch 32768] [--rounds 7] [--iters 20] [--no-driver] [--out profiles/q8_linear_measurements.txt]

1. Per layer shape (the Terabyte top MLP 3456-1024-1024-512-256 and one narrow layer): four legs in one process, interleaved (every round times each
   once, in turn, after a warm-up of all): the activation quantizer alone, the quantizer + int8 GEMM (what eval_batch() runs for the layer), and
   ffh_linear_fwd in the exact mode and in the tensor-op mode (fp32 operands rounded to bf16 in the kernel).  Device events around `iters` calls;
   median and min..max of the windows; rates by the layer's 2 B in out operations.
2. The driver: a Criteo-Kaggle-like model trained from random data with synthetic logistic labels and saved, then --eval-only --load-checkpoint twice,
   --eval-mlp-dtype fp32 and int8: the EVAL lines side by side.
Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dlrm_flexflow_amd import capi  # noqa: E402
import _lab  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32768)
ap.add_argument("--shapes", default="3456x1024,1024x1024,1024x512,512x256,256x64")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--no-driver", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q8_linear_measurements.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "q8_linear_bench.py measures on the GPU"
hip = _lab.load_hip(0)
q8l = capi.q8_linear_api(hip)
s = torch.cuda.current_stream().cuda_stream
B = a.batch


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def legs(fns):
    for fn in fns:
        window(fn, 5)
    t = [[] for _ in fns]
    for _ in range(a.rounds):
        for k, fn in enumerate(fns):
            t[k].append(window(fn, a.iters))
    return [(statistics.median(v), min(v), max(v)) for v in t]


def math_mode(mode):
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, mode) == 0


lines = [f"# tools/q8_linear_bench.py --batch {B} --shapes {a.shapes} --rounds {a.rounds} --iters {a.iters}   ({torch.cuda.get_device_name(0)})",
         "# 1. us per call: median (min..max) of the windows, legs interleaved; T(FL)OP/s = 2 B in out / time; relu, bias"]
for shape in a.shapes.split(","):
    n_in, n_out = (int(v) for v in shape.split("x"))
    x, W, bias = torch.randn(B, n_in, device="cuda"), torch.randn(n_out, n_in, device="cuda") * 0.05, torch.randn(n_out, device="cuda")
    y = torch.empty(B, n_out, device="cuda")
    ldq = q8l.ldq(n_in)
    xq, sx = torch.empty(B * ldq, dtype=torch.int8, device="cuda"), torch.empty(B, device="cuda")
    wq, sw = torch.empty(n_out * ldq, dtype=torch.int8, device="cuda"), torch.empty(n_out, device="cuda")
    q8l.quantize_weights([(W, n_in, wq, sw, n_out, n_in)], s)

    def quant():
        q8l.quantize_rows(x, n_in, xq, sx, B, n_in, s)

    def int8():
        quant()
        q8l.fwd(xq, wq, sx, sw, bias, y, n_out, B, n_in, n_out, capi.AC_MODE_RELU, s)

    def fp32():
        hip.call("ffh_linear_fwd", x, n_in, y, n_out, W, bias, n_in, n_out, B, capi.AC_MODE_RELU, s)

    def bf16():
        math_mode(1)
        fp32()
        math_mode(0)

    r = legs([quant, int8, fp32, bf16])
    ops = 2.0 * B * n_in * n_out
    fmt = lambda k: f"{r[k][0]:.1f} ({r[k][1]:.1f}..{r[k][2]:.1f}) us"
    rate = lambda k: f"{ops / (r[k][0] * 1e-6) / 1e12:.1f}"
    line = (f"B={B} {n_in}->{n_out}: int8 with its row quantizer {fmt(1)} [{rate(1)} TOP/s], of that the quantizer {fmt(0)}; exact fp32 {fmt(2)} "
            f"[{rate(2)} TFLOP/s]; bf16 tensor-op {fmt(3)} [{rate(3)} TFLOP/s]; fp32 / int8 = {r[2][0] / r[1][0]:.2f}, bf16 / int8 = {r[3][0] / r[1][0]:.2f}")
    lines.append(line)
    print(line, flush=True)

if not a.no_driver:
    exe = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
    model = ["-ll:gpu", "1", "-b", "2048", "--arch-sparse-feature-size", "64", "--arch-embedding-size", "-".join(["20000"] * 26), "--arch-mlp-bot",
             "13-512-256-64", "--arch-mlp-top", "1728-1024-1024-512-256-1", "--data-size", str(2048 * 50), "--loss", "bce", "--synthetic-labels", "logistic",
             "--eval-batches", "8", "--seed", "1", "--lr", "0.1"]
    lines.append("# 2. the driver: " + " ".join(model) + "; 4 epochs, --save-checkpoint; then --eval-only --load-checkpoint, --eval-mlp-dtype fp32 and int8")
    with tempfile.TemporaryDirectory() as ck:
        runs = (("train", ["--epochs", "4", "--save-checkpoint", ck]), ("fp32 eval", ["--eval-only", "--load-checkpoint", ck, "--eval-mlp-dtype", "fp32"]),
                ("int8 eval", ["--eval-only", "--load-checkpoint", ck, "--eval-mlp-dtype", "int8"]))
        for name, extra in runs:
            p = subprocess.run([exe, *model, *extra], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:      # (what part 1 measured is still written)
                lines.append(f"   {name}: exit status {p.returncode}: {p.stderr.strip().splitlines()[-1] if p.stderr.strip() else ''}")
                print(lines[-1], flush=True)
                break
            for ln in p.stdout.splitlines():
                if ln.startswith("EVAL") or "eval MLP" in ln:
                    lines.append(f"   {name}: {ln}")
                    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
