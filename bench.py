#!/usr/bin/env python3
"""bench.py -- DLRM training throughput (samples/s) of the MI355X-native path, one JSON line.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload terabyte|kaggle|tiny|mlperf|giant|giant-row]
                  [--scaling strong|weak] [--per-gpu-batch B] [--dump-outputs DIR] [--full]

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process never touches a GPU -- it starts N child
ranks of itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set), relays rank 0's single
JSON line and exits non-zero if any child fails.  Under `python -m torch.distributed.run --nproc-per-node N ...
bench.py --gpus N` (WORLD_SIZE already set) it is one of the ranks.

A "step" is one training iteration of the reference driver's loop -- forward, zero_gradients, backward, update
[ref: examples/cpp/DLRM/dlrm.cc:166-182] -- on one resident synthetic batch (the reference reuses the warm-up batch
for random input, :167-173).  Default workload = the configuration BASELINE.json's metric is quoted on: the
Criteo-Terabyte shape (26 tables with the MLPerf 40M-capped row counts, 96 GB fp32, emb_dim 128, bot 13-512-256-128,
top 3456-1024-1024-512-256-1, cat interaction) at GLOBAL batch 32768.  It fits one MI355X, so N = 1 runs exactly it;
N > 1 shards the tables table-wise (table t on rank t % N, the reference strategy generator's policy), keeps the MLPs
data-parallel and, by default, keeps the global batch at 32768 ("scaling": "strong", BASELINE configs[2]);
`--scaling weak` gives every rank 32768 samples instead.  All-to-all each way + one all-reduce of the MLP gradients
over RCCL, called from the C++ host layer on a communicator bootstrapped over torch.distributed ("nccl");
`--torch-collectives` serves them through torch.distributed instead.  fp32 throughout (the reference's arithmetic).

A plain run sets up, warms up, times the K steps and prints the headline line (samples/s, ms_per_step, the workload, the
loss over the timed steps; at N > 1 the collective counts and payloads).  `--dump-outputs DIR` writes what the last timed step
computed (dump_outputs()) before the line is printed.  With `--full` the line also carries
  roofline      the embedding gather kernel (BASELINE's second metric) of THIS workload on rank 0: algorithmic bytes
                (B*(L*(8+4D)+4D) per table; 26,832 B/sample at the Terabyte shape = 879 MB per launch at
                N = 1) / average HIP-event time of back-to-back launches on the model's own stream; `traffic` = HBM
                bytes per launch from the committed rocprofv3 --pmc passes (profiles/), `achieved_from_traffic` the
                same rate priced on those bytes
  kernels       the fused embedding backward+SGD (same treatment); the largest Linear layer alone (MFMA roofline,
                forward and backward); the whole step; `kaggle_secondary` = BASELINE configs[1] (B = 2048) timed in
                the same process after the headline (skipped with --no-secondary and for N > 1)
  cpu_baseline  the same application on the host cores with the CPU oracle as kernel library (kind "port": the
                reference has no CPU path for this step), N = 1 only, on a bounded sample (stated in `sample`)
  collectives_in_step_us  (N > 1 or --force-exchange) the collectives' intervals inside real eager steps

The measured path always runs the HIP library and refuses to start without a GPU.  (tests/test_launchers.py walks this
file's N > 1 rank code on the CPU through the hidden --functional-test-backend <kernel library> flag -- gloo collectives, an
explicitly named kernel library, the line marked FUNCTIONAL_TEST_NOT_A_MEASUREMENT; nothing is measured or reported there.)
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

KAGGLE_ROWS = "1396-550-1761917-507795-290-21-11948-608-3-58176-5237-1497287-3127-26-12153-1068715-10-4836-2085-4-1312273-17-15-110946-91-72655"
TERABYTE_ROWS = "39884406-39043-17289-7420-20263-3-7120-1543-63-38532951-2953546-403346-10-2208-11938-155-4-976-14-39979771-25641295-39664984-585935-12972-108-36"
HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured streaming ceiling
F32_PEAK_TFLOPS = 157.3     # v_mfma_f32_32x32x2_f32 dense peak
BF16_PEAK_TFLOPS = 2500.0   # v_mfma_f32_32x32x16_bf16 dense peak (no sparsity)
DEFAULT_BATCH = {"terabyte": 32768, "kaggle": 2048, "tiny": 128, "giant": 4096, "giant-row": 4096, "mlperf": 8192, "mlperf-allpairs": 8192}


def workload(name: str, global_batch: int):
    B = global_batch
    if name == "terabyte":     # BASELINE configs[2]: all 26 tables (96 GB fp32) fit one MI355X; table-wise for N > 1
        return dict(name="criteo-terabyte-shape", rows=TERABYTE_ROWS, D=128, bot="13-512-256-128", top="3456-1024-1024-512-256-1", B=B)
    if name == "kaggle":       # BASELINE configs[1]
        return dict(name="criteo-kaggle-shape", rows=KAGGLE_ROWS, D=16, bot="13-512-256-64-16", top="432-512-256-1", B=B)
    if name == "tiny":         # BASELINE configs[0]
        return dict(name="tiny", rows="-".join(["1000"] * 8), D=16, bot="13-64-16", top="144-64-1", B=B)
    if name == "giant":        # BASELINE configs[4]: one 200M-row x 256 table (204.8 GB), column-wise over the ranks
        return dict(name="giant-table-column-wise", rows="200000000", D=256, bot="13-512-256", top="512-512-256-1", B=B,
                    extra=["--column-shard-rows", "100000000"])
    if name == "mlperf":       # BASELINE configs[3]: dot interaction keeping the 351 products i > j of the 27 x 27 matrix
        return dict(name="mlperf-dlrm-dot", rows=TERABYTE_ROWS, D=128, bot="13-512-256-128", top="479-1024-1024-512-256-1", B=B,
                    extra=["--arch-interaction-op", "dot-tril"])
    if name == "mlperf-allpairs":   # the same with all 729 products, the composition of the reference's op tests (test_harness.py:125-177)
        return dict(name="mlperf-dlrm-dot-allpairs", rows=TERABYTE_ROWS, D=128, bot="13-512-256-128", top="857-1024-1024-512-256-1", B=B,
                    extra=["--arch-interaction-op", "dot"])
    if name == "giant-row":    # the same table split ROW-wise: partial bag sums + reduce-scatter forward, all-gather backward
        return dict(name="giant-table-row-wise", rows="200000000", D=256, bot="13-512-256", top="512-512-256-1", B=B,
                    extra=["--row-shard-rows", "100000000"])
    raise SystemExit(f"unknown workload {name}")


def flags_of(w, extra=()):
    return ["-b", str(w["B"]), "--arch-sparse-feature-size", str(w["D"]), "--arch-embedding-size", w["rows"],
            "--arch-mlp-bot", w["bot"], "--arch-mlp-top", w["top"], "--data-size", str(w["B"]), *w.get("extra", []), *extra]


def pmc_traffic(key):
    """HBM bytes per launch of the embedding kernels from the committed rocprofv3 --pmc passes (profiles/), or {}."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if not files:
        return {}, None
    return json.load(open(files[-1])).get(key) or {}, os.path.relpath(files[-1], ROOT)


def traffic_file_is_current(src):
    """The committed PMC file names the kernels it measured; if one of them no longer exists in libffhip.so the kernels have
    changed since and the `traffic` figure is stale."""
    if not src:
        return None
    try:
        d = json.load(open(os.path.join(ROOT, src)))
        names = set()
        for blk in d.values():
            for k in (blk.get("per_kernel") or {}):
                names.add(k.split("<")[0].strip())
        blob = open(os.path.join(ROOT, "dlrm_flexflow_amd", "csrc", "libffhip.so"), "rb").read()
        missing = sorted(n for n in names if n.encode() not in blob)
        if missing:
            print(f"bench: WARNING: {src} names kernels that are not in libffhip.so any more ({', '.join(missing)}): roofline.traffic is stale, "
                  "re-run tools/pmc_traffic.sh", file=sys.stderr, flush=True)
        return not missing
    except Exception as e:  # noqa: BLE001
        print("bench: could not check", src, e, file=sys.stderr)
        return None


def mlp_flops_per_sample(w):
    bot = [int(x) for x in w["bot"].split("-")]
    top = [int(x) for x in w["top"].split("-")]
    if "--arch-interaction-op" not in w.get("extra", []):
        top[0] = bot[-1] + len(w["rows"].split("-")) * w["D"]     # cat: input width comes from the tensor, not the flag
    f = sum(2 * a * b for a, b in zip(bot[:-1], bot[1:])) + sum(2 * a * b for a, b in zip(top[:-1], top[1:]))
    return 3 * f   # forward + dX + dW


# ------------------------------------------------------------------------------------------------------------------
# CPU baseline (host only; the oracle is the kernel library of the same C++ application)
# ------------------------------------------------------------------------------------------------------------------
CPU_ROW_CAP = 1_000_000     # rows per table in the CPU sample: initialising 24 G table elements on the host would take minutes
CPU_BATCH = 2048            # samples per CPU step (a 32768-sample step is ~1 TFLOP: minutes on one thread): 256 blocks of 8 samples for the oracle's
                            # OpenMP loops, so that the all-threads leg of a 256-thread host has one block per thread


def cpu_sample_workload(name):
    w = workload(name, min(CPU_BATCH, DEFAULT_BATCH.get(name, CPU_BATCH)))
    rows = [min(int(r), CPU_ROW_CAP) for r in w["rows"].split("-")]
    w = dict(w, rows="-".join(str(r) for r in rows))
    w["extra"] = [x for x in w.get("extra", []) if x not in ("--column-shard-rows", "--row-shard-rows", "100000000")]
    return w


def cpu_baseline_leg(name, budget_s, out):
    """One timed leg in its own process (OMP_NUM_THREADS is read when libgomp starts): prints {steps, seconds, threads}."""
    from oracle import oracle
    from dlrm_flexflow_amd import ffmodel
    oracle.build()
    import ctypes
    w = cpu_sample_workload(name)
    threads = int(ctypes.CDLL("libgomp.so.1").omp_get_max_threads())     # threads the oracle's OpenMP loops will use
    app = ffmodel.DLRM(flags_of(w, ["--backend", oracle.ORACLE_LIB, "--no-trace"]))
    app.warmup()
    t0 = time.perf_counter()
    app.train_steps(1, trace=False)
    app.model.sync()
    t1 = time.perf_counter() - t0
    n = max(1, min(5000, int(budget_s / max(t1, 1e-5))))      # a few seconds of CPU work per leg
    t0 = time.perf_counter()
    app.train_steps(n, trace=False)
    app.model.sync()
    dt = time.perf_counter() - t0
    app.close()
    print("CPU_LEG " + json.dumps({"steps": n, "seconds": dt, "threads": threads, "batch": w["B"]}), file=out, flush=True)


def reference_lookup(budget_s=6.0):
    """The reference's ONLY CPU arithmetic for this path -- EmbeddingLookup_int64_t_float_float__avx2_fma
    [ref: src/ops/embedding.cc:23-342, caller forward_task_cpu :377-415], compiled from the reference's own source into
    oracle/_ref/libref_embedding.so (oracle/Makefile) -- timed as the reference runs it: one thread, bags of one id, emb_dim
    128, uniform ids over a table far larger than the caches.  None when the library is not on this box."""
    import ctypes as C
    import numpy as np
    lib_path = os.path.join(ROOT, "oracle", "_ref", "libref_embedding.so")
    if not os.path.exists(lib_path):
        return None
    fn = getattr(C.CDLL(lib_path), "_Z45EmbeddingLookup_int64_t_float_float__avx2_fmaiiiiPKfPKlPKiS0_bPf")
    fn.restype = None
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_bool, C.c_void_p]
    D, R, B = 128, 4_000_000, 32768                      # 2.05 GB table, one bench batch of one table per call
    rng = np.random.default_rng(0)
    w = np.empty((R, D), np.float32); w[:] = 0.5
    idx = rng.integers(0, R, B).astype(np.int64)
    lengths = np.ones(B, np.int32)
    out = np.empty((B, D), np.float32)
    call = lambda: fn(D, B, B, R, w.ctypes.data, idx.ctypes.data, lengths.ctypes.data, None, False, out.ctypes.data)
    call()                                               # warm (page-in of the table)
    sets = [rng.integers(0, R, B).astype(np.int64) for _ in range(8)]
    t = 0.0; calls = 0
    while t < budget_s:
        idx = sets[calls % 8]
        t1 = time.perf_counter(); call(); t += time.perf_counter() - t1; calls += 1
    nbytes = B * (8 + 4 * D + 4 * D)                      # the same per-lookup bytes the GPU roofline bills
    return {"kind": "reference", "function": "EmbeddingLookup_int64_t_float_float__avx2_fma (oracle/_ref/libref_embedding.so, compiled from "
            "/root/reference/src/ops/embedding.cc:17-374 by oracle/Makefile)", "cores": 1,
            "lookups_per_s": round(calls * B / t, 1), "GB/s": round(calls * nbytes / t / 1e9, 3), "unit": "lookups/s",
            "sample": f"{calls} calls of {B} single-id bags, emb_dim {D}, uniform ids over a {R}-row table ({R * D * 4 / 1e9:.2f} GB), {t:.1f} s, 1 thread"}


def cpu_baseline(args, budget_s=24.0):
    """The same DLRM application with the CPU oracle as its kernel library, timed on the host: one thread (the reference's
    CPU embedding loop is serial), a quarter of the hardware threads and all of them; `value` is the fastest."""
    ncpu = os.cpu_count() or 1
    w = cpu_sample_workload(args.workload)
    legs = {}
    for threads in sorted({1, max(1, ncpu // 4), ncpu}):
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND="false")
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-leg", "--workload", args.workload, "--leg-budget", str(budget_s / 3)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("CPU_LEG ")]
        if r.returncode != 0 or not line:
            raise RuntimeError(f"cpu baseline leg ({threads} threads) failed:\n{r.stdout[-500:]}{r.stderr[-500:]}")
        leg = json.loads(line[-1][8:])
        legs[leg["threads"]] = {"value": round(leg["steps"] * leg["batch"] / leg["seconds"], 2), "steps": leg["steps"], "seconds": round(leg["seconds"], 2)}
    best = max(legs, key=lambda t: legs[t]["value"])
    b = legs[best]
    capped = w["rows"] != workload(args.workload, 1)["rows"]
    return {"value": b["value"], "unit": "samples/s", "cores": best, "kind": "port",
            "sample": f"{b['steps']} training steps of the same {w['name']} model (emb_dim {w['D']}, bot {w['bot']}, top {w['top']}) at batch {w['B']} in "
                      f"{b['seconds']:.1f} s" + (f", rows per table capped at {CPU_ROW_CAP} (host-side table init; favours the CPU's caches)" if capped else "") +
                      "; oracle/ffh_oracle.c (OpenMP over the batch) behind the same C++ FFModel host code",
            "host_cpus": ncpu,
            "by_threads": {str(t): legs[t]["value"] for t in sorted(legs)},
            "scaling_note": "the port is the test oracle: clarity over speed.  Its GEMMs run one fp32 FMA chain per output element (the order the parity tests "
                            "pin), OpenMP over blocks of 8 samples (forward / dX: a weight row is used for the whole block while it is cached) and of 8 output rows "
                            "(dW: a sample's x row likewise) -- round 6: before, every sample re-streamed the layer's whole weight matrix and the all-threads leg was "
                            "slower than the quarter leg; `value` is the fastest leg, `cores` its thread count.  The reference's own CPU arithmetic for this "
                            "path is `reference_lookup` (one thread, as the reference runs it).",
            "reference_lookup": reference_lookup()}


# ------------------------------------------------------------------------------------------------------------------
# N > 1 without a launcher: start the ranks ourselves, before anything initialises a GPU
# ------------------------------------------------------------------------------------------------------------------
def spawn_ranks(n: int) -> int:
    """Starts the n ranks (nothing here touches a GPU), relays rank 0's single JSON line, and makes every rank's stderr visible in
    this process's stderr with a "[rank r]" tag in front of each line -- a failure on rank 5 of 8 is then readable in the driver's log."""
    import threading
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), FFM_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    buf = []
    tails = [[] for _ in range(n)]

    def relay(r, pipe):
        for line in pipe:
            tails[r].append(line)
            del tails[r][:-40]
            sys.stderr.write(f"[rank {r}] {line}")
            sys.stderr.flush()

    threads = [threading.Thread(target=lambda: buf.append(procs[0].stdout.read()), daemon=True)]   # rank 0 prints the one JSON line
    threads += [threading.Thread(target=relay, args=(r, p.stderr), daemon=True) for r, p in enumerate(procs)]
    for t in threads:
        t.start()
    deadline = time.time() + float(os.environ.get("FFM_SPAWN_TIMEOUT", "1500"))
    while True:
        rcs = [p.poll() for p in procs]
        if all(rc is not None for rc in rcs):
            break
        if any(rc not in (None, 0) for rc in rcs) or time.time() > deadline:
            first_bad = [i for i, rc in enumerate(rcs) if rc not in (None, 0)]
            time.sleep(2.0)                  # let the failing rank's peers print what they have
            for p in procs:
                if p.poll() is None:
                    p.kill()                 # exactly the children started above, by handle
            rcs = [p.wait() for p in procs]
            if first_bad:
                sys.stderr.write(f"bench.py: rank(s) {first_bad} failed first; the others were ended by the launcher\n")
            break
        time.sleep(0.05)
    for t in threads:
        t.join(timeout=10)
    out0 = buf[0] if buf else ""
    bad = [i for i, rc in enumerate(rcs) if rc != 0]
    line = [l for l in out0.splitlines() if l.startswith("{")]
    if bad or not line:
        sys.stderr.write(f"bench.py: rank(s) {bad} failed (exit codes {rcs}); rank 0 printed {len(line)} JSON line(s)\n")
        for r in bad:
            sys.stderr.write(f"---- last lines of rank {r} ----\n" + "".join(f"[rank {r}] {l}" for l in tails[r][-15:]))
        return 1
    print(line[-1], flush=True)
    return 0


def largest_linear(w, B, t_fwd, t_bwd, bf16):
    """MFMA roofline of the Linear layer with the most multiply-adds, timed alone with HIP events on the model's stream,
    back to back."""
    bot, top = [int(v) for v in w["bot"].split("-")], [int(v) for v in w["top"].split("-")]
    if "--arch-interaction-op" not in w.get("extra", []):
        top[0] = bot[-1] + len(w["rows"].split("-")) * w["D"]
    pairs = [(a, b) for d in (bot, top) for a, b in zip(d[:-1], d[1:])]
    i, o = max(pairs, key=lambda p: p[0] * p[1])
    f = 2.0 * B * i * o
    peak = BF16_PEAK_TFLOPS if bf16 else F32_PEAK_TFLOPS
    return {"layer": f"{i}->{o}, batch {B}", "bound": "mfma", "peak": peak, "unit": "TFLOP/s",
            "dtype": "bf16 operands, f32 accumulate" if bf16 else "f32",
            "fwd": {"us": round(t_fwd * 1e6, 2), "achieved": round(f / t_fwd / 1e12, 1), "frac": round(f / t_fwd / 1e12 / peak, 3)},
            "bwd": {"us": round(t_bwd * 1e6, 2), "achieved": round(2 * f / t_bwd / 1e12, 1), "frac": round(2 * f / t_bwd / 1e12 / peak, 3),
                    "note": "dX and dW GEMMs of the layer (dW on its own stream where the layer is large enough), interval on the model's stream incl. the join"}}


def hbm_block(kernel, nbytes, sec, traffic=None, src=None, note=None, in_step_sec=None):
    d = {"kernel": kernel, "bound": "hbm", "achieved": round(nbytes / sec / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(nbytes / sec / 1e9 / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": src if traffic else None,
         "us_per_launch": round(sec * 1e6, 2), "algorithmic_bytes_per_launch": nbytes,
         "probe": "back-to-back launches on the model's stream, HIP events; the launches rotate over 4 id sets drawn with their own seeds (a launch "
                  "never finds the previous launch's rows in the 256 MiB Infinity Cache)"}
    if in_step_sec:
        d["us_per_launch_in_step"] = round(in_step_sec * 1e6, 2)     # events around the same launch inside real steps: it shares the chip there
    if traffic:
        d["traffic_source_current"] = traffic_file_is_current(src)
    if traffic:
        d["achieved_from_traffic"] = round(traffic / sec / 1e9, 1)     # HBM GB/s priced on the PMC bytes instead of the formula
        d["traffic_over_algorithmic"] = round(traffic / nbytes, 3)
    if note:
        d["note"] = note
    return d


def bf16_mode_block(ffmodel, w, local_rank, B, split=False):
    """The same workload in one of the two bf16-pipe math modes, reported beside the exact-fp32 headline, never as it:
    --allow-tensor-op-math-conversion (bf16 operands, fp32 accumulate: the reference's tensor-op switch) or, split=True,
    --fp32-split-bf16x3 (fp32-accurate: three bf16 terms per operand, six products; held to the fp32 parity bound)."""
    flag = "--fp32-split-bf16x3" if split else "--allow-tensor-op-math-conversion"
    app = ffmodel.DLRM(flags_of(w, ["--device", str(local_rank), flag, "--no-trace"]))
    app.warmup()
    # (settled clocks: the first ~60 launches after an idle stretch run 10-15 % slow -- 0.2 s of steps before the timed ones)
    app.train_steps(40 if B > 4096 else 200, trace=False)
    app.model.sync()
    n = 50 if B > 4096 else 200
    t0 = time.perf_counter()
    app.train_steps(n, trace=False)
    app.model.sync()
    dt = (time.perf_counter() - t0) / n
    app.time_kernel(6, 60)
    t_f = app.time_kernel(6, 30) * 1e-3
    t_b = app.time_kernel(7, 30) * 1e-3
    app.close()
    flops = mlp_flops_per_sample(w) * B
    blk = largest_linear(w, B, t_f, t_b, not split)
    if split:
        # the GEMMs run on the bf16 matrix pipe: six bf16 MFMAs per fp32-equivalent product, so the pipe's ceiling for this mode is
        # BF16_PEAK / 6 fp32-equivalent TFLOP/s (not the fp32 MFMA peak: priced on that the fraction would exceed 1)
        peak6 = BF16_PEAK_TFLOPS / 6.0
        blk["dtype"] = "fp32 via 3x bf16 split: three bf16 terms per operand, six v_mfma_f32_16x16x32_bf16 products per k-step, fp32 accumulate"
        blk["peak"] = round(peak6, 1)
        for leg in ("fwd", "bwd"):
            blk[leg]["frac"] = round(blk[leg]["achieved"] / peak6, 3)
            blk[leg]["x_fp32_mfma_peak"] = round(blk[leg]["achieved"] / F32_PEAK_TFLOPS, 3)
        blk["note"] = "achieved = fp32-equivalent flops (2*B*in*out); peak = bf16 MFMA peak / 6 (six bf16 products per fp32-accurate product); x_fp32_mfma_peak = the same rate over the 157.3 TFLOP/s fp32 MFMA peak"
        i_o = blk["layer"].split(",")[0]
        roof = {"kernel": f"gemm_x3_dma_kernel<false, false, 0> (csrc/linear_x3_dma.hip): forward GEMM of the largest layer ({i_o}), operands streamed from producer-kept "
                          "three-plane images by LDS-DMA, bias + relu + the output's image in the epilogue",
                "bound": "mfma", "achieved": blk["fwd"]["achieved"], "peak": round(peak6, 1), "unit": "TFLOP/s", "frac": blk["fwd"]["frac"], "traffic": None,
                "us_per_launch": blk["fwd"]["us"],
                "algorithmic_flop_per_launch": 2.0 * B * int(i_o.split("->")[0]) * int(i_o.split("->")[1]),
                "note": "achieved = fp32-equivalent flops (2 * batch * in * out) over the launch time (HIP events on the model's stream, back to back, settled clocks); "
                        "peak = dense bf16 MFMA peak / 6: six bf16 products make one fp32-accurate product; counters: profiles/r06_pmc_split_bf16x3_gemm.json "
                        "(matrix pipe busy 86 % of the launch, 0.26 other vector instructions per MFMA); bare MFMAs of this shape sustain 0.81-0.82 of `peak` on this part "
                        "(338-342 TFLOP/s in these units: profiles/r06_lab_mfma_power_probe.txt)"}
        return {"flag": "--fp32-split-bf16x3 (ffh_ctx_set_math_mode(FFH_MATH_FP32_SPLIT_BF16X3)); opt-in: `value` above stays the exact-fp32-MFMA route",
                "metric": "dlrm_training_samples_per_sec", "value": round(B / dt, 1), "unit": "samples/s", "ms_per_step": round(dt * 1e3, 4), "steps": n, "dtype": "f32",
                "parity": "the SAME bound as the exact-fp32 kernels: |error| <= 1e-5 of the term mass (sum_k |a_k b_k|) + 1e-6 against float64 / the fp32 oracle, every GEMM form "
                          "(tests/test_gpu_round6.py, tests/test_bf16_mode.py); error against float64 within 4x the exact kernels' own; three training steps of the whole model "
                          "against the oracle backend in its fp32 mode at rtol 2e-5; producer-kept images bit for bit against a numpy and an oracle restatement",
                "layers": "Linear layers whose GEMMs are at least FFH_BF16X3_MIN_FLOP (1e10: 3456->1024, 1024->1024, 1024->512 at this batch); smaller ones stay on the fp32 MFMA kernels",
                "mlp_tflops_over_whole_step_fp32_equivalent": round(flops / dt / 1e12, 1),
                "x_fp32_mfma_peak_over_whole_step": round(flops / dt / 1e12 / F32_PEAK_TFLOPS, 3), "roofline": roof, "linear_largest_layer": blk}
    return {"flag": "--allow-tensor-op-math-conversion (ffh_ctx_set_math_mode(FFH_MATH_TENSOR_OP_BF16))",
            "dtype": "bf16 GEMM operands, fp32 accumulate; fp32 master weights / activations / gradients in HBM with bfloat16 twins kept by their producers (ffh_ctx_bf16_mirror_set), which the big layers' LDS-DMA GEMMs read",
            "samples_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 4), "mlp_tflops_over_whole_step": round(flops / dt / 1e12, 1),
            "linear_largest_layer": blk,
            "note": "results are fp32 sums of products of bf16-rounded operands, held to the oracle run in the same mode and to a stated 2^-8 bound against the exact mode (tests/test_bf16_mode.py); layers below the twin size round their 4-byte operands between the global load and the LDS store"}


def kaggle_secondary(ffmodel, local_rank):
    """BASELINE configs[1] (Criteo-Kaggle shape, B = 2048) in the same process: the launch-latency regime of the path."""
    w = workload("kaggle", 2048)
    app = ffmodel.DLRM(flags_of(w, ["--device", str(local_rank)]))
    app.warmup()
    g = min(app.time_kernel(2, 30), app.time_kernel(2, 30))
    e = min(app.time_kernel(4, 30), app.time_kernel(4, 30))
    trace = g <= e
    app.train_steps(30, trace=trace)
    app.model.sync()
    t0 = time.perf_counter()
    app.train_steps(300, trace=trace)
    app.model.sync()
    dt = time.perf_counter() - t0
    t_fwd = app.time_kernel(8, 200) * 1e-3
    t_bwd = app.time_kernel(9, 100) * 1e-3
    app.close()
    T, B, D = 26, 2048, 16
    return {"workload": "criteo-kaggle-shape (BASELINE configs[1]): 26 tables, emb_dim 16, batch 2048, bot 13-512-256-64-16, top 432-512-256-1",
            "value": round(300 * B / dt, 1), "unit": "samples/s", "us_per_step": round(dt / 300 * 1e6, 1), "step_graph": bool(trace),
            "step_us_graph_vs_eager": {"graph": round(g * 1e3, 1), "eager": round(e * 1e3, 1)},
            "gather": {"us_per_launch": round(t_fwd * 1e6, 2), "GB/s": round(T * B * (8 + 8 * D) / t_fwd / 1e9, 1)},
            "fused_update": {"us_per_launch": round(t_bwd * 1e6, 2), "GB/s": round(T * B * (8 + 12 * D) / t_bwd / 1e9, 1)}}


DUMP_BYTES = 64_000_000     # --dump-outputs: the files of one run together
DUMP_TABLE_ROWS = 1024      # rows sampled per embedding table


def dump_outputs(app, out_dir, device, on_gpu):
    """--dump-outputs (one rank): what the last timed step computed, as float32 DIR/<name>.npy -- the predictions, the MLP layers'
    parameters after the update and, of each embedding table (tens of GB at the Terabyte shape), the rows at a fixed sample of
    the batch's lookups, drawn with seed 0 (rows the step wrote), gathered by the kernel library the model runs on.  The model's
    inputs and initial weights come from its fixed seed, so equal arguments give equal inputs in every run."""
    import numpy as np
    from dlrm_flexflow_amd import capi
    m = app.model
    m.sync()
    arrays = {"predictions": m.layer_output(m.num_layers - 1).get()}
    tables = []
    for layer in range(m.num_layers):
        name = m.layer_name(layer)
        if name.startswith("Embedding"):
            tables.append((name, m.parameter(layer, 0)))
        else:
            for i in range(m.layer_num_weights(layer)):
                arrays[f"{name}.weight{i}"] = m.parameter(layer, i).get_weights()
    left = DUMP_BYTES - sum(a.nbytes for a in arrays.values())
    if tables:
        assert len(tables) == app.num_tables, f"{len(tables)} embedding layers, {app.num_tables} sparse inputs"
        lib = capi.FFHLib(m.backend["path"], device)
        rng = np.random.default_rng(0)
        try:
            for t, (name, p) in enumerate(tables):
                R, D = p.dims
                ids = app.sparse_input(t).get(np.int64).reshape(-1)
                k = min(ids.size, DUMP_TABLE_ROWS, left // (4 * D * len(tables)))
                sel = np.ascontiguousarray(ids[np.sort(rng.choice(ids.size, k, replace=False))]).reshape(k, 1)
                if k == 0 or sel.min() < 0 or sel.max() >= R:
                    raise SystemExit(f"bench: --dump-outputs: {name}: ids outside [0, {R}) or no room left")
                if on_gpu:
                    import torch
                    idx, rows = torch.from_numpy(sel).to(f"cuda:{device}"), torch.empty(k, D, device=f"cuda:{device}")
                else:
                    idx, rows = sel, np.empty((k, D), np.float32)
                lib.call("ffh_embedding_fwd", idx, rows, p.device_ptr, 1, D, k, R, D, capi.AGGR_MODE_SUM, None)
                if on_gpu:
                    torch.cuda.synchronize(device)
                    rows = rows.cpu().numpy()
                arrays[f"{name}.rows"] = rows
        finally:
            lib.close()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_BYTES, f"--dump-outputs: {total} bytes"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, np.float32))
    print(f"bench: wrote {len(arrays)} arrays ({total / 1e6:.1f} MB) to {out_dir}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="terabyte", help="terabyte (default, BASELINE configs[2] shape at global batch 32768) | kaggle | tiny | mlperf | giant | giant-row | mlperf-allpairs")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"], help="N > 1: keep the GLOBAL batch (strong, default: BASELINE configs[2]) or the per-GPU batch (weak)")
    ap.add_argument("--per-gpu-batch", type=int, default=None, help="samples per GPU and step (implies weak scaling)")
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure what the headline does not need: the per-kernel rooflines, "
                    "the in-step probes, the bf16-pipe modes, the Kaggle-shape block and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write what the last timed step computed as DIR/<name>.npy (float32, "
                    f"at most {DUMP_BYTES // 1_000_000} MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the bf16-pipe modes and the Kaggle-shape block (profile runs: keeps the rocprof averages single-shape)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--force-graph", action="store_true", help="time the hipGraph-replayed step even where eager launches are faster (diagnosis)")
    ap.add_argument("--force-exchange", action="store_true", help="1 GPU: still run the all-to-all / all-reduce path (1-rank RCCL group)")
    ap.add_argument("--torch-collectives", action="store_true", help="serve the all-to-all / all-reduce through torch.distributed callbacks "
                                                                     "instead of calling RCCL from the C++ host layer")
    ap.add_argument("--cpu-baseline-leg", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--leg-budget", type=float, default=7.0, help=argparse.SUPPRESS)
    ap.add_argument("--replicate-embedding-rows", type=int, default=0, help="N > 1: tables with at most this many rows are data-parallel (a copy on every "
                    "rank, dense gradient in the MLP's all-reduce bucket) instead of table-wise in the all-to-all; 0 (default): every table table-wise")
    ap.add_argument("--allreduce-shared-channel", action="store_true", help="N > 1: the MLP-gradient buckets on the SAME RCCL communicator as the all-to-alls (A/B; by default "
                    "they get a second one from ncclCommSplit where every rank has it -- one communicator runs its collectives in issue order)")
    ap.add_argument("--allreduce-own-channel", action="store_true", help=argparse.SUPPRESS)     # (the default since round 6: accepted, no effect)
    ap.add_argument("--shim-flags", default="", help="extra FFConfig flags for A/B runs, e.g. '--serial-dw --no-overlap'")
    ap.add_argument("--dry-run", action="store_true", help=argparse.SUPPRESS)   # tests: ranks rendezvous over gloo and report, no GPU
    ap.add_argument("--functional-test-backend", default="", help=argparse.SUPPRESS)   # tests only: walk this file's whole rank path on the
    #                      CPU (gloo + the given kernel library, i.e. the oracle); the line it prints is not a measurement
    args = ap.parse_args()
    if args.dump_outputs and args.gpus > 1:
        ap.error("--dump-outputs is for one GPU: with more ranks a table may be split over them")
    args.shim_flags = args.shim_flags.replace(",", " ")      # (a comma also separates flags: one shell word in scripted visits)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.cpu_baseline_leg:
        sys.exit(spawn_ranks(args.gpus))   # the parent: no torch import, no HIP call, nothing that initialises a GPU
    # stdout carries the ONE JSON line and nothing else: the C++ driver's printf banner ("[DLRM] ...", flushed by the C
    # runtime at exit) is sent to stderr
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    if args.cpu_baseline_leg:          # child of cpu_baseline(): host only, never touches the GPU
        cpu_baseline_leg(args.workload, args.leg_budget, json_out)
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("FFM_TEST_FAIL_RANK") == str(rank) and args.functional_test_backend:      # tests/test_launchers.py: a rank that dies on purpose
        raise SystemExit(f"rank {rank}: failing on purpose (FFM_TEST_FAIL_RANK)")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: run `python bench.py --gpus {args.gpus}` (it starts its own ranks) or\n"
                         f"  python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
                         f"--master-port 29511 bench.py --gpus {args.gpus} --steps {args.steps} --warmup {args.warmup}")
    # multi-process GPU work on this pool needs dmabuf IPC (hipIpcGetMemHandle fails under the legacy mode): spawn_ranks() sets it for its
    # children, a torchrun launch inherits the shell's -- make sure it is there before anything initialises the GPU
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    if args.dry_run:                   # launcher test (CPU): the ranks meet over gloo, rank 0 reports what it saw
        dist.init_process_group("gloo")
        t = torch.ones(1)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": args.gpus, "ranks_observed": dist.get_world_size(), "sum": float(t.item())}), file=json_out, flush=True)
        dist.barrier()
        dist.destroy_process_group()
        return
    from dlrm_flexflow_amd import ffmodel

    ftest = args.functional_test_backend           # tests only (see the flag): everything below runs, nothing is measured
    if ftest and os.environ.get("FFM_TESTING") != "1":
        sys.exit("bench.py: --functional-test-backend is test scaffolding (tests/test_launchers.py sets FFM_TESTING=1); it measures nothing")
    if not ftest and not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the product path has no CPU fallback)")
    if not ftest:
        torch.cuda.set_device(local_rank)
    comm = None
    collectives = ""
    if world > 1 or args.force_exchange:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        from dlrm_flexflow_amd.comm import RcclComm, TorchComm
        if ftest:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        comm = TorchComm(on_gpu=not ftest)
        collectives = "torch.distributed (RCCL) callbacks" if not ftest else "torch.distributed (gloo) callbacks: FUNCTIONAL TEST, not a measurement"
        if not ftest and not args.torch_collectives and not os.environ.get("FFM_NO_DIRECT_RCCL"):
            try:
                comm = RcclComm(comm, own_bucket_channel=not args.allreduce_shared_channel)       # the same callbacks served by RCCL from the C++ host layer, no Python per collective
                collectives = "RCCL called from the C++ host layer"
            except Exception as e:  # noqa: BLE001  every rank raises together (comm.py): fall back to the torch callbacks
                if rank == 0:
                    print("bench: direct RCCL not used:", e, file=sys.stderr, flush=True)

    weak = args.scaling == "weak" or args.per_gpu_batch is not None
    base = args.per_gpu_batch or DEFAULT_BATCH[args.workload]
    if weak:
        gb = base * world
    else:
        gb = base
        if gb % world:
            raise SystemExit(f"global batch {gb} is not divisible by {world} ranks")
    w = workload(args.workload, gb)
    bf16 = "--allow-tensor-op-math-conversion" in args.shim_flags.split()
    extra = (["--backend", ftest] if ftest else ["--device", str(local_rank)]) + (["--no-trace"] if args.no_trace else []) + (["--force-exchange"] if args.force_exchange else []) + \
            (["--replicate-embedding-rows", str(args.replicate_embedding_rows)] if args.replicate_embedding_rows > 0 else []) + args.shim_flags.split()
    app = ffmodel.DLRM(flags_of(w, extra), comm=comm.struct if comm else None)
    trace = not args.no_trace

    def barrier():
        if not ftest:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    app.warmup()                                   # the reference's own warm-up iteration (loads the batch)
    # hipGraph replay (the reference's Legion trace) vs eager launches: keep whichever is faster on this box
    step_us = {}
    solo = world == 1 and not args.force_exchange
    if not solo and not ("--capture-exchange" in args.shim_flags.split() and collectives.startswith("RCCL called")):
        trace = False                              # collectives served by host callbacks are not capturable; RcclComm's are, behind --capture-exchange
    if trace:
        # best of two short measurements each: one hiccup in either must not pick the slower mode for the whole timed region
        n_probe = 30 if w["B"] <= 4096 else 5
        step_us["graph"] = min(app.time_kernel(2, n_probe), app.time_kernel(2, n_probe)) * 1e3
        step_us["eager"] = min(app.time_kernel(4, n_probe), app.time_kernel(4, n_probe)) * 1e3
        trace = step_us["graph"] <= step_us["eager"] or args.force_graph
    app.train_steps(args.warmup, trace=trace)      # W untimed steps
    app.model.reset_metrics()
    app.model.sync()
    barrier()
    t0 = time.perf_counter()
    app.train_steps(args.steps, trace=trace)       # EXACTLY K timed steps
    app.model.sync()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if ftest else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    pm = app.model.perf_metrics()                  # loss over the K timed steps (before the kernel probes below touch the tables)
    calls = dict(comm.calls) if comm is not None and hasattr(comm, "calls") else None     # collectives of warm-up + W + K steps (the probes below add theirs)
    if args.dump_outputs:
        dump_outputs(app, args.dump_outputs, local_rank, on_gpu=not ftest)
    T = len(w["rows"].split("-"))
    rows_of = [int(r) for r in w["rows"].split("-")]
    replicated = [t for t in range(T) if world > 1 and 0 < rows_of[t] <= args.replicate_embedding_rows]
    owned = len([t for t in range(T) if t % world == rank and t not in replicated])      # tables in this rank's gather launch / all-to-all
    B, D = w["B"], w["D"]
    table_wise = not any(f in w.get("extra", []) for f in ("--column-shard-rows", "--row-shard-rows")) or world == 1
    t_fwd = t_bwd = t_fwd_in = t_bwd_in = t_step_dev = t_lin_fwd = t_lin_bwd = None
    in_step = in_step_max = {}
    if args.full:
        # per-kernel device time, HIP events on the stream the kernels are launched on (the model's stream)
        n_g = 200 if B * owned <= 65536 else 40
        t_fwd = app.time_kernel(8, n_g) * 1e-3 if (rank == 0 and table_wise and owned) else None           # gather kernel alone (no exchange)
        t_bwd = app.time_kernel(9, max(10, n_g // 2)) * 1e-3 if (rank == 0 and table_wise and owned) else None   # fused update kernels alone
        # the same kernels and the collectives inside real eager steps, by events on the streams they are issued on.  COLLECTIVE: the
        # steps run the exchange, so at N > 1 every rank walks them (round-3 advisor: rank 0 alone hung in the first all-to-all); the
        # line reports rank 0's intervals and the maximum over the ranks
        # (also when the timed steps were replayed from a hipGraph: the probed steps are launched eagerly, the kernels are the same)
        in_step = app.probe_step(10 if B > 4096 else 50)
        in_step_max = dict(in_step)
        if world > 1:
            keys = sorted(in_step)
            t = torch.tensor([in_step[k] for k in keys], dtype=torch.float64, device="cpu" if ftest else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            in_step_max = {k: float(v) for k, v in zip(keys, t.tolist())}
        t_fwd_in = in_step["gather"] * 1e-3 if (in_step and t_fwd and in_step["gather"] > 0) else None
        t_bwd_in = in_step["table_update"] * 1e-3 if (in_step and t_bwd and in_step["table_update"] > 0) else None
        t_step_dev = app.time_kernel(2 if trace else 4, 20 if B > 4096 else 100) * 1e-3 if solo else None
        t_lin_fwd = app.time_kernel(6, 20 if B > 4096 else 200) * 1e-3 if solo else None      # largest Linear layer alone: forward, backward (dX + dW)
        t_lin_bwd = app.time_kernel(7, 20 if B > 4096 else 100) * 1e-3 if solo else None
    uses_graph = app.model.uses_graph and trace
    backend = app.model.backend       # the kernel library the timed steps ran on (host/backend.cc honours --backend / $FFH_BACKEND_LIB)
    nbk = max(app.model.counter("allreduce_buckets"), 0)
    bucket_mb = [round(app.model.counter(f"allreduce_bucket_floats_{k}") * 4 / 1e6, 2) for k in range(nbk)]
    bucketed = app.model.counter("allreduce_bucket_calls") > 0
    grads = (f"gradients all-reduced in {nbk} buckets issued from inside backward() ({' + '.join(str(v) for v in bucket_mb)} MB, "
             f"{'a communicator of their own (ncclCommSplit)' if app.model.counter('allreduce_bucket_channel_own') == 1 else 'the all-to-alls communicator: held until the backward all-to-all is enqueued'})"
             if bucketed else "1 all-reduce of the gradient slab")
    grads += ("; each sum DIRECT: all-to-all of 1/N slices + local sum in rank order + all-gather (--direct-allreduce)" if app.model.counter("direct_allreduces") > 0
              else "; each sum by the transport's all-reduce (ring)")
    app.close()
    if world > 1:
        barrier()                                  # the probes above are rank 0's: nobody tears the group down under them

    if rank != 0:
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        return

    samples = w["B"] * args.steps
    wx = w.get("extra", [])
    layout = ("the table row-wise (partial bag sums + RCCL reduce-scatter fwd, all-gather bwd)" if "--row-shard-rows" in wx else
              "the table column-wise (RCCL all-to-all fwd+bwd)" if "--column-shard-rows" in wx else "tables table-wise, table t on rank t % N (RCCL all-to-all fwd+bwd)")
    if replicated:
        layout += f"; the {len(replicated)} tables of <= {args.replicate_embedding_rows} rows data-parallel (a copy per rank, dense gradients in the all-reduce bucket)"
    out = {
        "metric": "dlrm_training_samples_per_sec", "value": round(samples / elapsed, 1), "unit": "samples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "weak" if weak else "strong", "vs_baseline": None, **({"FUNCTIONAL_TEST_NOT_A_MEASUREMENT": True} if ftest else {}),
        "dtype": "f32" if not bf16 else "bf16 GEMM operands (fp32 accumulate, fp32 master weights); fp32 elsewhere", "data": "synthetic",
        "config": {"workload": f"{w['name']}: {T} tables (rows {w['rows']}), emb_dim {D}, bag 1, bot {w['bot']}, top {w['top']}, "
                               f"{'dot (strict lower triangle)' if 'dot-tril' in wx else 'dot (all pairs)' if 'dot' in wx else 'cat'} interaction, SGD lr 0.01, MSE loss",
                   "global_batch": w["B"], "per_gpu_batch": w["B"] // world,
                   "parallelism": ("single GPU, hipGraph-replayed step" if uses_graph else "single GPU, eager launches on 3 HIP streams") if world == 1 else
                                  f"{layout} over {world} ranks, MLPs data-parallel ({grads}); {collectives}",
                   "kernel_library": backend, "step_graph": bool(uses_graph), "step_us_graph_vs_eager": {k: round(v, 1) for k, v in step_us.items()}},
        "mse_over_timed_steps": round(2.0 * pm.mse_loss / max(pm.train_all, 1), 6),   # train_all is double-counted (1 class + accuracy), as in the reference
        # what "the same results as the reference" is held to in tests/ (the round-5 review asked for it on the line itself)
        "parity": ("index / integer work and the embedding kernels bit-exact against the oracle (gather: also against the reference's own AVX2 lookup); GEMMs: "
                   "|error| <= 1e-5 of the term mass (sum_k |a_k b_k|) + 1e-6 against the fp32 oracle -- the forward-error form of north_star's '1e-5 relative' "
                   "(a sum that cancels has no relative bound in any fp32 order); whole steps against torch-CPU golden vectors; tests/test_gpu_*.py"),
    }
    if world > 1 or args.force_exchange:
        out["config"]["ranks_observed"] = dist.get_world_size()
        out["config"]["collective_calls_rank0"] = calls
        out["config"]["gradient_allreduce"] = grads          # buckets, their communicator, ring or direct: what this run did (also part of `parallelism` at N > 1)
        # what one step moves over xGMI from / to rank 0 (payload, not counting RCCL's own protocol)
        def mlp_params(spec, first_in=None):
            dims = [int(v) for v in spec.split("-")]
            return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
        a2a = owned * B * D * 4 * (world - 1) // world if table_wise else None     # column- / row-wise layouts: not itemised here
        dense = mlp_params(w["bot"]) + mlp_params(w["top"]) + sum(rows_of[t] for t in replicated) * D
        out["config"]["collective_payload_bytes_per_step_rank0"] = {"alltoall_forward_sent": a2a, "alltoall_backward_sent": a2a,
                                                                    "allreduce_buffer": 4 * dense}
        if in_step:
            us = lambda d, k: round(d[k] * 1e3, 1)
            # what the collectives cost inside the step, so that a scaling record explains its own efficiency: each collective's own
            # interval on the stream it is issued on (side stream: both all-to-alls) and `embedding_branch_wait_us` = how long the compute stream stood at the join in front of the first
            # consumer of the embedding outputs -- the exposed part of [table update of the step before -> gather -> forward all-to-all]
            out["collectives_in_step_us"] = {
                "how": "HIP events around each call inside real eager steps, averaged; rank0 and max over ranks",
                "rank0": {"alltoall_fwd_us": us(in_step, "alltoall_fwd"), "alltoall_bwd_us": us(in_step, "alltoall_bwd"), "allreduce_us": us(in_step, "allreduce"),
                          "embedding_branch_wait_us": us(in_step, "join_wait"), "gather_plus_alltoall_fwd_us": us(in_step, "gather"),
                          "alltoall_bwd_plus_table_update_us": us(in_step, "table_update")},
                "max_over_ranks": {"alltoall_fwd_us": us(in_step_max, "alltoall_fwd"), "alltoall_bwd_us": us(in_step_max, "alltoall_bwd"), "allreduce_us": us(in_step_max, "allreduce"),
                                   "embedding_branch_wait_us": us(in_step_max, "join_wait"), "gather_plus_alltoall_fwd_us": us(in_step_max, "gather"),
                                   "alltoall_bwd_plus_table_update_us": us(in_step_max, "table_update")},
                # the MLP gradients' all-reduce goes out in buckets from inside backward() on a communication stream (round 5): each
                # bucket's own interval there, their sum, and what the compute stream stood waiting for them in front of the optimizer
                # (`allreduce_exposed_us`; `allreduce_us` above is what is left for update(): nothing, or the data-parallel tables)
                "allreduce_buckets_us": {"rank0": [us(in_step, f"bucket{i}") for i in range(8) if in_step.get(f"bucket{i}", 0) > 0],
                                         "max_over_ranks": [us(in_step_max, f"bucket{i}") for i in range(8) if in_step_max.get(f"bucket{i}", 0) > 0]},
                "allreduce_buckets_sum_us": round(sum(in_step_max.get(f"bucket{i}", 0) for i in range(8)) * 1e3, 1),
                "allreduce_exposed_us": us(in_step_max, "allreduce_wait"),
                "exposed_on_the_compute_stream_us": round((in_step_max["allreduce"] + in_step_max["allreduce_wait"] + in_step_max["join_wait"]) * 1e3, 1)}
    if args.force_exchange:
        out["config"]["parallelism"] = f"1 rank, exchange path forced: {layout} + all-reduce; {collectives}"
    if args.full:
        out["kernels"] = {}
    if t_fwd:
        key = args.workload if (world == 1 and w["B"] == DEFAULT_BATCH[args.workload]) else None
        pmc, src = pmc_traffic(key) if key else ({}, None)
        fwd_bytes = owned * B * (8 + 4 * D + 4 * D)            # indices + gathered rows + output write
        bwd_bytes = owned * B * (8 + 4 * D + 2 * 4 * D)        #            indices + out-grad read + row read-modify-write
        out["roofline"] = hbm_block("emb_fwd_kernel (embedding gather + bag-sum, this rank's tables in one launch)", fwd_bytes, t_fwd,
                                    pmc.get("gather_bytes_per_launch"), src, in_step_sec=t_fwd_in)
        out["roofline"]["bytes_per_sample"] = fwd_bytes // B
        out["roofline"]["tables_in_launch"] = owned
        out["kernels"]["embedding_bwd_sgd_fused"] = hbm_block(
            "radix_hist/radix_scatter (LDS-histogram stable radix passes on the ids) + emb_sgd_reduce (segmented sums, both folds by the last tile "
            "to arrive, W -= lr*sum); <= 64 K lookups per table: ONE pass on the top digit, the rest of the order per tile inside emb_sgd_reduce "
            "(3 launches); <= 2048: emb_sgd_small_kernel, one launch", bwd_bytes, t_bwd,
            pmc.get("update_bytes_per_call"), src, in_step_sec=t_bwd_in)
        sf = args.shim_flags.split()
        if "--early-sort" in sf or ("--no-early-sort" not in sf and (world > 1 or args.force_exchange or B // world < 8192)):
            out["kernels"]["embedding_bwd_sgd_fused"]["in_step_covers"] = (
                "the apply phase only (ffh_embedding_bwd_sgd_apply_multi): inside a step the index-only sort is issued behind the gather "
                "(ffh_embedding_bwd_sort_multi, --no-early-sort turns that off); us_per_launch above is the whole update, sort included")
        else:
            out["kernels"]["embedding_bwd_sgd_fused"]["in_step_covers"] = (
                "the whole update, sort + apply (one GPU, >= 8192 samples: the early sort is off by shape -- beside the top MLP's first forward GEMM "
                "it cost more than it saved; --early-sort forces it)")
    if solo and args.full:
        flops = mlp_flops_per_sample(w) * B
        peak = BF16_PEAK_TFLOPS if bf16 else F32_PEAK_TFLOPS
        out["kernels"]["linear_largest_layer"] = largest_linear(w, B, t_lin_fwd, t_lin_bwd, bf16)
        out["kernels"]["whole_step_device"] = {"us": round(t_step_dev * 1e6, 2), "mlp_gflop_per_step": round(flops / 1e9, 3),
                                               "mlp_tflops_over_whole_step": round(flops / t_step_dev / 1e12, 2), "mfma_peak_tflops": peak,
                                               "frac_of_mfma_peak": round(flops / t_step_dev / 1e12 / peak, 3)}
        if not args.no_secondary and not bf16 and not ftest:
            try:
                out["kernels"]["tensor_op_bf16_mode"] = bf16_mode_block(ffmodel, w, local_rank, B)
            except Exception as e:  # noqa: BLE001
                out["kernels"]["tensor_op_bf16_mode"] = {"error": repr(e)}
            # the fp32-accurate split mode: a SIBLING of the headline (same workload, same metric, same dtype contract), never the headline itself
            try:
                out["fp32_split"] = bf16_mode_block(ffmodel, w, local_rank, B, split=True)
            except Exception as e:  # noqa: BLE001
                out["fp32_split"] = {"error": repr(e)}
        if not args.no_secondary and args.workload != "kaggle" and not ftest:
            try:
                out["kernels"]["kaggle_secondary"] = kaggle_secondary(ffmodel, local_rank)
            except Exception as e:  # noqa: BLE001
                out["kernels"]["kaggle_secondary"] = {"error": repr(e)}
    if args.full and not args.no_cpu_baseline and not ftest and world == 1:
        # host only, rank 0, at N = 1 only (the contract): on the N > 1 lines the other ranks would stand in the closing barrier while rank 0's host cores run it
        out["cpu_baseline"] = cpu_baseline(args, budget_s=24.0)
    print(json.dumps(out), file=json_out, flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
