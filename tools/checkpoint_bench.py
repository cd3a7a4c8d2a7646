#!/usr/bin/env python3
"""Timings behind DESIGN section 15 (checkpoint save / exact resume), appended to profiles/checkpoint_measurements.txt:

  python tools/checkpoint_bench.py digest         ffh_state_digest over the Terabyte shape's largest table (39,884,406 rows x 128), fp32 and bf16
                                                  storage, HIP events on the stream; the yardstick is an ffh_memcpy_d2d of the same bytes timed in
                                                  the same process (it reads AND writes them; the digest only reads)
  python tools/checkpoint_bench.py saveload       wall time of FFModel.save_checkpoint / load_checkpoint at the Kaggle shape and the bytes written
  python tools/checkpoint_bench.py bench          bench.py's own result line, to be run on this tree and on the parent commit alternately
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "checkpoint_measurements.txt")


def say(line):
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def digest_bench():
    import torch
    from dlrm_flexflow_amd import capi
    lib = capi.load_hip(0)
    dg = capi.digest_api(lib)
    rows, dim = 39884406, 128
    acc = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    for name, elem in (("fp32", 4), ("bf16", 2)):
        nbytes = rows * dim * elem
        src = torch.randint(0, 2 ** 31 - 1, (nbytes // 4,), dtype=torch.int32, device="cuda:0")
        dst = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn, reps=5):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            return ms
        t_d = timed(lambda: dg.state_digest(src.data_ptr(), rows, dim * elem, dim * elem, 7, 0, acc))
        t_c = timed(lambda: lib.call("ffh_memcpy_d2d", dst, src, nbytes, None))
        say(f"digest {name}: {rows} x {dim} = {nbytes / 1e9:.2f} GB  ffh_state_digest {min(t_d):.2f} ms min, {sorted(t_d)[len(t_d) // 2]:.2f} median "
            f"({nbytes / min(t_d) / 1e6:.0f} GB/s read)   ffh_memcpy_d2d of the same bytes {min(t_c):.2f} ms min, {sorted(t_c)[len(t_c) // 2]:.2f} median "
            f"({nbytes / min(t_c) / 1e6:.0f} GB/s read + as much written)   digest / copy = {min(t_d) / min(t_c):.2f}")
        del src, dst


def saveload_bench():
    import bench
    from dlrm_flexflow_amd import ffmodel
    w = bench.workload("kaggle", bench.DEFAULT_BATCH["kaggle"])
    flags = ["-b", str(w["B"]), "--arch-sparse-feature-size", str(w["D"]), "--arch-embedding-size", w["rows"], "--arch-mlp-bot", w["bot"],
             "--arch-mlp-top", w["top"], "--data-size", str(w["B"])]
    with tempfile.TemporaryDirectory() as d:
        app = ffmodel.DLRM(flags)
        app.warmup()
        for rep in range(3):
            t0 = time.perf_counter()
            app.model.save_checkpoint(d, 1)
            t1 = time.perf_counter()
            nbytes = os.path.getsize(os.path.join(d, "rank-0-of-1.ffck"))
            app.model.load_checkpoint(d)
            t2 = time.perf_counter()
            say(f"kaggle shape rep {rep}: save {t1 - t0:.3f} s, load (with the digest check of every record) {t2 - t1:.3f} s, {nbytes / 1e6:.1f} MB written "
                f"({nbytes / (t1 - t0) / 1e9:.2f} GB/s save, {nbytes / (t2 - t1) / 1e9:.2f} GB/s load; the file system is the temporary directory's)")
        t0 = time.perf_counter()
        app.model.state_digest()
        say(f"kaggle shape: FFModel.state_digest() {1e3 * (time.perf_counter() - t0):.2f} ms (one launch per record, one word copied out)")
        app.close()


def bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10"], capture_output=True, text=True,
                       timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not line:
        sys.exit(f"bench.py failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    j = json.loads(line[-1])
    say("bench.py --gpus 1 --steps 100 --warmup 10: " + json.dumps({k: j[k] for k in j if isinstance(j[k], (int, float, str))}))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "digest":
        digest_bench()
    elif what == "saveload":
        saveload_bench()
    elif what == "bench":
        bench_line()
    else:
        sys.exit(__doc__)
