"""Shared by tests/test_checkpoint_cpu.py, tests/test_gpu_checkpoint.py and tests/_dist_worker_checkpoint.py: the tiny model of the
checkpoint tests (4 tables, batch 16, 64 samples), the three driver runs of an exact-resume check and the record-by-record comparison of
two checkpoint files."""
import os
import re
import subprocess

import numpy as np

from dlrm_flexflow_amd import ffmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")

# 4 tiny tables, batch 16, 64 samples: 4 batches an epoch (3 to train on where one is held out); concat width 4 + 4 x 4 = 20
MODEL = ["-b", "16", "--arch-sparse-feature-size", "4", "--arch-embedding-size", "30-20-10-40", "--arch-mlp-bot", "5-8-4",
         "--arch-mlp-top", "20-8-1", "--data-size", "64", "--synthetic-labels", "logistic", "--deterministic"]
# warm-up and decay both inside a 4-epoch run (13 to 17 optimizer steps)
SCHEDULE = ["--lr-num-warmup-steps", "3", "--lr-decay-start-step", "6", "--lr-num-decay-steps", "5"]
# what the HIP library adds (the CPU oracle has neither the CTR nor the data extension, so its runs cannot evaluate or shuffle)
EVAL = ["--loss", "bce", "--data-randomize", "total", "--eval-batches", "1"]


def run_driver(backend, *flags, exe=EXE, check=True):
    """One driver process on kernel library `backend` (None: the product's own)."""
    cmd = [exe] + (["--backend", backend] if backend else []) + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def abc(backend, tmp, flags, epochs=4, split=2, resume_flags=()):
    """The three runs of an exact-resume check: A trains `epochs` epochs and saves; B trains `split` and saves; C is a NEW process that loads B,
    trains on to `epochs` and saves.  Returns the three results and the three directories."""
    a, b, c = (os.path.join(str(tmp), d) for d in "ABC")
    ra = run_driver(backend, *flags, "--epochs", str(epochs), "--save-checkpoint", a)
    rb = run_driver(backend, *flags, "--epochs", str(split), "--save-checkpoint", b)
    rc = run_driver(backend, *flags, *resume_flags, "--epochs", str(epochs), "--load-checkpoint", b, f"--save-checkpoint={c}")
    return (ra, rb, rc), (a, b, c)


def assert_same_checkpoint(x, y):
    """Two checkpoint files agree record by record, bit for bit, and in every run field and digest."""
    cx, cy = ffmodel.read_checkpoint(x), ffmodel.read_checkpoint(y)
    mx, my = dict(cx["meta"]), dict(cy["meta"])
    mx.pop("path"), my.pop("path")
    assert list(mx["records"]) == list(my["records"]), (list(mx["records"]), list(my["records"]))
    for name in mx["records"]:
        assert cx[name].dtype == cy[name].dtype and cx[name].shape == cy[name].shape, name
        assert cx[name].tobytes() == cy[name].tobytes(), f"record {name} differs in {int((np.asarray(cx[name]) != np.asarray(cy[name])).sum())} elements"
    assert mx == my, {k: (mx[k], my.get(k)) for k in mx if mx[k] != my.get(k)}
    return cx


def assert_digests_hold(path):
    """Every record of the file has the digest its manifest line gives, and they add up to the manifest's own."""
    ck = ffmodel.read_checkpoint(path)
    total = 0
    for name, r in ck["meta"]["records"].items():
        got = ffmodel.state_digest_reference(ck[name], ffmodel.digest_record_seed(r["ordinal"]))
        assert got == r["digest"], name
        total = (total + got) % 2 ** 64
    assert total == ck["meta"]["digest"]
    return ck


def eval_lines(stdout, epochs):
    """the EVAL lines of the given epochs, the time field cut off"""
    out = []
    for e in epochs:
        hit = [re.sub(r" time [0-9.]+s$", "", l) for l in stdout.splitlines() if l.startswith(f"EVAL epoch {e}:")]
        assert len(hit) == 1, (e, stdout[-2000:])
        out.append(hit[0])
    return out
