"""GPU tests of checkpoint save / exact resume: ffh_state_digest (include/ff_hip_digest.h) through the C-ABI against
ffmodel.state_digest_reference bit for bit -- every load width, unaligned bases, padded rows, more than one grid pass, indices above 2^32 --
and the driver on the HIP library: train n epochs against train k, save, load in a new process, train to n, record by record."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from dlrm_flexflow_amd import capi, ffmodel
import checkpoint_helpers as K

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256
M64 = 2 ** 64 - 1
ROW_BYTES = [2, 4, 6, 8, 26, 52, 64, 72, 4096]
ROWS = [0, 1, 3, 257, 70001]
INDEX_BASES = [0, 2 ** 32 - 5, 2 ** 40]
OFFSETS = [0, 2, 4, 8]                   # bytes from a 16-byte boundary: the 16-, 2-, 4- and 8-byte load forms
FFH_ERR_BAD_ARG = capi.FFH_ERR_BAD_ARG


@pytest.fixture(scope="module")
def digest(hip):
    """Every test goes through here first: a library without the extension fails the test plainly (capi.FFHError)."""
    return capi.digest_api(hip)


def lds(row_bytes):
    return [row_bytes, row_bytes + 2, (row_bytes // 128 + 1) * 128]


class Buf:
    """`rows` rows of row_bytes bytes, ld apart, `off` bytes behind a 16-byte boundary, inside a sentinel-filled device allocation with a guard
    region behind the last row; the rows' contents are copied in on the device."""

    def __init__(self, content, ld, off):
        rows, rb = content.shape
        self.n = 16 + off + rows * ld + GUARD
        self.dev = torch.full((self.n,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        assert self.dev.data_ptr() % 16 == 0
        if rows:
            torch.as_strided(self.dev, (rows, rb), (ld, 1), 16 + off).copy_(content)
        self.before = self.dev.clone()
        self.ptr = self.dev.data_ptr() + 16 + off

    def untouched(self):
        return torch.equal(self.dev, self.before)


def run(digest, acc, buf, rows, rb, ld, seed, index_base):
    acc.zero_()
    digest.state_digest(buf.ptr, rows, rb, ld, seed, index_base, acc)
    torch.cuda.synchronize()
    return int(acc.cpu().numpy().view(np.uint64)[0])


# ---- 1. the kernel against state_digest_reference, bit for bit ---------------------------------------------------------------------------
# Every row size with every row count, but for 70001 rows of 4096 bytes (287 MB a buffer, and as much for the numpy reference).  What 70001 rows are
# for is a walk longer than one grid pass (2048 workgroups x 256 lanes = 524288 positions): one position is 8 bytes in the 8-, 4- and 2-byte forms, so
# 70001 rows of 64 and 72 bytes pass it there (560008 and 630009), and 16 bytes in the 16-byte form, where 2053 rows of 4096 bytes do (525568).
SHAPES = [(rb, rows) for rb in ROW_BYTES for rows in ROWS if (rb, rows) != (4096, 70001)] + [(4096, 2053)]


@pytest.mark.parametrize("rb,rows", SHAPES)
def test_state_digest_equals_the_reference_bit_for_bit(digest, rb, rows):
    """Every leading dimension x base offset x index base of one (row_bytes, rows): the reference is computed once per index base from the
    rows' contents alone -- it knows nothing of ld or the base -- and pad bytes and the guard behind the buffer are sentinel before and after."""
    rng = np.random.default_rng(rb * 1000003 + rows)
    host = rng.integers(0, 256, (rows, rb), dtype=np.uint8)
    content = torch.from_numpy(host).to("cuda:0")
    seed = 0x5EED0000 + rb
    exp = {ib: ffmodel.state_digest_reference(host, seed, ib) if rows else 0 for ib in INDEX_BASES}
    acc = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    for ld in lds(rb):
        for off in OFFSETS:
            buf = Buf(content, ld, off)
            for ib in INDEX_BASES:
                got = run(digest, acc, buf, rows, rb, ld, seed, ib)
                assert got == exp[ib], f"rb {rb} rows {rows} ld {ld} off {off} index_base {ib}: 0x{got:016x} != 0x{exp[ib]:016x}"
            assert buf.untouched(), f"rb {rb} rows {rows} ld {ld} off {off}: the buffer, its pad bytes or the guard were written"


def test_pad_bytes_do_not_enter(digest):
    """the same rows between other pad bytes give the same word"""
    rb, rows, ld = 26, 257, 128
    host = np.random.default_rng(5).integers(0, 256, (rows, rb), dtype=np.uint8)
    content = torch.from_numpy(host).to("cuda:0")
    acc = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    a = Buf(content, ld, 0)
    d0 = run(digest, acc, a, rows, rb, ld, 9, 0)
    pads = torch.as_strided(a.dev, (rows, ld - rb), (ld, 1), 16 + rb)
    pads.copy_(torch.randint(0, 256, (rows, ld - rb), dtype=torch.uint8, device="cuda:0"))
    assert run(digest, acc, a, rows, rb, ld, 9, 0) == d0 == ffmodel.state_digest_reference(host, 9)


def test_acc_accumulates_and_five_launches_agree(digest):
    rb, rows = 72, 70001
    host = np.random.default_rng(6).integers(0, 256, (rows, rb), dtype=np.uint8)
    buf = Buf(torch.from_numpy(host).to("cuda:0"), rb, 0)
    acc = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    words = [run(digest, acc, buf, rows, rb, rb, 77, 2 ** 40) for _ in range(5)]
    assert len(set(words)) == 1 and words[0] == ffmodel.state_digest_reference(host, 77, 2 ** 40)
    # two tensors fold into one word with distinct seeds; the second call adds to what the first left
    acc.zero_()
    digest.state_digest(buf.ptr, rows, rb, rb, 77, 0, acc)
    digest.state_digest(buf.ptr, 257, rb, rb, 78, 0, acc)
    torch.cuda.synchronize()
    got = int(acc.cpu().numpy().view(np.uint64)[0])
    assert got == (ffmodel.state_digest_reference(host, 77) + ffmodel.state_digest_reference(host[:257], 78)) & M64
    # a large tensor in pieces: rows [0, a) + rows [a, n) with index_base = a W
    a, W = 30000, (rb + 7) // 8
    acc.zero_()
    digest.state_digest(buf.ptr, a, rb, rb, 77, 0, acc)
    digest.state_digest(buf.ptr + a * rb, rows - a, rb, rb, 77, a * W, acc)
    torch.cuda.synchronize()
    assert int(acc.cpu().numpy().view(np.uint64)[0]) == ffmodel.state_digest_reference(host, 77)


def test_bad_arguments_are_refused_and_launch_nothing(digest):
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    acc = torch.full((2,), 41, dtype=torch.int64, device="cuda:0")
    p, a = buf.data_ptr(), acc.data_ptr()
    bad = [(p, -1, 8, 8, a), (p, 4, 0, 8, a), (p, 4, 7, 8, a), (p, 4, 8, 6, a), (p, 4, 8, 9, a), (p + 1, 4, 8, 8, a), (p, 4, 8, 8, a + 4),
           (p, 4, 8, 8, None), (None, 4, 8, 8, a)]
    for base, rows, rb, ld, ac in bad:
        assert digest.state_digest_rc(base, rows, rb, ld, 1, 0, ac) == FFH_ERR_BAD_ARG, (rows, rb, ld)
    assert digest.state_digest_rc(None, 0, 8, 8, 1, 0, a) == 0          # rows == 0: a no-op, whatever the base
    torch.cuda.synchronize()
    assert acc.cpu().tolist() == [41, 41]


# ---- 2. the model: exact resume on the HIP library -----------------------------------------------------------------------------------------
CONFIGS = {
    "fp32-sgd": ["--optimizer", "sgd"],
    "bf16-sparse-adam-device-lr": ["--optimizer", "adam", "--embedding-dtype", "bf16", "--embedding-rounding", "stochastic", "--sparse-embedding-optimizer",
                                   "--device-lr"],
    "dcn-1-layer": ["--optimizer", "sgd", "--arch-interaction-op", "dcn", "--dcn-num-layers", "1", "--dcn-low-rank-dim", "4"],
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_resume_is_bit_exact_on_the_hip_library(hip, tmp_path, config):
    """4 epochs straight (A) against 2 epochs, save (B), a new process that loads B and trains to 4 (C), --deterministic: A and C agree record by
    record, bit for bit, in every run field and digest, and their EVAL lines of epochs 3 and 4 are identical up to the time field.  The state
    digest of a model that loaded C, computed on the device, is the fold of C's manifest digests."""
    flags = K.MODEL + K.SCHEDULE + K.EVAL + CONFIGS[config]
    (ra, rb, rc), (a, b, c) = K.abc(None, tmp_path, flags)
    assert f"[DLRM] checkpoint: loaded {b} (epoch 2, step " in rc.stdout and "[DLRM] checkpoint: none" in ra.stdout
    ck = K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))
    K.assert_digests_hold(os.path.join(c, "rank-0-of-1.ffck"))
    assert ck["meta"]["epochs_done"] == 4 and ck["meta"]["steps"] == 13
    assert K.eval_lines(ra.stdout, (3, 4)) == K.eval_lines(rc.stdout, (3, 4))
    if config.startswith("bf16"):
        assert ck["meta"]["lr_route"] == "device" and {"lr_block/0", "lr_block/1", "bf16_counter"} <= set(ck["meta"]["records"])
        assert int(ck["bf16_counter"][0, 0]) == 13
        assert any(n.startswith("sparse_state1/") for n in ck["meta"]["records"])
    app = ffmodel.DLRM(flags + ["--epochs", "4", "--load-checkpoint", c])
    try:
        assert app.model.state_digest() == ck["meta"]["digest"]
    finally:
        app.close()


def test_traced_resume_gives_the_bits_of_the_eager_run(hip, tmp_path):
    """The resumed process starts at epoch 2 >= 1, so it traces at once (--always-replay: every traced step is a graph replay); the straight run
    never traces (--no-trace).  Same bits."""
    flags = K.MODEL + K.SCHEDULE + K.EVAL + ["--optimizer", "sgd"]
    a, b, c = (os.path.join(str(tmp_path), d) for d in "ABC")
    ra = K.run_driver(None, *flags, "--no-trace", "--epochs", "4", "--save-checkpoint", a)
    K.run_driver(None, *flags, "--no-trace", "--epochs", "2", "--save-checkpoint", b)
    rc = K.run_driver(None, *flags, "--always-replay", "--epochs", "4", "--load-checkpoint", b, "--save-checkpoint", c)
    K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))
    assert K.eval_lines(ra.stdout, (3, 4)) == K.eval_lines(rc.stdout, (3, 4))


def test_a_flipped_byte_is_reported_by_the_device_digest(hip, tmp_path):
    flags = K.MODEL + K.EVAL + ["--optimizer", "sgd"]
    b = os.path.join(str(tmp_path), "B")
    K.run_driver(None, *flags, "--epochs", "1", "--save-checkpoint", b)
    path = os.path.join(b, "rank-0-of-1.ffck")
    ck = ffmodel.read_checkpoint(path)
    name = "param/Embedding_104/0"
    data_start = (24 + int.from_bytes(open(path, "rb").read(24)[16:24], "little") + 4095) // 4096 * 4096
    with open(path, "r+b") as f:
        f.seek(data_start + ck["meta"]["records"][name]["offset"] + 5)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 0x10]))
    r = K.run_driver(None, *flags, "--epochs", "2", "--load-checkpoint", b, check=False)
    assert r.returncode != 0 and "FATAL: --load-checkpoint" in r.stderr and f"record {name} does not match its digest" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout


def test_another_schedule_is_refused_on_the_device_lr_route(hip, tmp_path):
    """On the device route the saved blocks carry their schedule, so the manifest names it and a resume under any other one is refused -- also
    where the two schedules agree at the step the file stands at (step 4 of 13: past the warm-up, before the decay starts)."""
    flags = K.MODEL + K.EVAL + ["--optimizer", "sgd", "--device-lr"]
    b = os.path.join(str(tmp_path), "B")
    K.run_driver(None, *flags, *K.SCHEDULE, "--epochs", "1", "--save-checkpoint", b)
    meta = ffmodel.read_checkpoint(b)["meta"]
    assert meta["lr_route"] == "device" and meta["steps"] == 4
    assert {k: meta["lr_schedule"][k] for k in ("warmup_steps", "decay_start", "decay_steps")} == {"warmup_steps": 3, "decay_start": 6, "decay_steps": 5}
    other = [f if f != "5" else "7" for f in K.SCHEDULE]                    # --lr-num-decay-steps 7
    r = K.run_driver(None, *flags, *other, "--epochs", "2", "--load-checkpoint", b, check=False)
    assert r.returncode != 0 and "FATAL: --load-checkpoint" in r.stderr and "--lr-num-decay-steps 5" in r.stderr and "give the same" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout
    K.run_driver(None, *flags, *K.SCHEDULE, "--epochs", "2", "--load-checkpoint", b)


def test_eval_only_evaluates_the_loaded_model_and_another_table_type_is_refused(hip, tmp_path):
    """--eval-only --load-checkpoint prints the EVAL line of the run that saved, under its epoch number; bf16 tables do not load into fp32 ones."""
    flags = K.MODEL + K.EVAL + ["--optimizer", "sgd", "--embedding-dtype", "bf16"]
    b = os.path.join(str(tmp_path), "B")
    rb = K.run_driver(None, *flags, "--epochs", "2", "--save-checkpoint", b)
    re_ = K.run_driver(None, *flags, "--eval-only", "--load-checkpoint", b)
    assert K.eval_lines(re_.stdout, (2,)) == K.eval_lines(rb.stdout, (2,))
    assert "THROUGHPUT" not in re_.stdout
    fp32 = [f for f in flags if f not in ("--embedding-dtype", "bf16")]
    r = K.run_driver(None, *fp32, "--epochs", "3", "--load-checkpoint", b, check=False)
    assert r.returncode != 0 and "it holds bf16 tables, this run has --embedding-dtype fp32" in r.stderr and "use --embedding-dtype bf16" in r.stderr, r.stderr[-2000:]


def _two_ranks(tmp_path, mode, ckdir):
    worker = os.path.join(ROOT, "tests", "_dist_worker_checkpoint.py")
    port = str(30100 + os.getpid() % 300 + (1 if mode == "load" else 0))
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, worker, "gpu", mode, str(tmp_path), ckdir], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(str(tmp_path), f"{mode}-rank{r}.npz")) for r in range(2)]


def test_two_ranks_sharing_the_gpu_save_and_load(hip, tmp_path):
    """Two ranks on one GPU (host-staged test transport): each saves its file; two new ranks load them, and each one's state digest, computed on
    the device, is its file's."""
    ckdir = os.path.join(str(tmp_path), "ck")
    saved = _two_ranks(tmp_path, "save", ckdir)
    assert sorted(os.listdir(ckdir)) == ["rank-0-of-2.ffck", "rank-1-of-2.ffck"]
    loaded = _two_ranks(tmp_path, "load", ckdir)
    for r in range(2):
        ck = K.assert_digests_hold(os.path.join(ckdir, f"rank-{r}-of-2.ffck"))
        assert ck["meta"]["world_size"] == 2 and ck["meta"]["rank"] == r
        assert int(saved[r]["digest"]) == int(loaded[r]["digest"]) == ck["meta"]["digest"]
        assert int(loaded[r]["epochs_done"]) == 1
