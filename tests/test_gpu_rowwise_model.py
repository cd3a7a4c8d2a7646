"""--optimizer adagrad --adagrad-rowwise through the host layer on the GPU: the driver's dot and DCNv2 models against a torch
float64 twin (torch.optim.Adagrad on the dense parameters, the row-wise rule on the tables), bf16 tables and the start-up line's byte count, the
schedule under graph replay, and checkpoint / resume with the refusals between the two accumulator layouts.  Two ranks:
tests/test_gpu_rowwise_ranks.py.  The kernels alone are tests/test_gpu_rowwise.py."""
import os
import re

import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import adagrad_helpers as A
import checkpoint_helpers as K
import rowwise_helpers as R

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
ROWWISE = ["--optimizer", "adagrad", "--adagrad-rowwise"]

_TORCH = {}


@pytest.mark.parametrize("trace", [False, True], ids=["eager", "traced"])
@pytest.mark.parametrize("interaction", ["dot", "dcn"])
def test_dot_and_dcn_models_with_bce_equal_the_float64_twin(hip, tmp_path, interaction, trace):
    """The driver's model (8 tables, batch 128) with the dot interaction and with the DCNv2 cross network, --loss bce, 4 steps on the resident
    batch, against the same composition in torch float64: every parameter, every table's row state (shape `rows`) and the last prediction within
    the Adagrad model test's own bound (rtol 2e-5, atol 2e-6)."""
    got, exp = R.run_driver_model(HIP, interaction, 4, trace, want_torch=interaction not in _TORCH, directory=tmp_path / "ck")
    exp = _TORCH.setdefault(interaction, exp)
    assert set(got) == set(exp), set(got) ^ set(exp)
    states = [k for k in exp if k.startswith("S/")]
    assert len(states) == len(A.DRV_ROWS) and all(got[k].shape == (rows,) for k, rows in zip(sorted(states), A.DRV_ROWS))
    assert all(exp[k].max() > 0 for k in states)
    worst = {k: float(np.max(np.abs(got[k].astype(np.float64) - exp[k]) / (A.ATOL + A.RTOL * np.abs(exp[k])))) for k in exp}
    print(f"{interaction} {'traced' if trace else 'eager'}: largest |error| / (atol + rtol |expected|) per parameter: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    for k in sorted(exp):
        np.testing.assert_allclose(got[k].astype(np.float64), exp[k], rtol=A.RTOL, atol=A.ATOL, err_msg=k)


def test_bf16_tables_keep_one_float_per_row_and_the_start_up_line_counts_it(hip, tmp_path):
    """--embedding-dtype bf16 --embedding-rounding nearest: the row state is `rows` floats, the run ends with finite weights, and the start-up
    line's byte count is the dense slab's accumulator (every dense parameter on a whole number of 32 floats) plus 4 bytes per table row."""
    a = os.path.join(str(tmp_path), "a")
    flags = K.MODEL + ["--loss", "bce", "--embedding-dtype", "bf16", "--embedding-rounding", "nearest"] + ROWWISE
    r = K.run_driver(None, *flags, "--epochs", "2", "--save-checkpoint", a)
    ck = ffmodel.read_checkpoint(os.path.join(a, "rank-0-of-1.ffck"))
    rows = [30, 20, 10, 40]
    slab = 0
    for (i, o) in ((5, 8), (8, 4), (20, 8), (8, 1)):
        assert hip.lib.ffh_linear_fast_in_dim(i, o) == i      # (no kernel of this model is padded: its size is out x in)
        slab += (i * o + 31) // 32 * 32 + (o + 31) // 32 * 32
    want = 4 * slab + 4 * sum(rows)
    line = [l for l in r.stdout.splitlines() if l.startswith("[DLRM] optimizer: adagrad")]
    assert len(line) == 1 and "tables: fused row-wise, accumulator " in line[0], r.stdout[-3000:]
    assert int(re.search(r"accumulator (\d+) bytes", line[0]).group(1)) == want, (line[0], want)
    states = sorted(n for n in ck["meta"]["records"] if n.startswith("sparse_state0/"))
    assert [ck[n].shape for n in states] == [(rw, 1) for rw in rows] and all(ck[n].dtype == np.float32 for n in states)
    assert all(np.isfinite(ck[n]).all() and float(ck[n].max()) > 0 for n in states)
    for n, rec in ck["meta"]["records"].items():
        if n.startswith("param/"):
            w = np.array(ck[n])
            w = (w.astype(np.uint32) << 16).view(np.float32) if rec["type"] == "bf16" else w
            assert np.isfinite(w).all(), n
    assert sum(rec["type"] == "bf16" for rec in ck["meta"]["records"].values()) == 4
    assert ck["meta"]["optimizer"] == "adagrad-rowwise" and ck["meta"]["embedding_dtype"] == "bf16"


def test_without_the_flag_the_start_up_line_is_the_element_wise_one(hip):
    r = K.run_driver(None, *K.MODEL, "--loss", "bce", "--optimizer", "adagrad", "--epochs", "1")
    line = [l for l in r.stdout.splitlines() if l.startswith("[DLRM] optimizer: adagrad")]
    assert len(line) == 1 and ", tables: fused, accumulator " in line[0] and "row-wise" not in r.stdout, r.stdout[-3000:]


SCHEDULE = ["--lr-num-warmup-steps", "3", "--lr-decay-start-step", "3", "--lr-num-decay-steps", "12"]      # the rate changes on every one of the 13 steps


def test_scheduled_rate_replays_to_the_bits_of_the_eager_run(hip, tmp_path):
    """--deterministic --device-lr: 3 epochs of 4 steps, the last two replayed from the captured graph (--always-replay) against --no-trace: the
    same checkpoint record by record (weights, dense accumulators, row states, both learning-rate blocks), so the same state digest."""
    flags = K.MODEL + ["--loss", "bce", "--adagrad-initial-accumulator", "0.1", "--device-lr"] + ROWWISE + SCHEDULE
    a, b = os.path.join(str(tmp_path), "traced"), os.path.join(str(tmp_path), "eager")
    ra = K.run_driver(None, *flags, "--always-replay", "--epochs", "3", "--save-checkpoint", a)
    K.run_driver(None, *flags, "--no-trace", "--epochs", "3", "--save-checkpoint", b)
    assert "route=device" in ra.stdout and "[DLRM] optimizer: adagrad eps=1e-10 A=0.1" in ra.stdout and "tables: fused row-wise" in ra.stdout, ra.stdout[-3000:]
    ck = K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(b, "rank-0-of-1.ffck"))
    K.assert_digests_hold(os.path.join(a, "rank-0-of-1.ffck"))
    assert ck["meta"]["optimizer"] == "adagrad-rowwise" and ck["meta"]["lr_route"] == "device" and ck["meta"]["steps"] == 13
    names = set(ck["meta"]["records"])
    assert any(n.startswith("adagrad_s/") for n in names) and not any(n.startswith("sparse_state1/") for n in names)
    states = [n for n in names if n.startswith("sparse_state0/")]
    assert len(states) == 4 and all(ck[n].shape[1] == 1 for n in states)
    assert all(float(ck[n].min()) >= np.float32(0.1) and float(ck[n].max()) > np.float32(0.1) for n in states)


def test_resume_is_bit_exact_and_the_other_accumulator_layout_is_refused(hip, tmp_path):
    """4 epochs straight (A) against 2 epochs, save (B), a new process that loads B and trains to 4 (C), --deterministic: A and C agree record by
    record and in their digests; --eval-only --load-checkpoint evaluates it.  The row-wise checkpoint under plain --optimizer adagrad is refused,
    and an element-wise one under --adagrad-rowwise, both naming the flag."""
    flags = K.MODEL + K.SCHEDULE + K.EVAL + ROWWISE
    (ra, rb, rc), (a, b, c) = K.abc(None, tmp_path, flags)
    assert f"[DLRM] checkpoint: loaded {b} (epoch 2, step " in rc.stdout
    ck = K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))
    K.assert_digests_hold(os.path.join(c, "rank-0-of-1.ffck"))
    assert ck["meta"]["epochs_done"] == 4 and ck["meta"]["optimizer"] == "adagrad-rowwise" and ck["meta"]["table_optimizer"] == "sparse"
    assert K.eval_lines(ra.stdout, (3, 4)) == K.eval_lines(rc.stdout, (3, 4))
    states = [n for n in ck["meta"]["records"] if n.startswith("sparse_state0/")]
    assert len(states) == 4 and all(ck[n].shape == (rows, 1) for n, rows in zip(sorted(states), (30, 20, 10, 40)))
    r = K.run_driver(None, *flags, "--eval-only", "--load-checkpoint", c)
    assert "EVAL" in r.stdout, r.stdout[-2000:]
    # the other layout, both ways
    elementwise = [f for f in flags if f != "--adagrad-rowwise"]
    r = K.run_driver(None, *elementwise, "--epochs", "4", "--load-checkpoint", b, check=False)
    assert r.returncode != 0 and "FATAL: --load-checkpoint" in r.stderr and "add --adagrad-rowwise" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout
    e = os.path.join(str(tmp_path), "E")
    K.run_driver(None, *elementwise, "--epochs", "1", "--save-checkpoint", e)
    r = K.run_driver(None, *flags, "--epochs", "4", "--load-checkpoint", e, check=False)
    assert r.returncode != 0 and "FATAL: --load-checkpoint" in r.stderr and "drop --adagrad-rowwise" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout
