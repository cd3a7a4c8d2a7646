"""GPU tests (-m gpu) of --eval-embedding-dtype int8 through the host model, on small Kaggle-like models.

The yardstick everywhere: a second model that evaluates with fp32 tables whose gathered tables were set() to
q8_dequantize_reference(q8_quantize_reference(get())).  The int8 gather gives the bits of the fp32 gather on the dequantized table
(tests/test_gpu_q8.py), so samples, the log-loss sum and both AUC histograms must be EQUAL, not close."""
import os
import re
import subprocess

import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import fold_helpers as FH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm")
INT8 = ["--eval-embedding-dtype", "int8"]
NT, B, D = 8, 128, 16
BASE = ["-ll:gpu", "1", "-b", str(B), "--arch-sparse-feature-size", str(D), "--arch-embedding-size", "-".join(["1000"] * NT),
        "--arch-mlp-bot", f"13-64-{D}", "--arch-mlp-top", f"{D * (NT + 1)}-64-1", "--data-size", str(B * 12), "--loss", "bce", "--eval-batches", "4",
        "--deterministic", "--lr", "0.1"]
MIXED = ["--embedding-bag-sizes", "1-3-2-7-1-1-12-5"]
EVAL_LINE = re.compile(r"^EVAL epoch (\d+): samples (\d+) logloss ([\d.]+) accuracy ([\d.]+) auc ([\d.]+|nan) time [\d.]+s$", re.M)
START_LINE = re.compile(r"^\[DLRM\] eval tables: int8 rows \(row_bytes (\d+)\), (\d+) bytes beside (\d+) bytes of tables, (\d+) folded tables keep fp32$", re.M)


def _tables(m):
    """(layer index, parameter) of every embedding table, in model order"""
    return [(li, m.parameter(li, 0)) for li in range(m.num_layers) if m.layer_name(li).startswith("Embedding")]


def _dequantized(w):
    return ffmodel.q8_dequantize_reference(*ffmodel.q8_quantize_reference(w))


def _evaluate(app):
    app.evaluate(0)
    e = app.model.eval_metrics(histograms=True)
    return {k: e[k] for k in ("samples", "positives", "correct", "logloss_sum", "hist_pos", "hist_neg")}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, a[k], b[k])
    assert a["samples"] > 0 and int(a["hist_pos"].sum() + a["hist_neg"].sum()) == a["samples"]


def _reference_eval(flags, tables_from=None, only=None):
    """The yardstick: the model of `flags` without the int8 flag, its tables (all, or those `only` picks by row count) replaced by their dequantized
    images -- of its own values, or of `tables_from` (a list of fp32 arrays in table order) -- and evaluated with fp32 tables."""
    app = ffmodel.DLRM(flags)
    m = app.model
    for k, (li, p) in enumerate(_tables(m)):
        w = p.get() if tables_from is None else tables_from[k]
        if only is None or only(w.shape[0]):
            p.set(_dequantized(w))
        elif tables_from is not None:
            p.set(w)
    assert m.counter("q8_gather_launches") == 0 and m.counter("q8_quantize_launches") == 0
    e = _evaluate(app)
    n_ragged = m.counter("ragged_gather_launches")
    assert m.counter("q8_gather_launches") == 0
    app.close()
    return e, n_ragged


def test_uniform_bags_equal_fp32_evaluation_of_the_dequantized_tables(hip):
    flags = BASE + ["--no-fold-small-tables"]
    app = ffmodel.DLRM(flags + INT8)
    m = app.model
    got = _evaluate(app)
    assert m.counter("q8_quantize_launches") == 1 and m.counter("q8_gather_launches") == 4 and m.counter("folded_tables") == 0      # 4 held-out batches, one group
    again = _evaluate(app)                                          # nothing wrote a table: the images are current
    assert m.counter("q8_quantize_launches") == 1 and m.counter("q8_gather_launches") == 8
    app.close()
    ref, _ = _reference_eval(flags)
    _same(got, ref, "uniform")
    _same(again, ref, "uniform, second evaluation")
    plain, _ = _reference_eval(flags, only=lambda rows: False)     # the flag is not a no-op: fp32 tables give other figures
    assert plain["logloss_sum"] != got["logloss_sum"]


@pytest.mark.parametrize("extra", [[], ["--no-ragged-gather"]], ids=["ragged", "per-bag-size"])
def test_mixed_bags_equal_fp32_evaluation_of_the_dequantized_tables(hip, extra):
    flags = BASE + MIXED + extra
    app = ffmodel.DLRM(flags + INT8)
    m = app.model
    got = _evaluate(app)
    n_q8, n_ragged_here = m.counter("q8_gather_launches"), m.counter("ragged_gather_launches")
    app.close()
    ref, n_ragged = _reference_eval(flags)
    _same(got, ref, f"mixed {extra}")
    assert n_ragged_here == 0                                      # every table of the evaluation came from its image
    if not extra:
        assert n_q8 == n_ragged == 4                                # the launches of the ragged fp32 gather: one per held-out batch
    else:
        assert n_ragged == 0 and n_q8 == 4 * len(set(MIXED[1].split("-")))      # one launch per bag size


def test_folded_tables_keep_their_fp32_path(hip):
    """The model of the fold tests (6 tables of 3-5000-1-40-70000-300 rows, D = 32, batch 512): the tables the first top layer reads as products
    (4 R <= 3 batch: 3, 1, 40 and 300 rows) have no image and are evaluated from fp32 as before; the other two are replaced in the yardstick."""
    flags = FH.model_args(["--loss", "bce", "--eval-batches", "2", "--deterministic"])
    flags[flags.index("--data-size") + 1] = str(FH.MODEL_B * 4)
    small = lambda rows: 4 * rows <= 3 * FH.MODEL_B
    app = ffmodel.DLRM(flags + INT8)
    m = app.model
    nfold = m.counter("folded_tables")
    assert nfold == sum(small(r) for r in FH.MODEL_ROWS) > 0
    got = _evaluate(app)
    assert m.counter("q8_gather_launches") == 2 and m.counter("q8_quantize_launches") == 1
    app.close()
    ref, _ = _reference_eval(flags, only=lambda rows: not small(rows))
    _same(got, ref, "fold")


def _params(m):
    return {f"{m.layer_name(li)}/{wi}": m.parameter(li, wi).get() for li in range(m.num_layers) for wi in range(m.layer_num_weights(li))}


def test_images_follow_the_tables_through_training(hip):
    """Evaluate, train (one eager step, then traced steps of which at least one is a replayed graph), evaluate again: the second evaluation sees
    the tables as they are then, after exactly one more quantizer launch (one group), and training is bit for bit what it is without the flag."""
    flags = BASE + ["--no-fold-small-tables", "--always-replay"]

    def train(app):
        app.warmup()
        app.train_steps(1, trace=False)
        app.train_steps(3, trace=True)
        app.model.sync()

    app = ffmodel.DLRM(flags + INT8)
    m = app.model
    first = _evaluate(app)
    q0 = m.counter("q8_quantize_launches")
    train(app)
    assert m.counter("graph_replays") >= 1 and m.counter("q8_quantize_launches") == q0 == 1      # training never touches the images
    second = _evaluate(app)
    assert m.counter("q8_quantize_launches") == q0 + 1
    trained = _params(m)
    # set() on a table makes the images stale as well
    li, p = _tables(m)[0]
    p.set(np.zeros_like(p.get()))
    zeroed = _evaluate(app)
    assert m.counter("q8_quantize_launches") == q0 + 2 and zeroed["logloss_sum"] != second["logloss_sum"]
    # ... and set() on anything that is no table with an image does not: a caller that feeds held-out batches with set() pays no quantizer pass per batch
    m.parameter(0, 1).set(m.parameter(0, 1).get())
    app.dense_input().set(app.dense_input().get())
    same = _evaluate(app)
    assert m.counter("q8_quantize_launches") == q0 + 2 and same["logloss_sum"] == zeroed["logloss_sum"]
    app.close()

    ref_app = ffmodel.DLRM(flags)
    train(ref_app)
    ref_trained = _params(ref_app.model)
    assert ref_trained.keys() == trained.keys()
    for k in trained:
        assert trained[k].tobytes() == ref_trained[k].tobytes(), f"{k}: training with the flag differs from training without it"
    for li, p in _tables(ref_app.model):
        p.set(_dequantized(p.get()))
    ref = _evaluate(ref_app)
    ref_app.close()
    _same(second, ref, "after training")
    assert first["logloss_sum"] != second["logloss_sum"]


def test_load_checkpoint_leaves_the_images_stale(hip, tmp_path):
    """Through the Python API: save, evaluate, train on, evaluate (other figures), load the checkpoint, evaluate: the figures of the first evaluation
    again, after exactly one more quantizer launch -- the loader's writes of the tables are what marked the images."""
    app = ffmodel.DLRM(BASE + ["--no-fold-small-tables", "--no-trace"] + INT8)
    m = app.model
    app.warmup()
    app.train_steps(1, trace=False)
    m.save_checkpoint(str(tmp_path / "ck"))
    saved = _evaluate(app)
    app.train_steps(2, trace=False)
    moved = _evaluate(app)
    q = m.counter("q8_quantize_launches")
    assert q == 2 and moved["logloss_sum"] != saved["logloss_sum"]
    m.load_checkpoint(str(tmp_path / "ck"))
    back = _evaluate(app)
    assert m.counter("q8_quantize_launches") == q + 1
    app.close()
    _same(back, saved, "after load_checkpoint")


def test_bf16_tables_are_widened_exactly(hip):
    """int8 evaluation of a bf16-table model equals int8 evaluation of an fp32-table model that holds the widened values."""
    flags = BASE + ["--no-fold-small-tables"]
    app = ffmodel.DLRM(flags + ["--embedding-dtype", "bf16"] + INT8)
    wide = [p.get() for _, p in _tables(app.model)]                 # bf16 tables come out widened
    got = _evaluate(app)
    assert app.model.counter("q8_quantize_launches") == 1
    app.close()
    app = ffmodel.DLRM(flags + INT8)
    for (li, p), w in zip(_tables(app.model), wide):
        p.set(w)
    ref = _evaluate(app)
    app.close()
    _same(got, ref, "bf16")
    ref32, _ = _reference_eval(flags, tables_from=wide)             # ... and the fp32 evaluation of the dequantized widened tables
    _same(got, ref32, "bf16 against fp32 evaluation")


def test_driver_evaluates_a_checkpoint_with_int8_tables(hip, tmp_path):
    ck = str(tmp_path / "ck")
    r = subprocess.run([EXE, *BASE, "--epochs", "1", "--save-checkpoint", ck], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "eval tables" not in r.stdout and len(EVAL_LINE.findall(r.stdout)) == 1
    runs = {}
    for name, extra in (("fp32", []), ("int8", INT8), ("int8=", ["--eval-embedding-dtype=int8"])):
        r = subprocess.run([EXE, *BASE, "--eval-only", "--load-checkpoint", ck, *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = EVAL_LINE.findall(r.stdout)
        assert len(lines) == 1 and lines[0][1] == str(4 * B), r.stdout[-2000:]
        runs[name] = lines[0]
        start = START_LINE.findall(r.stdout)
        if name == "fp32":
            assert not start
            continue
        assert len(start) == 1, r.stdout[-2000:]
        rb, nbytes, tbytes, folded = (int(v) for v in start[0])
        assert rb == D + 8 and nbytes == NT * 1000 * (D + 8) and tbytes == NT * 1000 * D * 4 and folded == 0
    assert runs["int8"] == runs["int8="]
    assert abs(float(runs["int8"][2]) - float(runs["fp32"][2])) < 0.05      # 8 bits per element move the held-out log-loss, a little
