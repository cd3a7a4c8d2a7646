"""--optimizer adagrad through the host layer on the GPU: the fused table route against the dense one, the golden DLRM and
the driver's dot and DCNv2 models against torch.optim.Adagrad in float64, the weights' twin and three-plane image behind a model step, the
schedule under graph replay, and checkpoint / resume.  Two ranks: tests/test_gpu_adagrad_ranks.py.  The kernels alone are
tests/test_gpu_adagrad.py."""
import os

import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import adagrad_helpers as A
import checkpoint_helpers as K
import dlrm_helpers as H

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
HP = dict(lr=0.05, weight_decay=0.0, epsilon=1e-10, initial_accumulator=0.0)


# ---- 9. the fused path is the dense path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [0.0, 0.1])
def test_fused_table_update_equals_the_dense_path_bit_for_bit(hip, acc):
    """3 steps with the tables on the sorted-segments update (the default for Adagrad without weight decay) and again with
    --dense-embedding-update (zero, scatter-add, ffh_adagrad_update over every row).  Distinct ids per table: no atomics order to differ in;
    --deterministic: the MLP gradients have none either.  Tables, MLPs and predictions end in the same bits."""
    g = A.distinct_id_fixture()
    hp = dict(HP, initial_accumulator=acc)
    recs = []
    for dense in (False, True):
        m, h = A.build_dlrm(HIP, g, hp, argv=["--deterministic"], dense_update=dense)
        recs.append(H.run_steps(m, h, 3))
        m.close()
    for step in range(3):
        for k in recs[0][step]:
            assert recs[0][step][k].tobytes() == recs[1][step][k].tobytes(), f"step {step} {k}"
    # the tables did move, and only in the rows the batch hit
    for t, R in enumerate(g["rows"]):
        moved = (recs[0][2][f"emb.{t}.weight"] != g[f"init/emb.{t}.weight"]).any(axis=1)
        hit = np.zeros(R, bool)
        hit[g[f"sparse{t}"].ravel()] = True
        assert moved.any() and not (moved & ~hit).any()


# ---- 10 (the concat model of the Adam test's harness). the whole model against torch ---------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "traced"])
@pytest.mark.parametrize("wd,acc", [(0.0, 0.0), (1e-3, 0.1)], ids=["fused_tables", "wd_dense_tables"])
def test_golden_dlrm_equals_torch_adagrad_float64(hip, graph, wd, acc):
    """The golden DLRM of test_adam_optimizer_matches_torch_on_gpu for 4 steps against torch.optim.Adagrad (float64, CPU) at that test's own
    bound (rtol 2e-5, atol 2e-6).  Without weight decay the tables take the fused route, with it the dense one."""
    g = H.golden("dlrm_step_torch")
    hp = dict(HP, lr=0.02, weight_decay=wd, initial_accumulator=acc)
    m, h = A.build_dlrm(HIP, g, hp, enable_graph=graph)
    recs = H.run_steps(m, h, 4, trace=graph)
    m.close()
    exp = A.torch_adagrad_reference(g, 4, hp["lr"], wd, hp["epsilon"], acc)
    for step in range(4):
        for k in recs[step]:
            np.testing.assert_allclose(recs[step][k].astype(np.float64), exp[step][k], rtol=2e-5, atol=2e-6, err_msg=f"step {step} {k}")


_TORCH = {}


@pytest.mark.parametrize("trace", [False, True], ids=["eager", "traced"])
@pytest.mark.parametrize("interaction", ["dot", "dcn"])
def test_dot_and_dcn_models_with_bce_equal_torch_adagrad_float64(hip, interaction, trace):
    """The driver's model (8 tables, batch 128) with the dot interaction and with the DCNv2 cross network (2 layers, rank 8), --loss bce,
    --optimizer adagrad, 4 steps on the resident batch, against the same composition in torch float64 under torch.optim.Adagrad: every
    parameter -- the cross layers' V, W and b among them -- and the last prediction within the Adam test's own bound (rtol 2e-5, atol 2e-6)."""
    got, exp = A.run_driver_model(HIP, interaction, 4, trace, want_torch=interaction not in _TORCH)
    exp = _TORCH.setdefault(interaction, exp)
    assert set(got) == set(exp), set(got) ^ set(exp)
    worst = {k: float(np.max(np.abs(got[k].astype(np.float64) - exp[k]) / (A.ATOL + A.RTOL * np.abs(exp[k])))) for k in exp}
    print(f"{interaction} {'traced' if trace else 'eager'}: largest |error| / (atol + rtol |expected|) per parameter: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    for k in sorted(exp):
        np.testing.assert_allclose(got[k].astype(np.float64), exp[k], rtol=A.RTOL, atol=A.ATOL, err_msg=k)


# ---- 14. the weights' mirrors in the bf16-pipe modes, through the model -----------------------------------------------------------------------
_MIRROR_MODELS = {
    # Kaggle widths: 432 -> 512 and 512 -> 256 read the weights' twin
    "tensor-op": H.KAGGLE_ARGS(2048) + ["--allow-tensor-op-math-conversion"],
    # layers big enough for the split mode to take them (tests/test_gpu_round4.py)
    "split": ["-b", "16384", "--arch-sparse-feature-size", "128", "--arch-embedding-size", "3000-700", "--arch-mlp-bot", "13-256-128",
              "--arch-mlp-top", "384-1024-512-1", "--data-size", "16384", "--fp32-split-bf16x3"],
}


@pytest.mark.parametrize("device_lr", [False, True], ids=["scalar", "device-lr"])
@pytest.mark.parametrize("mode", sorted(_MIRROR_MODELS))
def test_model_step_leaves_the_weight_twin_and_image_current(hip, mode, device_lr):
    """One Adagrad step behind the warm-up step in tensor-op mode and in --fp32-split-bf16x3: the bf16 twin / three-plane image the host layer
    registered for the weight slab equals a fresh conversion of the updated fp32 weights, bit for bit (FFModel.weight_mirror_stale_bytes).
    A host write of the slab is reported as pending (-2), not as current."""
    app = ffmodel.DLRM(["--backend", HIP] + _MIRROR_MODELS[mode] + ["--optimizer", "adagrad", "--no-trace"] + (["--device-lr"] if device_lr else []))
    try:
        m = app.model
        app.warmup()
        app.train_steps(1, trace=False)
        w0 = m.parameter(0, 0).get_weights()
        assert m.weight_mirror_stale_bytes() == 0
        app.train_steps(1, trace=False)
        assert m.weight_mirror_stale_bytes() == 0
        assert not np.array_equal(m.parameter(0, 0).get_weights(), w0)          # the weights did move
        # a host write to the slab: the mirror is stale until the next step reconverts it, and the check says so
        lay = [l for l in range(m.num_layers) if m.layer_name(l).startswith("Dense")][-2]
        p = m.parameter(lay, 0)
        p.set_weights((p.get_weights() * 1.5).astype(np.float32))
        assert m.weight_mirror_stale_bytes() == -2
    finally:
        app.close()


# ---- 11. the schedule under capture --------------------------------------------------------------------------------------------------------
SCHEDULE = ["--lr-num-warmup-steps", "3", "--lr-decay-start-step", "3", "--lr-num-decay-steps", "12"]      # the rate changes on every one of the 13 steps


@pytest.mark.parametrize("interaction", ["cat", "dcn"])
def test_scheduled_rate_replays_to_the_bits_of_the_eager_run(hip, tmp_path, interaction):
    """--deterministic --device-lr: 3 epochs of 4 steps, the last two replayed from the captured graph (--always-replay) against --no-trace:
    the same checkpoint record by record (weights, accumulators, both learning-rate blocks), so the same state digest."""
    flags = K.MODEL + ["--loss", "bce", "--optimizer", "adagrad", "--adagrad-initial-accumulator", "0.1", "--device-lr"] + SCHEDULE
    if interaction == "dcn":
        flags += ["--arch-interaction-op", "dcn", "--dcn-num-layers", "1", "--dcn-low-rank-dim", "4"]
    a, b = os.path.join(str(tmp_path), "traced"), os.path.join(str(tmp_path), "eager")
    ra = K.run_driver(None, *flags, "--always-replay", "--epochs", "3", "--save-checkpoint", a)
    K.run_driver(None, *flags, "--no-trace", "--epochs", "3", "--save-checkpoint", b)
    assert "route=device" in ra.stdout and "[DLRM] optimizer: adagrad eps=1e-10 A=0.1" in ra.stdout and "tables: fused" in ra.stdout, ra.stdout[-3000:]
    ck = K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(b, "rank-0-of-1.ffck"))
    assert ck["meta"]["optimizer"] == "adagrad" and ck["meta"]["lr_route"] == "device" and ck["meta"]["steps"] == 13
    names = set(ck["meta"]["records"])
    assert any(n.startswith("adagrad_s/") for n in names) and any(n.startswith("sparse_state0/") for n in names)
    assert not any(n.startswith("sparse_state1/") for n in names)
    s = next(n for n in names if n.startswith("sparse_state0/"))
    assert float(ck[s].min()) >= np.float32(0.1) and float(ck[s].max()) > np.float32(0.1)


# ---- 12. checkpoint ----------------------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "fp32": [],
    "bf16-stochastic": ["--embedding-dtype", "bf16", "--embedding-rounding", "stochastic"],
    "bf16-nearest": ["--embedding-dtype", "bf16", "--embedding-rounding", "nearest"],
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_resume_is_bit_exact_and_another_optimizer_is_refused(hip, tmp_path, config):
    """4 epochs straight (A) against 2 epochs, save (B), a new process that loads B and trains to 4 (C), --deterministic: A and C agree record
    by record and in their digests.  The same checkpoint under --optimizer adam is refused, naming the optimizer to use."""
    flags = K.MODEL + K.SCHEDULE + K.EVAL + ["--optimizer", "adagrad"] + CONFIGS[config]
    (ra, rb, rc), (a, b, c) = K.abc(None, tmp_path, flags)
    assert f"[DLRM] checkpoint: loaded {b} (epoch 2, step " in rc.stdout
    ck = K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))
    K.assert_digests_hold(os.path.join(c, "rank-0-of-1.ffck"))
    assert ck["meta"]["epochs_done"] == 4 and ck["meta"]["steps"] == 13 and ck["meta"]["optimizer"] == "adagrad" and ck["meta"]["table_optimizer"] == "sparse"
    assert K.eval_lines(ra.stdout, (3, 4)) == K.eval_lines(rc.stdout, (3, 4))
    names = set(ck["meta"]["records"])
    assert sum(n.startswith("sparse_state0/") for n in names) == 4 and any(n.startswith("adagrad_s/") for n in names)
    if config.startswith("bf16"):
        assert int(ck["bf16_counter"][0, 0]) == 13
    app = ffmodel.DLRM(flags + ["--epochs", "4", "--load-checkpoint", c])
    try:
        assert app.model.state_digest() == ck["meta"]["digest"]
    finally:
        app.close()
    other = [f if f != "adagrad" else "adam" for f in flags] + (["--sparse-embedding-optimizer"] if config.startswith("bf16") else [])
    r = K.run_driver(None, *other, "--epochs", "4", "--load-checkpoint", b, check=False)
    assert r.returncode != 0 and "FATAL: --load-checkpoint" in r.stderr and "--optimizer adagrad" in r.stderr, r.stderr[-2000:]
    assert "THROUGHPUT" not in r.stdout


def test_weight_decay_sends_the_tables_down_the_dense_path_unless_asked(hip):
    """The routing of FFModel::fused_embedding_update for Adagrad, seen through what a step leaves: with weight decay every row of a table
    decays (dense sweep); with --sparse-embedding-optimizer as well, only the rows the batch hit move."""
    g = A.distinct_id_fixture()
    hp = dict(HP, weight_decay=1e-2, initial_accumulator=0.1)
    for argv, lazy in (([], False), (["--sparse-embedding-optimizer"], True)):
        m, h = A.build_dlrm(HIP, g, hp, argv=argv)
        rec = H.run_steps(m, h, 1)[0]
        m.close()
        for t, R in enumerate(g["rows"]):
            moved = (rec[f"emb.{t}.weight"] != g[f"init/emb.{t}.weight"]).any(axis=1)
            hit = np.zeros(R, bool)
            hit[g[f"sparse{t}"].ravel()] = True
            assert moved[hit].all()
            assert (not moved[~hit].any()) if lazy else moved[~hit].all(), (argv, t)
