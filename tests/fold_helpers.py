"""Shared by the tests of the fold extension (include/ff_hip_fold.h): the float64 statement of the UNFOLDED formulas with the project's bound, and
the small `cat` DLRM the model-level tests train."""
import numpy as np

from dlrm_flexflow_amd import ffmodel

NONE, RELU = 10, 11      # FFH_AC_MODE_*
AGGR_SUM, AGGR_AVG = 21, 22
UNSUPPORTED = -3


def bound(mass):
    """|error| <= 1e-5 * sum_k |a_k b_k| + 1e-6, the term mass over every term of the full-width sum."""
    return 1e-5 * mass + 1e-6


def assert_within(got, ref, mass, what):
    err = np.abs(got.astype(np.float64) - ref)
    tol = bound(mass)
    worst = float((err / tol).max()) if err.size else 0.0
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}")
    assert np.all(err <= tol), f"{what}: worst |got - ref| / bound = {worst:.3f} at flat index {int((err / tol).argmax())}"


def make_ids(rng, kind, batch, bag, rows):
    if kind == "random":
        return rng.integers(0, rows, (batch, bag)).astype(np.int64)
    if kind == "equal":
        return np.full((batch, bag), rng.integers(0, rows), np.int64)
    if kind == "last":
        return np.full((batch, bag), rows - 1, np.int64)
    raise ValueError(kind)


# ---- the model of the issue: 6 tables of 3-5000-1-40-70000-300 rows, D = 32, bot 13-64-32, top 224-128-64-1, batch 512 ----------------------------------
MODEL_ROWS = [3, 5000, 1, 40, 70000, 300]
MODEL_B, MODEL_D = 512, 32


def model_args(extra=()):
    top = MODEL_D * (len(MODEL_ROWS) + 1)
    return ["-b", str(MODEL_B), "--arch-sparse-feature-size", str(MODEL_D), "--arch-embedding-size", "-".join(str(r) for r in MODEL_ROWS),
            "--arch-mlp-bot", f"13-64-{MODEL_D}", "--arch-mlp-top", f"{top}-128-64-1", "--data-size", str(MODEL_B)] + list(extra)


def weights_of(m):
    out = {}
    for li in range(m.num_layers):
        for wi in range(m.layer_num_weights(li)):
            p = m.parameter(li, wi)
            if p.is_local:
                out[f"{m.layer_name(li)}/{wi}"] = p.get_weights()
    return out


def run_model(backend, flags, steps=3, trace=False, snapshots=False):
    """warm-up iteration + `steps` training steps of the model above; the weights before and after, the predictions, the counters.  snapshots: one
    step per call, the ReLU layers' (y > 0) kept after every step (where two runs' relu' masks differ), and the last step's activations / gradients."""
    app = ffmodel.DLRM(["--backend", backend, "--lr", "0.01"] + model_args(flags))
    m = app.model
    rec = {"w0": weights_of(m), "masks": []}
    names = [m.layer_name(li) for li in range(m.num_layers)]
    dense = [li for li in range(m.num_layers) if names[li].startswith("Dense")]

    def snap():
        m.sync()
        rec["masks"].append({names[li]: m.layer_output(li).get() > 0 for li in dense[:-1]})
    app.warmup()
    if snapshots:
        snap()
        for _ in range(steps):
            app.train_steps(1, trace=trace)
            snap()
    else:
        app.train_steps(steps, trace=trace)
    m.sync()
    rec["w1"] = weights_of(m)
    rec["pred"] = m.layer_output(m.num_layers - 1).get()
    rec["folded"] = m.counter("folded_tables")
    rec["replays"] = m.counter("graph_replays")
    rec["names"] = names
    if snapshots:
        rec["dy"] = {names[li]: m.layer_output(li).get_grad() for li in dense}
        rec["out"] = {names[li]: m.layer_output(li).get() for li in range(m.num_layers) if not names[li].startswith("Embedding")}
        rec["x0"] = app.dense_input().get()
        rec["ids"] = [app.sparse_input(t).get(np.int64) for t in range(len(MODEL_ROWS))]
    app.close()
    return rec
