"""Shared by the tests of the weight-gradient half of the fold extension (include/ff_hip_fold.h, ABI 2): the seeded inputs of the kernel tests, the
folded formula restated in float32 numpy (G in the canonical order of the fused table update, then G^T E), and the `cat` DLRM of the model test."""
import numpy as np

from dlrm_flexflow_amd import ffmodel
import fold_helpers as FH

ROWS = [1, 3, 300, 5000]         # the tables of the segment-sum and product tests, in one call
WIDTH, BATCH, D = 256, 512, 128  # width of dy (= out_dim of the layer), batch, table width
KINDS = ["random", "equal", "last"]
CHUNK = 256                      # FFH_FOLD_DW_CHUNK


def segment_inputs(bag, kind):
    """dy [BATCH][WIDTH], the ids of the four tables [BATCH][bag], the tables [rows][D]: seeded by (bag, kind)."""
    rng = np.random.default_rng(1000 * bag + KINDS.index(kind))
    dy = rng.uniform(-1, 1, (BATCH, WIDTH)).astype(np.float32)
    ids = [FH.make_ids(rng, kind, BATCH, bag, r) for r in ROWS]
    E = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    return dy, ids, E


def segment_sum_f64(ids, dy, rows):
    """G[r] = the sum of dy[b] over the hits of row r, and the same over |dy| (the term mass), in float64."""
    G, M = np.zeros((rows, dy.shape[1])), np.zeros((rows, dy.shape[1]))
    d64 = dy.astype(np.float64)
    for l in range(ids.shape[1]):
        np.add.at(G, ids[:, l], d64)
        np.add.at(M, ids[:, l], np.abs(d64))
    return G, M


def segment_sum_canonical_f32(ids, dy, rows):
    """include/ff_hip.h, "Canonical (deterministic) summation order": the hits sorted by (row, position b * bag + l); the sorted list cut at multiples of 32
    and of 1024; a row's hits inside a 32-block added left to right in fp32, its 32-block partials inside a 1024-block left to right, then its 1024-block
    partials left to right."""
    L = ids.shape[1]
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable")
    N = len(order)
    total = {}
    for k1 in range(0, N, 1024):
        p1 = {}
        for k0 in range(k1, min(k1 + 1024, N), 32):
            p0 = {}
            for j in range(k0, min(k0 + 32, N)):
                r, v = int(flat[order[j]]), dy[order[j] // L]
                p0[r] = v.copy() if r not in p0 else (p0[r] + v).astype(np.float32)
            for r, v in p0.items():
                p1[r] = v if r not in p1 else (p1[r] + v).astype(np.float32)
        for r, v in p1.items():
            total[r] = v if r not in total else (total[r] + v).astype(np.float32)
    G = np.zeros((rows, dy.shape[1]), np.float32)
    for r, v in total.items():
        G[r] = v
    return G


def product_f32(G, E):
    """G^T E in float32, the rows cut into the chunks whose partial products the kernel adds into dW."""
    acc = np.zeros((G.shape[1], E.shape[1]), np.float32)
    for r0 in range(0, G.shape[0], CHUNK):
        acc = (acc + G[r0:r0 + CHUNK].T @ E[r0:r0 + CHUNK]).astype(np.float32)
    return acc


def gathered(E, ids):
    """X_t in float64: the bag's rows summed."""
    return E.astype(np.float64)[ids].sum(1)


# ---- the model of the issue: D = 128, bottom 13-64-128, 7 tables of which three are folded, top 1024-256-64-1 -----------------------------------------
MODEL_ROWS = [3, 300, 70000, 40, 80000, 90000, 100000]
MODEL_D, MODEL_OUT = 128, 256
MODEL_KEPT_TILES = 5       # the bottom block and the four big tables
LR = 0.01


def model_batch(compute_units):
    """The smallest multiple of 64 at which the stream-K weight gradient takes 5 kept column tiles x 2 row tiles: 8 k-tiles of 64 per workgroup."""
    g = compute_units & ~7
    tiles = MODEL_KEPT_TILES * (MODEL_OUT // 128)
    return -(-8 * g // tiles) * 64


def model_args(batch, extra=()):
    top = MODEL_D * (len(MODEL_ROWS) + 1)
    return ["-b", str(batch), "--arch-sparse-feature-size", str(MODEL_D), "--arch-embedding-size", "-".join(str(r) for r in MODEL_ROWS),
            "--arch-mlp-bot", f"13-64-{MODEL_D}", "--arch-mlp-top", f"{top}-{MODEL_OUT}-64-1", "--data-size", str(batch)] + list(extra)


def run_model(backend, batch, flags, steps=3, trace=False, snapshots=False):
    """The warm-up iteration, then `steps` training steps.  Weights before (w0), after the warm-up (w_warm) and at the end (w1); snapshots: the ReLU
    layers' (y > 0) after every step, and the activations / gradients / inputs of the warm-up iteration and of the last step."""
    app = ffmodel.DLRM(["--backend", backend, "--lr", str(LR)] + model_args(batch, flags))
    m = app.model
    rec = {"w0": FH.weights_of(m), "masks": []}
    names = [m.layer_name(li) for li in range(m.num_layers)]
    dense = [li for li in range(m.num_layers) if names[li].startswith("Dense")]

    def snap(tag):
        m.sync()
        rec["masks"].append({names[li]: m.layer_output(li).get() > 0 for li in dense[:-1]})
        rec["dy" + tag] = {names[li]: m.layer_output(li).get_grad() for li in dense}
        rec["out" + tag] = {names[li]: m.layer_output(li).get() for li in range(m.num_layers) if not names[li].startswith("Embedding")}
        rec["x0" + tag] = app.dense_input().get()
        rec["ids" + tag] = [app.sparse_input(t).get(np.int64) for t in range(len(MODEL_ROWS))]
    app.warmup()
    m.sync()
    rec["w_warm"] = FH.weights_of(m)
    if snapshots:
        snap("_warm")
        for _ in range(steps):
            app.train_steps(1, trace=trace)
            snap("")
    else:
        app.train_steps(steps, trace=trace)
    m.sync()
    rec["w1"] = FH.weights_of(m)
    rec["pred"] = m.layer_output(m.num_layers - 1).get()
    rec["folded"] = m.counter("folded_tables")
    rec["folded_dw"] = m.counter("folded_dw_tables")
    rec["replays"] = m.counter("graph_replays")
    rec["names"] = names
    app.close()
    return rec
