"""Shared by the tests of the data-gradient half of the fold extension (include/ff_hip_fold.h, ABI 3): the seeded inputs of the table-update tests,
the route restated in float32 numpy (G in the canonical order, the product G W_t in the documented chain order, one fmaf), its float64 reference with
the term mass of the UNFOLDED sum, and the batch of the model test."""
import functools

import numpy as np

import fold_helpers as FH
import fold_dw_helpers as DH

ROWS = [1, 3, 63, 1543]          # one row, fewer rows than an MFMA tile, one short of two wave tiles, 48 wave tiles and a ragged one
BATCH, D = 4096, 128
OUTS = [256, 1024]               # depth of the product (= out_dim of the layer); the CPU test runs the first
LR = 0.05
NTAB = len(ROWS)
IN = D * (NTAB + 1)              # the layer's width: block 0 belongs to nobody, block t + 1 to table t


@functools.lru_cache(maxsize=None)
def inputs(bag, out):
    """dy [BATCH][out], w [out][IN], the ids [BATCH][bag] and rows [rows][D] of the four tables; seeded by (bag, out).  Row 1 of the 3-row table and
    the last row of the 63-row table are hit by nobody."""
    rng = np.random.default_rng(9000 + 10 * bag + out)
    dy = (rng.uniform(-1, 1, (BATCH, out)) / 32).astype(np.float32)
    w = rng.uniform(-1, 1, (out, IN)).astype(np.float32)
    ids = []
    for r in ROWS:
        i = rng.integers(0, r, (BATCH, bag)).astype(np.int64)
        if r == 3:
            i[i == 1] = 2
        if r == 63:
            i[i == 62] = 0
        ids.append(i)
    E = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    for a in [dy, w] + ids + E:
        a.setflags(write=False)
    return dy, w, ids, E


def unhit(t, bag, out):
    ids = inputs(bag, out)[2][t]
    hit = np.zeros(ROWS[t], bool)
    hit[ids.reshape(-1)] = True
    return ~hit


def w_block(w, t):
    return w[:, D * (t + 1):D * (t + 2)]


@functools.lru_cache(maxsize=None)
def references(bag, out):
    """Per table: (E - lr sum_hits dy[b] W_t in float64, the term mass sum_hits sum_o |dy| |w|): the unfolded formula, the sum over the hits first."""
    dy, w, ids, E = inputs(bag, out)
    res = []
    for t, r in enumerate(ROWS):
        wt = w_block(w, t).astype(np.float64)
        dx, mdx = dy.astype(np.float64) @ wt, np.abs(dy).astype(np.float64) @ np.abs(wt)        # the rows of the data gradient the route never forms
        dE, mass = np.zeros((r, D)), np.zeros((r, D))
        for l in range(bag):
            np.add.at(dE, ids[t][:, l], dx)
            np.add.at(mass, ids[t][:, l], mdx)
        ref = E[t].astype(np.float64) - float(np.float32(LR)) * dE
        ref.setflags(write=False); mass.setflags(write=False)
        res.append((ref, mass))
    return res


@functools.lru_cache(maxsize=None)
def canonical_G(bag, out):
    """G_t of every table in the canonical order of the fused table update (tests/fold_dw_helpers.py), float32."""
    dy, _, ids, _ = inputs(bag, out)
    G = [DH.segment_sum_canonical_f32(ids[t], dy, r) for t, r in enumerate(ROWS)]
    for g in G:
        g.setflags(write=False)
    return G


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64, one rounding of the sum (double rounding aside, which no bound here sees)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def update_f32(G, wt, E, lr):
    """include/ff_hip_fold.h, ffh_fold_table_update: one fp32 chain per element over the depth o -- groups j of 16 ascending, in a group the four MFMAs
    e = 0..3, MFMA e adding o = 16 j + 4 q + e for q = 0..3 -- then E = fmaf(-lr, sum, E)."""
    acc = np.zeros(E.shape, np.float32)
    for j in range(G.shape[1] // 16):
        for e in range(4):
            for q in range(4):
                o = 16 * j + 4 * q + e
                acc = fma32(G[:, o:o + 1], wt[o:o + 1, :], acc)
    return fma32(np.float32(-np.float32(lr)), acc, E)


def bound(mass, E, lr):
    """1e-5 lr (term mass of the unfolded sum) + 2 ulp(w)."""
    return 1e-5 * float(np.float32(lr)) * mass + 2.0 * np.spacing(np.abs(E)).astype(np.float64)


def assert_update_within(got, ref, mass, E, lr, what):
    err = np.abs(got.astype(np.float64) - ref)
    tol = bound(mass, E, lr)
    worst = float((err / tol).max())
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}")
    assert np.all(err <= tol), f"{what}: worst |got - ref| / bound = {worst:.3f} at flat index {int((err / tol).argmax())}"


# ---- the model test: tests/fold_dw_helpers.py's DLRM at a batch the kept data gradient is served at ---------------------------------------------------
def model_batch(compute_units):
    """The smallest multiple of 128 from DH.model_batch up at which the first top layer (8 column tiles of dX, depth 256 = 4 k-tiles) runs whole 128 x 128
    tiles on one workgroup per CU -- whole rounds, or a last round whose idle share is below two k-tiles per workgroup -- and its 5 kept column tiles
    still fill their rounds to 80 %: the rule ffh_fold_linear_bwd_dx_plan restates from the persistent kernel's plan."""
    g = compute_units & ~7
    nt, kept, nk = (DH.MODEL_D * (len(DH.MODEL_ROWS) + 1)) // 128, DH.MODEL_KEPT_TILES, DH.MODEL_OUT // 64
    b = -(-DH.model_batch(compute_units) // 128) * 128
    while True:
        nby = b // 128

        def whole(ntiles):
            rounds = -(-ntiles // g)
            return ntiles >= g and ntiles * 100 >= rounds * g * 80

        tiles = nt * nby
        idle_it = (-(-tiles // g) * g - tiles) * nk // g
        if whole(tiles) and idle_it < 2 and whole(kept * nby):
            return b
        b += 128


def run_model(backend, batch, flags, steps=3, trace=False, snapshots=False):
    """tests/fold_dw_helpers.py::run_model with the data-gradient half's counter: the warm-up iteration, then `steps` training steps."""
    from dlrm_flexflow_amd import ffmodel
    app = ffmodel.DLRM(["--backend", backend, "--lr", str(DH.LR)] + DH.model_args(batch, flags))
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
        rec["ids" + tag] = [app.sparse_input(t).get(np.int64) for t in range(len(DH.MODEL_ROWS))]
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
    rec["counters"] = counters_of(m)
    rec["replays"] = m.counter("graph_replays")
    rec["names"] = names
    app.close()
    return rec


def counters_of(m):
    return tuple(m.counter(k) for k in ("folded_tables", "folded_dw_tables", "folded_dx_tables"))


def route_counters(backend, batch, flags):
    """(folded, dw-folded, dx-folded tables) of the model built with `flags`; nothing runs."""
    from dlrm_flexflow_amd import ffmodel
    app = ffmodel.DLRM(["--backend", backend, "--lr", str(DH.LR)] + DH.model_args(batch, flags))
    c = counters_of(app.model)
    app.close()
    return c
