"""Shared by the tests of per-table embedding bag sizes (tests/test_bags_cpu.py, tests/test_gpu_bags*.py): a small DLRM of mixed bag
sizes built through the Python FFModel API, its float64 numpy restatement, and the flags of the driver cases."""
import numpy as np

from dlrm_flexflow_amd import capi, ffmodel

# the 26 pooling sizes of the MLPerf DLRM-DCNv2 recipe
MLPERF_BAGS = [3, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 100, 27, 10, 3, 1, 1]

SMALL = dict(B=8, D=4, rows=(11, 5, 7), bags=(1, 3, 2), bot=(4, 8, 4), top=(16, 8, 1), lr=0.01)


def build_mixed_model(backend, cfg=SMALL, extra_argv=(), comm=None, seed=3):
    """Returns (model, handles): the cat-interaction DLRM of `cfg`, one [B][bags[t]] id tensor per table, plain SGD; inputs set from
    numpy's seeded generator, weights left as the initializers made them (handles["init"] holds what Tensor.get() returned)."""
    B, D = cfg["B"], cfg["D"]
    rows, bags, bot, top = cfg["rows"], cfg["bags"], cfg["bot"], cfg["top"]
    c = ffmodel.FFConfig(argv=["-b", str(B)] + list(extra_argv), backend=backend, comm=comm)
    c.set(enable_graph=False, overlap_embedding=True, dense_embedding_update=False)
    m = ffmodel.FFModel(c)
    sparse = [m.create_tensor([B, L], ffmodel.DT_INT64) for L in bags]
    dense = m.create_tensor([B, bot[0]], ffmodel.DT_FLOAT)
    x = dense
    for i in range(len(bot) - 1):
        x = m.dense(x, bot[i + 1], capi.AC_MODE_RELU)
    ly = [m.embedding(s, r, D, capi.AGGR_MODE_SUM) for s, r in zip(sparse, rows)]
    z = m.concat([x] + ly, 1)
    for i in range(len(top) - 1):
        z = m.dense(z, top[i + 1], capi.AC_MODE_SIGMOID if i == len(top) - 2 else capi.AC_MODE_RELU)
    m.set_sgd_optimizer(lr=cfg["lr"])
    m.compile()
    m.init_layers()
    nb, nt = len(bot) - 1, len(top) - 1
    names, layer = {}, 0
    for i in range(nb):
        names[f"bot.{i}"] = layer; layer += 1
    for t in range(len(rows)):
        names[f"emb.{t}"] = layer; layer += 1
    layer += 1
    for i in range(nt):
        names[f"top.{i}"] = layer; layer += 1
    assert layer == m.num_layers
    rng = np.random.default_rng(seed)
    data = {"dense": rng.random((B, bot[0]), dtype=np.float32), "label": rng.integers(0, 2, (B, 1)).astype(np.float32)}
    for t, (r, L) in enumerate(zip(rows, bags)):
        data[f"sparse{t}"] = rng.integers(0, r, (B, L)).astype(np.int64)
    data["sparse1"][0, :] = data["sparse1"][0, 0]            # a bag that repeats one row
    dense.set(data["dense"])
    m.label_tensor.set(data["label"])
    for t, s in enumerate(sparse):
        s.set(data[f"sparse{t}"])
    init = {}
    for k, li in names.items():
        init[f"{k}.weight"] = m.parameter(li, 0).get_weights()
        if not k.startswith("emb"):
            init[f"{k}.bias"] = m.parameter(li, 1).get_weights()
    return m, {"names": names, "final": m.num_layers - 1, "data": data, "init": init, "cfg": cfg}


def numpy_reference(h, steps):
    """The model of build_mixed_model in float64: forward, the MSE gradient (z - y) / B of the 0.5-sum-over-B loss the golden torch model uses,
    plain SGD on every parameter (a table row's gradient is the sum over the lookups that hit it).  Per-step records like dlrm_helpers.run_steps."""
    cfg, d = h["cfg"], h["data"]
    B, lr = cfg["B"], cfg["lr"]
    nb, nt, T = len(cfg["bot"]) - 1, len(cfg["top"]) - 1, len(cfg["rows"])
    P = {k: np.array(v, np.float64) for k, v in h["init"].items()}
    out = []
    for _ in range(steps):
        acts, x = [], d["dense"].astype(np.float64)
        for i in range(nb):
            acts.append(x)
            x = np.maximum(x @ P[f"bot.{i}.weight"].T + P[f"bot.{i}.bias"], 0.0)
        xb = x
        ly = [P[f"emb.{t}.weight"][d[f"sparse{t}"]].sum(1) for t in range(T)]
        z = np.concatenate([xb] + ly, 1)
        tacts = []
        for i in range(nt):
            tacts.append(z)
            z = z @ P[f"top.{i}.weight"].T + P[f"top.{i}.bias"]
            z = 1.0 / (1.0 + np.exp(-z)) if i == nt - 1 else np.maximum(z, 0.0)
        pred = z
        G = {}
        g = (pred - d["label"]) / B
        y = pred
        for i in reversed(range(nt)):
            g = g * (y * (1.0 - y)) if i == nt - 1 else g * (y > 0)
            G[f"top.{i}.weight"] = g.T @ tacts[i]
            G[f"top.{i}.bias"] = g.sum(0)
            g = g @ P[f"top.{i}.weight"]
            y = tacts[i]
        D, w0 = cfg["D"], cfg["bot"][-1]
        for t in range(T):
            ge = g[:, w0 + t * D:w0 + (t + 1) * D]
            gw = np.zeros_like(P[f"emb.{t}.weight"])
            np.add.at(gw, d[f"sparse{t}"].reshape(-1), np.repeat(ge, cfg["bags"][t], axis=0))
            G[f"emb.{t}.weight"] = gw
        g, y = g[:, :w0], xb
        for i in reversed(range(nb)):
            g = g * (y > 0)
            G[f"bot.{i}.weight"] = g.T @ acts[i]
            G[f"bot.{i}.bias"] = g.sum(0)
            g = g @ P[f"bot.{i}.weight"]
            y = acts[i]
        for k in P:
            P[k] = P[k] - lr * G[k]
        rec = {"pred": pred.copy()}
        rec.update({k: v.copy() for k, v in P.items()})
        out.append(rec)
    return out


# the driver cases of tests/test_gpu_bags_model.py: 4 tables of bag sizes 1, 3, 2, 7; D = 16; batch 256; small MLPs
DRIVER_ROWS = "1000-37-500-2000"
DRIVER_BAGS = "1-3-2-7"
DRIVER_ARGS = ["-b", "256", "--arch-sparse-feature-size", "16", "--arch-embedding-size", DRIVER_ROWS, "--arch-mlp-bot", "13-64-16",
               "--arch-mlp-top", "80-64-1", "--data-size", "256", "--embedding-bag-sizes", DRIVER_BAGS]


def trajectory(backend, args, steps, trace, counters=()):
    """1 warm-up + `steps` steps through the DLRM application object; every parameter and the predictions (and the named counters)."""
    app = ffmodel.DLRM(["--backend", backend] + list(args))
    app.warmup()
    app.train_steps(steps, trace=trace)
    app.model.sync()
    out = {}
    for li in range(app.model.num_layers):
        for wi in range(app.model.layer_num_weights(li)):
            out[f"{app.model.layer_name(li)}/{wi}"] = app.model.parameter(li, wi).get_weights()
    out["pred"] = app.model.layer_output(app.model.num_layers - 1).get()
    cnt = {c: app.model.counter(c) for c in counters}
    app.close()
    return (out, cnt) if counters else out
