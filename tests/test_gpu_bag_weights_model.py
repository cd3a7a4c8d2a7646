"""GPU tests (-m gpu) of per-sample weights in the host model (FFModel.embedding(..., per_sample_weights=)): the small model of
tests/bags_helpers.py with a weights tensor per table against a float64 restatement, and a weights tensor of ones against the model without one."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import bags_helpers as BH
import dlrm_helpers as H

pytestmark = pytest.mark.gpu
HIP = capi.HIP_LIB_PATH
COUNTERS = ("bag_weight_gather_launches", "bag_weight_update_launches", "pad_gather_launches", "pad_update_launches")


def build(cfg, data, wts, padding=False):
    """The cat-interaction DLRM of tests/bags_helpers.py, plain SGD; wts[t]: table t's [B][L] float32 weights, or None for a table without."""
    B, D, rows, bags, bot, top = cfg["B"], cfg["D"], cfg["rows"], cfg["bags"], cfg["bot"], cfg["top"]
    c = ffmodel.FFConfig(argv=["-b", str(B)], backend=HIP)
    c.set(enable_graph=False, overlap_embedding=True, dense_embedding_update=False, embedding_padding=padding)
    m = ffmodel.FFModel(c)
    sparse = [m.create_tensor([B, L], ffmodel.DT_INT64) for L in bags]
    wt = [None if w is None else m.create_tensor([B, L], ffmodel.DT_FLOAT) for w, L in zip(wts, bags)]
    dense = m.create_tensor([B, bot[0]], ffmodel.DT_FLOAT)
    x = dense
    for i in range(len(bot) - 1):
        x = m.dense(x, bot[i + 1], capi.AC_MODE_RELU)
    ly = [m.embedding(s, r, D, capi.AGGR_MODE_SUM, per_sample_weights=w) for s, r, w in zip(sparse, rows, wt)]
    z = m.concat([x] + ly, 1)
    for i in range(len(top) - 1):
        z = m.dense(z, top[i + 1], capi.AC_MODE_SIGMOID if i == len(top) - 2 else capi.AC_MODE_RELU)
    m.set_sgd_optimizer(lr=cfg["lr"])
    m.compile()
    m.init_layers()
    keys = [f"bot.{i}" for i in range(len(bot) - 1)] + [f"emb.{t}" for t in range(len(rows))] + [None] + [f"top.{i}" for i in range(len(top) - 1)]
    names = {k: i for i, k in enumerate(keys) if k}
    dense.set(data["dense"])
    m.label_tensor.set(data["label"])
    for t, s in enumerate(sparse):
        s.set(data[f"sparse{t}"])
        if wt[t] is not None:
            wt[t].set(wts[t])
    init = {}
    for k, li in names.items():
        init[f"{k}.weight"] = m.parameter(li, 0).get_weights()
        if not k.startswith("emb"):
            init[f"{k}.bias"] = m.parameter(li, 1).get_weights()
    return m, {"names": names, "final": m.num_layers - 1, "data": data, "init": init, "cfg": cfg}


def reference(h, wts, steps):
    """BH.numpy_reference with a weight per lookup, float64: bag = sum_j w_j W[id_j]; row gradient = sum over its lookups of w_j * the bag's gradient."""
    cfg, d = h["cfg"], h["data"]
    B, lr, D, w0 = cfg["B"], cfg["lr"], cfg["D"], cfg["bot"][-1]
    nb, nt, T = len(cfg["bot"]) - 1, len(cfg["top"]) - 1, len(cfg["rows"])
    P = {k: np.array(v, np.float64) for k, v in h["init"].items()}
    W = [np.asarray(w, np.float64) for w in wts]
    out = []
    for _ in range(steps):
        acts, x = [], d["dense"].astype(np.float64)
        for i in range(nb):
            acts.append(x)
            x = np.maximum(x @ P[f"bot.{i}.weight"].T + P[f"bot.{i}.bias"], 0.0)
        xb = x
        z = np.concatenate([xb] + [(P[f"emb.{t}.weight"][d[f"sparse{t}"]] * W[t][:, :, None]).sum(1) for t in range(T)], 1)
        tacts = []
        for i in range(nt):
            tacts.append(z)
            z = z @ P[f"top.{i}.weight"].T + P[f"top.{i}.bias"]
            z = 1.0 / (1.0 + np.exp(-z)) if i == nt - 1 else np.maximum(z, 0.0)
        pred, G = z, {}
        g, y = (pred - d["label"]) / B, pred
        for i in reversed(range(nt)):
            g = g * (y * (1.0 - y)) if i == nt - 1 else g * (y > 0)
            G[f"top.{i}.weight"], G[f"top.{i}.bias"] = g.T @ tacts[i], g.sum(0)
            g, y = g @ P[f"top.{i}.weight"], tacts[i]
        for t in range(T):
            ge = g[:, w0 + t * D:w0 + (t + 1) * D]
            gw = np.zeros_like(P[f"emb.{t}.weight"])
            np.add.at(gw, d[f"sparse{t}"].reshape(-1), np.repeat(ge, cfg["bags"][t], axis=0) * W[t].reshape(-1, 1))
            G[f"emb.{t}.weight"] = gw
        g, y = g[:, :w0], xb
        for i in reversed(range(nb)):
            g = g * (y > 0)
            G[f"bot.{i}.weight"], G[f"bot.{i}.bias"] = g.T @ acts[i], g.sum(0)
            g, y = g @ P[f"bot.{i}.weight"], acts[i]
        P = {k: P[k] - lr * G[k] for k in P}
        out.append(dict(P, pred=pred.copy()))
    return out


def test_the_driver_flag_reaches_the_weighted_kernels(hip):
    """--embedding-per-sample-weights: the start-up line, both counters, and other bits than the run without it -- which calls none of the new entries."""
    import os
    import subprocess
    from conftest import ROOT
    args = BH.DRIVER_ARGS + ["--deterministic", "--no-trace"]
    a, ca = BH.trajectory(HIP, args + ["--embedding-per-sample-weights"], 2, trace=False, counters=COUNTERS)
    b, cb = BH.trajectory(HIP, args, 2, trace=False, counters=COUNTERS)
    assert ca["bag_weight_gather_launches"] > 0 and ca["bag_weight_update_launches"] > 0 and ca["pad_gather_launches"] == 0, ca
    assert not any(cb.values()), cb
    assert a.keys() == b.keys() and any(a[k].tobytes() != b[k].tobytes() for k in a), "the weights changed nothing"
    line = "[DLRM] embedding weights: per sample, synthetic uniform [0.5, 1.5)"
    for flags, there in ((["--embedding-per-sample-weights=1"], True), ([], False)):
        r = subprocess.run([os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm"), "--backend", HIP, *args, "--epochs", "1", *flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "THROUGHPUT" in r.stdout, r.stderr[-2000:]
        assert (line in r.stdout.splitlines()) == there, r.stdout[-2000:]


def case(seed=3):
    cfg = BH.SMALL
    rng = np.random.default_rng(seed)
    data = {"dense": rng.random((cfg["B"], cfg["bot"][0]), dtype=np.float32), "label": rng.integers(0, 2, (cfg["B"], 1)).astype(np.float32)}
    for t, (r, L) in enumerate(zip(cfg["rows"], cfg["bags"])):
        data[f"sparse{t}"] = rng.integers(0, r, (cfg["B"], L)).astype(np.int64)
    wts = [rng.uniform(0.5, 1.5, (cfg["B"], L)).astype(np.float32) for L in cfg["bags"]]
    return cfg, data, wts


def test_small_model_equals_the_float64_model(hip):
    """Two steps at the bound of tests/test_gpu_pad_model.py; three tables of mixed bag sizes, a weight per lookup."""
    cfg, data, wts = case()
    assert len(cfg["rows"]) == 3 and len(set(cfg["bags"])) > 1
    m, h = build(cfg, data, wts)
    recs = H.run_steps(m, h, steps=2, trace=False)
    got = {c: m.counter(c) for c in COUNTERS}
    m.close()
    assert got["bag_weight_gather_launches"] > 0 and got["bag_weight_update_launches"] > 0 and got["pad_gather_launches"] == 0, got
    for step, (g, r) in enumerate(zip(recs, reference(h, wts, 2))):
        assert g.keys() == r.keys()
        for k in g:
            np.testing.assert_allclose(g[k], r[k], rtol=2e-5, atol=2e-6, err_msg=f"{k} step {step}")
    unweighted = BH.numpy_reference(h, 1)[0]
    assert not np.allclose(recs[0]["emb.1.weight"], unweighted["emb.1.weight"], rtol=2e-5, atol=2e-6), "the weights changed nothing"


def test_a_weights_tensor_of_ones_changes_no_bit(hip):
    """Against the model without a weights tensor (the ragged entries, whose bits the pad forms keep where there is no pad, and reference 1 of the
    header); one table keeps no weights tensor and runs on the pad form beside the weighted ones."""
    cfg, data, wts = case()
    ones = [np.ones_like(wts[0]), None, np.ones_like(wts[2])]
    runs = []
    for w, padding in ((ones, False), ([None] * 3, False)):
        m, h = build(cfg, data, w, padding)
        runs.append((H.run_steps(m, h, steps=2, trace=False), {c: m.counter(c) for c in COUNTERS}))
        m.close()
    (a, ca), (b, cb) = runs
    assert ca["bag_weight_gather_launches"] > 0 and ca["bag_weight_update_launches"] > 0 and ca["pad_gather_launches"] > 0 and ca["pad_update_launches"] > 0, ca
    assert not any(cb.values()), cb
    for ra, rb in zip(a, b):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert ra[k].tobytes() == rb[k].tobytes(), k
