"""GPU tests (-m gpu) of per-sample bag weights that the model computes (include/ffh_bag_weights_grad.h): a table's weights are a
gate sigmoid(Linear(dense -> L)), and one training step -- predictions, the gates' weights, the tables -- equals a float64 model of it.  Two models:
  own     every table has a gate of its own, read by nothing else: the gradient is stored
  shared  tables 0 and 1 read ONE gate, which the Concat above the tables reads as well; table 2's gate also feeds a Linear that stands between the
          gate and the tables: every gradient is accumulated, beside readers on the compute stream, and the shared gate takes one launch per table"""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import dlrm_helpers as H

pytestmark = pytest.mark.gpu
B, D, ROWS, NIN, BOT, AUX, LR = 64, 16, (11, 5, 7), 4, 4, 3, 0.05
T = len(ROWS)
MODELS = {"own": dict(bags=(1, 2, 5), gate_of=(0, 1, 2), extra=False, launches=1), "shared": dict(bags=(2, 2, 5), gate_of=(0, 0, 1), extra=True, launches=2)}


def case(bags, seed=3):
    rng = np.random.default_rng(seed)
    data = {"dense": rng.random((B, NIN), dtype=np.float32), "label": rng.integers(0, 2, (B, 1)).astype(np.float32)}
    for t, (r, L) in enumerate(zip(ROWS, bags)):
        ids = rng.integers(0, r, (B, L)).astype(np.int64)
        ids[rng.random((B, L)) < 0.3] = -1
        ids[2, :] = -1                                     # a bag of only pads
        data[f"sparse{t}"], data[f"w{t}"] = ids, rng.uniform(0.5, 1.5, (B, L)).astype(np.float32)      # w: the weights where they are an input
    return data


def build(v, data, produced=True, graph=False, argv=()):
    """bot = relu(Linear(dense)), the gates (or a weights input per table), [aux = relu(Linear(last gate))], the weighted tables,
    concat(bot, tables[, gate 0, aux]), the click layer."""
    bags, gate_of = v["bags"], v["gate_of"]
    c = ffmodel.FFConfig(argv=["-b", str(B), *argv], backend=capi.HIP_LIB_PATH)
    c.set(enable_graph=graph, overlap_embedding=True, dense_embedding_update=False, embedding_padding=True)
    m = ffmodel.FFModel(c)
    sparse = [m.create_tensor([B, L], ffmodel.DT_INT64) for L in bags]
    win = [] if produced else [m.create_tensor([B, L], ffmodel.DT_FLOAT) for L in bags]
    dense = m.create_tensor([B, NIN], ffmodel.DT_FLOAT)
    x = m.dense(dense, BOT, capi.AC_MODE_RELU)
    ng = max(gate_of) + 1 if produced else 0
    gates = [m.dense(dense, bags[gate_of.index(g)], capi.AC_MODE_SIGMOID) for g in range(ng)]
    extra = [gates[0], m.dense(gates[-1], AUX, capi.AC_MODE_RELU)] if produced and v["extra"] else []
    ly = [m.embedding(s, r, D, capi.AGGR_MODE_SUM, per_sample_weights=gates[gate_of[t]] if produced else win[t]) for t, (s, r) in enumerate(zip(sparse, ROWS))]
    m.dense(m.concat([x] + ly + extra, 1), 1, capi.AC_MODE_SIGMOID)
    m.set_sgd_optimizer(lr=LR)
    m.compile()
    m.init_layers()
    keys = ["bot"] + [f"gate.{g}" for g in range(ng)] + (["aux"] if extra else []) + [f"emb.{t}" for t in range(T)] + [None, "top"]
    names = {k: i for i, k in enumerate(keys) if k}
    dense.set(data["dense"])
    m.label_tensor.set(data["label"])
    for t, s in enumerate(sparse):
        s.set(data[f"sparse{t}"])
        if not produced:
            win[t].set(data[f"w{t}"])
    init = {f"{k}.weight": m.parameter(li, 0).get_weights() for k, li in names.items()}
    init.update({f"{k}.bias": m.parameter(li, 1).get_weights() for k, li in names.items() if not k.startswith("emb")})
    return m, {"names": names, "final": m.num_layers - 1, "init": init}


def reference(v, init, data):
    """One step in float64: dL/dw[b][l] = dY[b] . W[id] summed over the tables (and other readers) of a gate, through the sigmoid into the gate; a
    row's gradient is weighted; a pad does neither."""
    gate_of, ng = v["gate_of"], max(v["gate_of"]) + 1
    P = {k: np.array(a, np.float64) for k, a in init.items()}
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    x0, G = data["dense"].astype(np.float64), {}
    xb = np.maximum(x0 @ P["bot.weight"].T + P["bot.bias"], 0.0)
    w = [sig(x0 @ P[f"gate.{g}.weight"].T + P[f"gate.{g}.bias"]) for g in range(ng)]
    aux = np.maximum(w[-1] @ P["aux.weight"].T + P["aux.bias"], 0.0) if v["extra"] else None
    ids = [np.maximum(data[f"sparse{t}"], 0) for t in range(T)]
    rows = [P[f"emb.{t}.weight"][ids[t]] for t in range(T)]                                      # [B][L][D]
    live = [data[f"sparse{t}"] >= 0 for t in range(T)]
    z = np.concatenate([xb] + [(rows[t] * (w[gate_of[t]] * live[t])[:, :, None]).sum(1) for t in range(T)] + ([w[0], aux] if v["extra"] else []), 1)
    pred = sig(z @ P["top.weight"].T + P["top.bias"])
    g = (pred - data["label"]) / B * pred * (1.0 - pred)
    G["top.weight"], G["top.bias"], gz = g.T @ z, g.sum(0), g @ P["top.weight"]
    gw = [np.zeros_like(a) for a in w]
    for t in range(T):
        ge = gz[:, BOT + t * D:BOT + (t + 1) * D]
        G[f"emb.{t}.weight"] = np.zeros_like(P[f"emb.{t}.weight"])
        np.add.at(G[f"emb.{t}.weight"], ids[t].reshape(-1), (ge[:, None, :] * (w[gate_of[t]] * live[t])[:, :, None]).reshape(-1, D))
        gw[gate_of[t]] += (ge[:, None, :] * rows[t]).sum(2) * live[t]
    if v["extra"]:
        c0 = BOT + T * D
        ga = gz[:, c0 + w[0].shape[1]:] * (aux > 0)
        G["aux.weight"], G["aux.bias"] = ga.T @ w[-1], ga.sum(0)
        gw[0] += gz[:, c0:c0 + w[0].shape[1]]
        gw[-1] += ga @ P["aux.weight"]
    for k in range(ng):
        gg = gw[k] * w[k] * (1.0 - w[k])
        G[f"gate.{k}.weight"], G[f"gate.{k}.bias"] = gg.T @ x0, gg.sum(0)
    gb = gz[:, :BOT] * (xb > 0)
    G["bot.weight"], G["bot.bias"] = gb.T @ x0, gb.sum(0)
    return dict({k: P[k] - LR * G[k] for k in P}, pred=pred)


@pytest.mark.parametrize("model", list(MODELS))
def test_one_step_equals_the_float64_model(hip, model):
    """At the bound of tests/test_gpu_bag_weights_model.py.  The gates must move, and as the reference says: without a gradient they keep their values.
    One launch per step and table group (a shared gate: one per table on it); none where the weights are an input."""
    v = MODELS[model]
    data = case(v["bags"])
    for produced in (False, True):
        m, h = build(v, data, produced)
        got = H.run_steps(m, h, steps=1, trace=False)[0]
        cnt = [m.counter(f"bag_weight_{c}_launches") for c in ("grad", "gather", "update")]
        m.close()
        assert cnt == [v["launches"] * produced, 1, 1], cnt
    ref = reference(v, h["init"], data)
    assert got.keys() == ref.keys()
    for k in got:
        np.testing.assert_allclose(got[k], ref[k], rtol=2e-5, atol=2e-6, err_msg=k)
    for k in [k for k in got if k.startswith("gate") and k.endswith("weight")]:
        assert not np.allclose(got[k], h["init"][k], rtol=2e-5, atol=2e-6), f"{k} did not move"


@pytest.mark.parametrize("model", list(MODELS))
def test_replayed_steps_equal_eager_steps_bit_for_bit(hip, model):
    """--deterministic; the first traced step is captured and launched, the next three are replays."""
    v, runs = MODELS[model], []
    data = case(v["bags"])
    for graph in (False, True):
        m, h = build(v, data, graph=graph, argv=["--deterministic"])
        runs.append(H.run_steps(m, h, steps=4, trace=graph))
        assert m.counter("graph_replays") == (3 if graph else 0)
        m.close()
    for step, (a, b) in enumerate(zip(*runs)):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), f"{k} step {step}"
