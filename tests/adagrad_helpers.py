"""Shared by tests/test_gpu_adagrad_model.py, tests/test_gpu_adagrad_ranks.py and tests/_dist_worker_adagrad.py: the golden DLRM of tests/dlrm_helpers.py (the harness of the Adam-versus-torch whole-step test)
built with an AdagradOptimizer, a float64 torch twin of it under torch.optim.Adagrad, and a second tiny DLRM whose tables are large enough
for a batch of distinct ids; and the driver's DLRM with the dot or the DCNv2 interaction and the BCE loss beside a live torch float64 twin of it."""
import numpy as np

from conftest import golden
from dlrm_flexflow_amd import capi, ffmodel


def build_dlrm(backend, g, hp, argv=(), enable_graph=False, overlap=False, dense_update=False, comm=None):
    """tests/dlrm_helpers.build_golden_dlrm with ffmodel.AdagradOptimizer(**hp); `g`: the fixture (or a dict shaped like it).  With `comm`
    (world_size > 1) each rank loads its batch slice and the tables it holds (table-wise or replicated: whole tables)."""
    B, D, L = int(g["B"]), int(g["D"]), int(g["L"])
    rows, bot, top = list(g["rows"]), list(g["bot"]), list(g["top"])
    world = comm.world_size if comm is not None else 1
    rank = comm.rank if comm is not None else 0
    cfg = ffmodel.FFConfig(argv=["-b", str(B)] + list(argv), backend=backend, comm=comm)
    cfg.set(enable_graph=enable_graph, overlap_embedding=overlap, dense_embedding_update=dense_update)
    m = ffmodel.FFModel(cfg)
    sparse = [m.create_tensor([B, L], ffmodel.DT_INT64) for _ in rows]
    dense = m.create_tensor([B, bot[0]], ffmodel.DT_FLOAT)
    x = dense
    for i in range(len(bot) - 1):
        x = m.dense(x, bot[i + 1], capi.AC_MODE_RELU)
    ly = [m.embedding(s, r, D, capi.AGGR_MODE_SUM) for s, r in zip(sparse, rows)]
    z = m.concat([x] + ly, 1)
    for i in range(len(top) - 1):
        z = m.dense(z, top[i + 1], capi.AC_MODE_SIGMOID if i == len(top) - 2 else capi.AC_MODE_RELU)
    ffmodel.AdagradOptimizer(m, **hp)
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
    for k, li in names.items():
        if m.parameter(li, 0).is_local:
            m.parameter(li, 0).set_weights(np.ascontiguousarray(g[f"init/{k}.weight"]))
        if not k.startswith("emb"):
            m.parameter(li, 1).set_weights(np.ascontiguousarray(g[f"init/{k}.bias"]))
    Bl = B // world
    sl = slice(rank * Bl, (rank + 1) * Bl)
    dense.set(np.ascontiguousarray(g["dense"][sl]))
    m.label_tensor.set(np.ascontiguousarray(g["label"][sl]))
    for t, s in enumerate(sparse):
        if s.is_local:
            s.set(np.ascontiguousarray(g[f"sparse{t}"]))
    return m, {"names": names, "final": m.num_layers - 1, "slice": sl, "g": g}


def torch_adagrad_reference(g, steps, lr, weight_decay, epsilon, initial_accumulator):
    """The golden DLRM in torch float64 on the CPU (autograd for the gradients, the MSE mean of the harness) under torch.optim.Adagrad.
    Returns per-step records like dlrm_helpers.run_steps(), in float64."""
    import torch
    rows, bot, top = list(g["rows"]), list(g["bot"]), list(g["top"])
    B = int(g["B"])
    keys = [f"bot.{i}" for i in range(len(bot) - 1)] + [f"top.{i}" for i in range(len(top) - 1)]
    P = {}
    for k in keys:
        P[f"{k}.weight"] = g[f"init/{k}.weight"]; P[f"{k}.bias"] = g[f"init/{k}.bias"]
    for t in range(len(rows)):
        P[f"emb.{t}.weight"] = g[f"init/emb.{t}.weight"]
    P = {k: torch.tensor(np.array(v, np.float64), requires_grad=True) for k, v in P.items()}
    opt = torch.optim.Adagrad(list(P.values()), lr=lr, lr_decay=0, weight_decay=weight_decay, initial_accumulator_value=initial_accumulator, eps=epsilon)
    dense, label = torch.from_numpy(np.asarray(g["dense"], np.float64)), torch.from_numpy(np.asarray(g["label"], np.float64))
    sparse = [torch.from_numpy(np.asarray(g[f"sparse{t}"])) for t in range(len(rows))]
    out = []
    for _ in range(steps):
        x = dense
        for i in range(len(bot) - 1):
            x = torch.relu(x @ P[f"bot.{i}.weight"].T + P[f"bot.{i}.bias"])
        ly = [P[f"emb.{t}.weight"][s].sum(1) for t, s in enumerate(sparse)]
        z = torch.cat([x] + ly, 1)
        for i in range(len(top) - 1):
            z = z @ P[f"top.{i}.weight"].T + P[f"top.{i}.bias"]
            z = torch.sigmoid(z) if i == len(top) - 2 else torch.relu(z)
        opt.zero_grad()
        (0.5 * ((z - label) ** 2).sum() / B).backward()
        opt.step()
        rec = {"pred": z.detach().numpy().copy()}
        rec.update({k: v.detach().numpy().copy() for k, v in P.items()})
        out.append(rec)
    return out


def distinct_id_fixture(seed=3):
    """A dict shaped like the golden fixture: B = 16, bags of 2, four tables of 64 .. 200 rows, and ids that are the head of a permutation per
    table -- every row is hit at most once a step, so the scatter-add of the dense table path has no order to differ in."""
    g0 = golden("dlrm_step_torch")
    rng = np.random.default_rng(seed)
    B, D, L = 16, 8, 2
    rows = [64, 200, 33, 97]
    g = {"B": B, "D": D, "L": L, "rows": rows, "bot": list(g0["bot"]), "top": list(g0["top"])}
    for k in g0.files:
        if k.startswith("init/") and not k.startswith("init/emb"):
            g[k] = g0[k]
    g["dense"], g["label"] = g0["dense"], g0["label"]
    for t, R in enumerate(rows):
        g[f"init/emb.{t}.weight"] = (rng.uniform(-1, 1, (R, D)) / np.sqrt(R)).astype(np.float32)
        g[f"sparse{t}"] = rng.permutation(R)[:B * L].reshape(B, L).astype(np.int64)
    return g


# ---- the driver's model with --arch-interaction-op dot | dcn, --loss bce, --optimizer adagrad, and its torch float64 twin --------------------
DRV_B, DRV_D, DRV_ROWS, DRV_BOT = 128, 16, (1000,) * 8, (13, 64, 16)
DCN_L, DCN_R = 2, 8
RTOL, ATOL = 2e-5, 2e-6          # the bound of test_adam_optimizer_matches_torch_on_gpu (tests/test_gpu_model.py)


def driver_args(backend, interaction, extra=()):
    C = 1 + len(DRV_ROWS)
    width = DRV_BOT[-1] + (C * C if interaction == "dot" else len(DRV_ROWS) * DRV_D)
    a = ["--backend", backend, "-b", str(DRV_B), "--arch-sparse-feature-size", str(DRV_D), "--arch-embedding-size", "-".join(map(str, DRV_ROWS)),
         "--arch-mlp-bot", "-".join(map(str, DRV_BOT)), "--arch-mlp-top", f"{width}-64-1", "--arch-interaction-op", interaction,
         "--data-size", str(DRV_B), "--loss", "bce", "--optimizer", "adagrad"]
    if interaction == "dcn":
        a += ["--dcn-num-layers", str(DCN_L), "--dcn-low-rank-dim", str(DCN_R)]
    return a + list(extra)


class TorchTwin:
    """float64 parameters keyed "<layer name>/<weight index>" as the host layer names them, under torch.optim.Adagrad"""

    def __init__(self, m, interaction, lr, eps, acc):
        import torch
        self.interaction = interaction
        names = [m.layer_name(i) for i in range(m.num_layers)]
        self.P = {}
        for li, n in enumerate(names):
            for i in range(m.layer_num_weights(li)):
                self.P[f"{n}/{i}"] = torch.tensor(m.parameter(li, i).get_weights().astype(np.float64), requires_grad=True)
        self.dense = [n for n in names if n.startswith("Dense")]
        self.emb = [n for n in names if n.startswith("Embedding")]
        assert len(self.emb) == len(DRV_ROWS) and len(self.dense) == len(DRV_BOT) - 1 + 2 + (2 * DCN_L if interaction == "dcn" else 0), names
        self.opt = torch.optim.Adagrad(list(self.P.values()), lr=lr, lr_decay=0, weight_decay=0, initial_accumulator_value=acc, eps=eps)

    def _lin(self, name, x):
        y = x @ self.P[name + "/0"].T
        return y + self.P[name + "/1"] if name + "/1" in self.P else y

    def forward(self, dense, sparse):
        import torch
        nb = len(DRV_BOT) - 1
        x = dense
        for n in self.dense[:nb]:
            x = torch.relu(self._lin(n, x))
        ly = [self.P[n + "/0"][s].sum(1) for n, s in zip(self.emb, sparse)]
        cat = torch.cat([x] + ly, 1)
        if self.interaction == "dcn":
            xl = cat
            for l in range(DCN_L):
                xl = cat * self._lin(self.dense[nb + 2 * l + 1], self._lin(self.dense[nb + 2 * l], xl)) + xl
            z, tops = xl, self.dense[nb + 2 * DCN_L:]
        else:      # "dot": [x | vec(Z Z^T)], Z the 1 + #tables vectors of a sample
            Z = cat.reshape(cat.shape[0], 1 + len(ly), DRV_D)
            z, tops = torch.cat([x, (Z @ Z.transpose(1, 2)).reshape(cat.shape[0], -1)], 1), self.dense[nb:]
        for i, n in enumerate(tops):
            z = self._lin(n, z)
            z = torch.sigmoid(z) if i == len(tops) - 1 else torch.relu(z)
        return z

    def step(self, dense, sparse, label):
        import torch
        self.opt.zero_grad()
        p = self.forward(dense, sparse)
        (torch.nn.functional.binary_cross_entropy(p, label, reduction="sum") / p.shape[0]).backward()
        self.opt.step()
        return p.detach().numpy()


def run_driver_model(backend, interaction, steps, trace, want_torch, acc=0.0, eps=1e-10, lr=0.01):
    """Warm-up + steps - 1 training steps on the resident batch.  Returns (got, exp): parameters after `steps` optimizer steps and the prediction
    of the last forward, from the host layer (float32) and from the torch twin (float64; None unless want_torch)."""
    import torch
    app = ffmodel.DLRM(driver_args(backend, interaction, ["--lr", str(lr), "--adagrad-eps", str(eps), "--adagrad-initial-accumulator", str(acc)]))
    m = app.model
    tm = TorchTwin(m, interaction, lr, eps, acc) if want_torch else None
    app.warmup()
    app.train_steps(steps - 1, trace=trace)
    m.sync()
    got = {f"{m.layer_name(l)}/{i}": m.parameter(l, i).get_weights() for l in range(m.num_layers) for i in range(m.layer_num_weights(l))}
    got["pred"] = m.layer_output(m.num_layers - 1).get()
    exp = None
    if want_torch:
        dense = torch.from_numpy(app.dense_input().get().astype(np.float64))
        sparse = [torch.from_numpy(app.sparse_input(t).get(np.int64)) for t in range(len(DRV_ROWS))]
        label = torch.from_numpy(m.label_tensor.get().astype(np.float64))
        for _ in range(steps):
            pred = tm.step(dense, sparse, label)
        exp = {k: v.detach().numpy() for k, v in tm.P.items()}
        exp["pred"] = pred
    app.close()
    return got, exp
