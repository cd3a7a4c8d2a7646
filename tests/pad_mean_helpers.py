"""Helpers of the pad-mean tests (include/ff_hip_pad_mean.h): id patterns with the counts 0, 1 and L pinned, the header's references restated
on the host, and a runner for the mean update.

THE REFERENCES (the header's identities 2 and 3, bit for bit): the EXISTING pad entries of include/ff_hip_pad.h in SUM mode -- the gather's
output multiplied on the host in float32 by float32(1) / float32(max(count, 1)); the update run on gradient rows divided on the host in float32
by float32(max(count, 1))."""
import numpy as np

import bf16_helpers as B
import pad_helpers as PH
from dlrm_flexflow_amd import capi, ffmodel

DEV = PH.DEV
SUM, AVG = capi.AGGR_MODE_SUM, capi.AGGR_MODE_AVG
EMPTY_BAG, FULL_BAG, ONE_BAG = 2, 3, 4      # the bags pin_counts sets by hand


def pin_counts(ids, R):
    """`ids` [batch][L] with three bags set by hand where L > 1: one empty, one full, one with exactly one lookup (its last slot) -- so the counts
    0, 1 and L are there whatever the pattern's mask drew.  In place; returns ids."""
    batch, L = ids.shape
    if L > 1:
        assert batch > ONE_BAG
        ids[EMPTY_BAG, :] = PH.PAD
        ids[FULL_BAG, :] = (np.arange(L) * 7 + 1) % R
        ids[ONE_BAG, :] = PH.PAD
        ids[ONE_BAG, -1] = (R - 1) // 2
    return ids


def inv_count(ids):
    """float32(1) / float32(max(count, 1)) per bag"""
    return np.float32(1) / np.maximum(ffmodel.padded_bag_counts(ids), 1).astype(np.float32)


def start(rule, wt, D, batch, bags, rows, pattern, tag=0, ids=None, pin=True):
    """pad_helpers.start with the three pinned bags per table (`pin`; never on ids given by the caller)."""
    tables = PH.start(rule, wt, D, batch, bags, rows, pattern, tag, ids)
    if pin and ids is None:
        for tb in tables:
            pin_counts(tb["idx"], tb["R"])
            tb["hit"][:] = False
            tb["hit"][tb["idx"][tb["idx"] >= 0]] = True
    return tables


class MeanRunner(PH.UpdateRunner):
    """UpdateRunner on a workspace sized by the pad-mean query.  `mean()` runs the mean entry (fused, or the pad sort and the mean apply) with
    FFH_AGGR_MODE_AVG; `ref()` is identity 3: UpdateRunner.pad() -- the existing pad entry in SUM mode -- on the pre-divided gradient rows."""

    def __init__(self, hip, tables, rule, wt, D, batch, **kw):
        super().__init__(hip, tables, rule, wt, D, batch, **kw)
        self.pm = capi.pad_mean_api(hip)
        self.old_ws_bytes = self.bu.workspace_bytes(self.bags, D, batch)
        self.ws_bytes = self.pm.workspace_bytes(self.bags, D, batch) + 256
        assert self.pm.workspace_bytes(self.bags, D, batch) > self.old_ws_bytes
        self.ws = self.torch.empty(self.ws_bytes, dtype=self.torch.uint8, device=DEV)
        hip.set_workspace(self.ws, self.ws_bytes)
        self.g_div = [self.dev(tb["g"] / np.maximum(ffmodel.padded_bag_counts(tb["idx"]), 1).astype(np.float32)[:, None]) for tb in tables]

    def mean(self, pair=False):
        w, s0, s1 = self.fresh()
        u = self.descriptor(w, s0, s1, aggr=AVG)
        if pair:
            self.pd.sort(u)
            self.pm.apply(u)
        else:
            self.pm.fused(u)
        out = self.host(w, s0, s1)
        self.route = self.hip.lib.ffh_embedding_last_route(self.hip.ctx).decode()
        return out

    def ref(self, pair=False):
        g, self.g = self.g, self.g_div
        try:
            return PH.UpdateRunner.pad(self, pair)
        finally:
            self.g = g

    def plain_avg(self):
        """the existing ragged update with FFH_AGGR_MODE_AVG on the same tables (ids without pads only)"""
        w, s0, s1 = self.fresh()
        self.bu.call(self.descriptor(w, s0, s1, aggr=AVG))
        return self.host(w, s0, s1)


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
GATHER_BAGS = (1, 3, 4, 7, 100)


def gather_rows(t):
    return 23 + 17 * t


def gather_case(D, batch, bf16, pattern):
    """The tables and ids of tests/test_gpu_pad.py's gather cases, with the three pinned bags."""
    rng = np.random.default_rng([PH.SEED, D, batch])
    W, ids = [], []
    for t, L in enumerate(GATHER_BAGS):
        w = rng.standard_normal((gather_rows(t), D)).astype(np.float32)
        w[0, :] = -0.0
        if bf16:
            w = B.widen(B.rne(w))
        i = rng.integers(0, gather_rows(t), (batch, L)).astype(np.int64)
        i[1, :] = 0
        W.append(w)
        ids.append(pin_counts(PH.apply_pattern(i, pattern, t, len(GATHER_BAGS)), gather_rows(t)))
    return W, ids


def gather(hip, W, ids, D, batch, bf16, which):
    """[batch][ld] with 7.0 where nothing may be written.  which: "mean" (the mean entry, AVG), "pad-sum" (the existing pad entry, SUM) or
    "plain-avg" (the existing ragged entry, AVG: only for ids without pads)."""
    import torch
    bags, b16 = capi.bags_api(hip), capi.bf16_api(hip)
    nt, ld = len(GATHER_BAGS), 4 + len(GATHER_BAGS) * D + 4
    out = torch.full((batch, ld), 7.0, device=DEV)
    conv = (lambda w: torch.from_numpy(B.rne(w).view(np.int16)).to(DEV)) if bf16 else (lambda w: torch.from_numpy(w).to(DEV))
    wd = [conv(w) for w in W]
    idd = [torch.from_numpy(i).to(DEV) for i in ids]
    ent = [(idd[t], wd[t], out.data_ptr() + 4 * (4 + t * D), gather_rows(t), ld) for t in range(nt)]
    arr = b16.tables(ent) if bf16 else hip.emb_tables(ent)
    dims = bags.in_dims(GATHER_BAGS)
    if which == "mean":
        capi.pad_mean_api(hip).fwd(arr, dims, nt, D, batch, AVG, bf16=bf16)
    elif which == "pad-sum":
        capi.pad_api(hip).fwd(arr, dims, nt, D, batch, SUM, bf16=bf16)
    else:
        assert which == "plain-avg"
        bags.call("ffh_embedding_fwd_multi_bags_bf16" if bf16 else "ffh_embedding_fwd_multi_bags", arr, dims, nt, D, batch, AVG)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- the host model ------------------------------------------------------------------------------------------------------------------------
def build_pad_mean_model(backend, cfg, data, extra_argv=()):
    """pad_helpers.build_pad_model with every table pooling AGGR_MODE_AVG: FFConfig.set(embedding_padding=True), plain SGD, one rank."""
    Bn, D = cfg["B"], cfg["D"]
    rows, bags, bot, top = cfg["rows"], cfg["bags"], cfg["bot"], cfg["top"]
    c = ffmodel.FFConfig(argv=["-b", str(Bn)] + list(extra_argv), backend=backend)
    c.set(enable_graph=False, overlap_embedding=True, dense_embedding_update=False, embedding_padding=True)
    m = ffmodel.FFModel(c)
    sparse = [m.create_tensor([Bn, L], ffmodel.DT_INT64) for L in bags]
    dense = m.create_tensor([Bn, bot[0]], ffmodel.DT_FLOAT)
    x = dense
    for i in range(len(bot) - 1):
        x = m.dense(x, bot[i + 1], capi.AC_MODE_RELU)
    ly = [m.embedding(s, r, D, capi.AGGR_MODE_AVG) for s, r in zip(sparse, rows)]
    z = m.concat([x] + ly, 1)
    for i in range(len(top) - 1):
        z = m.dense(z, top[i + 1], capi.AC_MODE_SIGMOID if i == len(top) - 2 else capi.AC_MODE_RELU)
    m.set_sgd_optimizer(lr=cfg["lr"])
    m.compile()
    m.init_layers()
    names, layer = {}, 0
    for i in range(len(bot) - 1):
        names[f"bot.{i}"] = layer; layer += 1
    for t in range(len(rows)):
        names[f"emb.{t}"] = layer; layer += 1
    layer += 1
    for i in range(len(top) - 1):
        names[f"top.{i}"] = layer; layer += 1
    assert layer == m.num_layers
    dense.set(data["dense"])
    m.label_tensor.set(data["label"])
    for t, s in enumerate(sparse):
        s.set(data[f"sparse{t}"])      # (-1 goes in unchanged)
    init = {}
    for k, li in names.items():
        init[f"{k}.weight"] = m.parameter(li, 0).get_weights()
        if not k.startswith("emb"):
            init[f"{k}.bias"] = m.parameter(li, 1).get_weights()
    return m, {"names": names, "final": m.num_layers - 1, "data": data, "init": init, "cfg": cfg}


def mean_reference(h, steps):
    """The float64 model of tests/bags_helpers.py (numpy_reference) with a mean over the lookups that are there: forward sum / count, a row's
    gradient the sum of g / count over the lookups that hit it, a pad and an empty bag contribute nothing.  Per-step records like
    dlrm_helpers.run_steps."""
    cfg, d = h["cfg"], h["data"]
    Bn, lr = cfg["B"], cfg["lr"]
    nb, nt, T = len(cfg["bot"]) - 1, len(cfg["top"]) - 1, len(cfg["rows"])
    P = {k: np.array(v, np.float64) for k, v in h["init"].items()}
    live = [d[f"sparse{t}"] >= 0 for t in range(T)]
    cnt = [np.maximum(l.sum(1), 1).astype(np.float64) for l in live]
    safe = [np.where(l, d[f"sparse{t}"], 0) for t, l in enumerate(live)]
    out = []
    for _ in range(steps):
        acts, x = [], d["dense"].astype(np.float64)
        for i in range(nb):
            acts.append(x)
            x = np.maximum(x @ P[f"bot.{i}.weight"].T + P[f"bot.{i}.bias"], 0.0)
        xb = x
        ly = [(P[f"emb.{t}.weight"][safe[t]] * live[t][:, :, None]).sum(1) / cnt[t][:, None] for t in range(T)]
        z = np.concatenate([xb] + ly, 1)
        tacts = []
        for i in range(nt):
            tacts.append(z)
            z = z @ P[f"top.{i}.weight"].T + P[f"top.{i}.bias"]
            z = 1.0 / (1.0 + np.exp(-z)) if i == nt - 1 else np.maximum(z, 0.0)
        pred = z
        G = {}
        g = (pred - d["label"]) / Bn
        y = pred
        for i in reversed(range(nt)):
            g = g * (y * (1.0 - y)) if i == nt - 1 else g * (y > 0)
            G[f"top.{i}.weight"] = g.T @ tacts[i]
            G[f"top.{i}.bias"] = g.sum(0)
            g = g @ P[f"top.{i}.weight"]
            y = tacts[i]
        D, w0 = cfg["D"], cfg["bot"][-1]
        for t in range(T):
            ge = g[:, w0 + t * D:w0 + (t + 1) * D] / cnt[t][:, None]
            gw = np.zeros_like(P[f"emb.{t}.weight"])
            L = cfg["bags"][t]
            rep = np.repeat(ge, L, axis=0) * live[t].reshape(-1)[:, None]
            np.add.at(gw, safe[t].reshape(-1), rep)
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
