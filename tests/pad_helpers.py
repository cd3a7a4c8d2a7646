"""Helpers of the pad tests (include/ff_hip_pad.h): pad patterns, the zero-row reference the header defines, and a runner for the update.

THE REFERENCE (the header's, bit for bit): append one all-zero row R to the table of R rows (and one state row where the rule has state),
replace every pad by R, and call the EXISTING ragged entries on that.  Rows [0, R) of the weights and of every state array, and the whole
gather output, must equal the pad entries' on the table of R rows."""
import numpy as np

import bf16_helpers as B
from dlrm_flexflow_amd import capi, ffmodel

DEV = "cuda:0"
SEED = 0x9AD
IT = 5      # the bf16 update counter
EPS = 1e-10
PAD = capi.EMB_PAD_ID
PATTERNS = ("none", "all", "first", "last", "one-table", "mask")
KINDS = {"sgd": capi.SPARSE_OPT_SGD, "momentum": capi.SPARSE_OPT_SGD_MOMENTUM, "adam": capi.SPARSE_OPT_ADAM,
         "adagrad": capi.SPARSE_OPT_ADAGRAD, "rowwise": capi.SPARSE_OPT_ROWWISE_ADAGRAD}


def apply_pattern(ids, pattern, t, nt, seed=SEED):
    """`ids` [batch][L] of table t (of nt) with the pads of `pattern` set, as a copy."""
    ids = ids.copy()
    if pattern == "all":
        ids[:] = PAD
    elif pattern == "first":
        ids[:, 0] = PAD
    elif pattern == "last":
        ids[:, -1] = PAD
    elif pattern == "one-table":
        if t == nt // 2:
            ids[:] = PAD
    elif pattern == "mask":      # the synthetic generator's pads at fill 0.5, a stream per table
        keep = ffmodel.pad_mask_reference(seed + t, 0, ids.size, 0.5).reshape(ids.shape)
        ids[~keep] = PAD
    else:
        assert pattern == "none"
    return ids


def to_zero_row(ids, R):
    """the reference's ids: every pad points at the appended row R"""
    return np.where(ids < 0, R, ids)


def extend(a):
    """one more all-zero row (a state vector of a row-wise rule: one more zero)"""
    return None if a is None else np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)])


def opt_of(rule, rate):
    o = capi.SparseOpt()
    o.kind = KINDS[rule]
    o.lr = rate
    o.beta1, o.beta2 = 0.9, 0.999
    o.epsilon = 1e-8 if rule == "adam" else EPS
    if rule == "momentum":
        o.weight_decay, o.momentum, o.nesterov = 1e-3, 0.9, 1
    elif rule == "adam":
        o.weight_decay = 1e-4
    return o


def start(rule, wt, D, batch, bags, rows, pattern, tag=0, ids=None):
    """Host side of an update case: per table the ids (pads set), the gradient rows, the weights (bf16: the bits) and the rule's state."""
    rng = np.random.default_rng([SEED, batch, D, tag] + list(bags) + list(rows))
    tables = []
    for t, (L, R) in enumerate(zip(bags, rows)):
        i = apply_pattern(rng.integers(0, R, (batch, L)), pattern, t, len(bags)) if ids is None else ids[t]
        w = (rng.standard_normal((R, D)) * 0.1).astype(np.float32)
        s0 = s1 = None
        if rule == "momentum":
            s0 = (np.abs(rng.standard_normal((R, D))) * 0.01).astype(np.float32)
        elif rule == "adam":
            s0 = (rng.standard_normal((R, D)) * 0.01).astype(np.float32)
            s1 = (np.abs(rng.standard_normal((R, D))) * 0.01).astype(np.float32)
        elif rule == "adagrad":
            s0 = np.full((R, D), 0.1, np.float32)
        elif rule == "rowwise":
            s0 = np.full((R,), 0.1, np.float32)
        hit = np.zeros(R, bool)
        hit[i[i >= 0]] = True
        tables.append(dict(R=R, L=L, idx=i, g=rng.standard_normal((batch, D)).astype(np.float32), w=B.rne(w) if wt == "bf16" else w, s0=s0, s1=s1, hit=hit))
    return tables


class UpdateRunner:
    """One start on the device.  `pad()` runs the pad entry (fused, or the sort / apply pair) on the tables of R rows, `zero_row()` the existing
    ragged entry on the extended tables; each returns the tables' (w, s0, s1) as numpy -- zero_row() cut back to R rows."""

    def __init__(self, hip, tables, rule, wt, D, batch, mode=B.ROUND_NEAREST, plain=False, lr_block=False):
        import torch
        self.torch, self.hip = torch, hip
        self.lr, self.b16, self.bu, self.bs, self.pd = capi.lr_api(hip), capi.bf16_api(hip), capi.bags_update_api(hip), capi.bags_sort_api(hip), capi.pad_api(hip)
        self.tables, self.rule, self.wt, self.D, self.batch, self.mode, self.plain, self.lr_block = tables, rule, wt, D, batch, mode, plain, lr_block
        self.bags = [tb["L"] for tb in tables]
        self.g = [self.dev(tb["g"]) for tb in tables]
        self.idx = [self.dev(tb["idx"]) for tb in tables]
        self.idx_ref = [self.dev(to_zero_row(tb["idx"], tb["R"])) for tb in tables]
        self.blk = torch.zeros(self.lr.state_bytes(), dtype=torch.uint8, device=DEV)
        self.lr.init(self.blk, 0.05, 3, 3, 4, 0.9, 0.999, 1)      # mid warm-up: neither rate is the base
        v = self.lr.read(self.blk)
        self.rate = float(np.float32(v.alpha_t if rule == "adam" else v.lr))
        self.ws_bytes = self.bu.workspace_bytes(self.bags, D, batch) + 256
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)
        hip.set_workspace(self.ws, self.ws_bytes)
        self.route = None

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)

    def fresh(self, extended=False):
        f = extend if extended else (lambda a: a)
        return tuple([self.dev(f(tb[k])) for tb in self.tables] for k in ("w", "s0", "s1"))

    def host(self, w, s0, s1):
        self.torch.cuda.synchronize()
        h = lambda ts: [None if x is None else x.cpu().numpy()[:tb["R"]] for x, tb in zip(ts, self.tables)]
        return dict(w=[x.view(np.uint16) if self.wt == "bf16" else x for x in h(w)], s0=h(s0), s1=h(s1))

    def descriptor(self, w, s0, s1, extended=False, **over):
        idx, more = (self.idx_ref, 1) if extended else (self.idx, 0)
        ent = [(idx[t], w[t], self.g[t], tb["R"] + more, self.D) for t, tb in enumerate(self.tables)]
        kw = dict(in_dims=self.bags, out_dim=self.D, batch=self.batch, aggr=capi.AGGR_MODE_SUM, states=self.hip.emb_states(list(zip(s0, s1))))
        if self.wt == "fp32":
            kw["tables"] = self.hip.emb_tables(ent)
        else:
            kw["tables_bf16"] = self.b16.tables([e + (10 + t, 0) for t, e in enumerate(ent)])
            kw["rounding"] = self.b16.rounding(self.mode, SEED, self.torch.tensor([IT], dtype=self.torch.int64, device=DEV))
        if self.plain:
            kw["lr"], kw["states"] = self.rate, None
        else:
            kw["opt"] = opt_of(self.rule, 123.0 if self.lr_block else self.rate)      # (with an lr_block opt.lr is ignored)
            if self.lr_block:
                kw["lr_block"] = self.blk
        kw.update(over)
        return capi.BagsUpdateApi.descriptor(**kw)

    def pad(self, pair=False):
        w, s0, s1 = self.fresh()
        u = self.descriptor(w, s0, s1)
        if pair:
            self.pd.sort(u)
            self.pd.apply(u)
        else:
            self.pd.fused(u)
        out = self.host(w, s0, s1)
        self.route = self.hip.lib.ffh_embedding_last_route(self.hip.ctx).decode()
        return out

    def zero_row(self):
        w, s0, s1 = self.fresh(extended=True)
        self.bu.call(self.descriptor(w, s0, s1, extended=True))
        return self.host(w, s0, s1)


def assert_same(tables, got, ref, what=""):
    """bit for bit, and: rows no real lookup hit keep the bits they started with"""
    for t, tb in enumerate(tables):
        hit = tb["hit"]
        for k in ("w", "s0", "s1"):
            a, r, s = got[k][t], ref[k][t], tb[k]
            if a is None:
                assert r is None and s is None
                continue
            bits = lambda x: x.view(np.uint32) if x.dtype == np.float32 else x
            np.testing.assert_array_equal(bits(a), bits(r), err_msg=f"{what} table {t} (bag {tb['L']}, {tb['R']} rows): {k} differs from the zero-row reference")
            np.testing.assert_array_equal(bits(a[~hit]), bits(s[~hit]), err_msg=f"{what} table {t}: {k}: rows no lookup hit have moved")
        if hit.any():
            assert not np.array_equal(got["w"][t][hit], tb["w"][hit]), f"{what} table {t}: the update did not run"


# ---- the host model ------------------------------------------------------------------------------------------------------------------------
def model_data(cfg, seed=3):
    """Inputs of build_pad_model: the ids of tests/bags_helpers.py's SMALL-style model with pads set -- the generator's at fill 0.5, then one empty
    bag (sample 0 of table 0), one bag with its last slot alone padded, and the LAST table's whole batch."""
    B, rows, bags, bot = cfg["B"], cfg["rows"], cfg["bags"], cfg["bot"]
    rng = np.random.default_rng(seed)
    data = {"dense": rng.random((B, bot[0]), dtype=np.float32), "label": rng.integers(0, 2, (B, 1)).astype(np.float32)}
    for t, (r, L) in enumerate(zip(rows, bags)):
        data[f"sparse{t}"] = apply_pattern(rng.integers(0, r, (B, L)).astype(np.int64), "mask", t, len(rows))
    data["sparse0"][0, :] = PAD
    data["sparse1"][1, :] = 0
    data["sparse1"][1, -1] = PAD
    data[f"sparse{len(rows) - 1}"][:] = PAD
    return data


def build_pad_model(backend, cfg, data, extra_argv=(), comm=None, rank=0, world=1):
    """The cat-interaction DLRM of tests/bags_helpers.py (build_mixed_model) with FFConfig.set(embedding_padding=True), plain SGD; `data` holds the
    GLOBAL batch (this rank's slice of the dense features and labels is set, and every id of the tables it holds).  Returns (model, handles)."""
    B, D = cfg["B"], cfg["D"]
    rows, bags, bot, top = cfg["rows"], cfg["bags"], cfg["bot"], cfg["top"]
    c = ffmodel.FFConfig(argv=["-b", str(B)] + list(extra_argv), backend=backend, comm=comm)
    c.set(enable_graph=False, overlap_embedding=True, dense_embedding_update=False, embedding_padding=True)
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
    names, layer = {}, 0
    for i in range(len(bot) - 1):
        names[f"bot.{i}"] = layer; layer += 1
    for t in range(len(rows)):
        names[f"emb.{t}"] = layer; layer += 1
    layer += 1
    for i in range(len(top) - 1):
        names[f"top.{i}"] = layer; layer += 1
    assert layer == m.num_layers
    sl = slice(rank * B // world, (rank + 1) * B // world)
    dense.set(data["dense"][sl])
    m.label_tensor.set(data["label"][sl])
    for t, s in enumerate(sparse):
        if s.is_local:
            s.set(data[f"sparse{t}"])      # (-1 goes in unchanged)
            assert np.array_equal(s.get(np.int64).reshape(B, -1), data[f"sparse{t}"])
    init = {}
    for k, li in names.items():
        p = m.parameter(li, 0)
        if p.is_local:
            init[f"{k}.weight"] = p.get_weights()
        if not k.startswith("emb"):
            init[f"{k}.bias"] = m.parameter(li, 1).get_weights()
    return m, {"names": names, "final": m.num_layers - 1, "data": data, "init": init, "cfg": cfg}


def masked_reference(h, steps):
    """The float64 model of tests/bags_helpers.py with the pads masked out: every table gets a zero row R that the pads point at, and that row is
    cleared again after every step (a pad reads nothing and moves nothing).  Per-step records like dlrm_helpers.run_steps, tables cut back to R rows."""
    import bags_helpers as BH
    cfg, T = h["cfg"], len(h["cfg"]["rows"])
    data = dict(h["data"])
    init = dict(h["init"])
    for t, R in enumerate(cfg["rows"]):
        data[f"sparse{t}"] = to_zero_row(data[f"sparse{t}"], R)
        init[f"emb.{t}.weight"] = extend(np.asarray(init[f"emb.{t}.weight"], np.float64))
    out = []
    for _ in range(steps):
        rec = BH.numpy_reference({"cfg": cfg, "data": data, "init": init}, 1)[0]
        for t, R in enumerate(cfg["rows"]):
            rec[f"emb.{t}.weight"][R] = 0.0
        init = {k: rec[k] for k in init}
        out.append({k: (v[:cfg["rows"][int(k.split(".")[1])]] if k.startswith("emb.") else v) for k, v in rec.items()})
    return out
