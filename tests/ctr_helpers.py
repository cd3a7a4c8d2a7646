"""Shared by the CTR tests (include/ff_hip_ctr.h): numpy / torch restatements of the contract and a way to build the golden DLRM of
dlrm_helpers with another loss."""
import contextlib

import numpy as np

from dlrm_flexflow_amd import capi, ffmodel
import dlrm_helpers as H

K = capi.AUC_BINS


def bce_f64(p, y):
    """The contract's per-element loss in float64 (log clamped at -100)."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    with np.errstate(divide="ignore"):
        return -(y * np.maximum(np.log(p), -100.0) + (1.0 - y) * np.maximum(np.log(1.0 - p), -100.0))


def bins_of(p):
    """bin(p) = min(K - 1, (int)(p * K)) with the product in fp32 (exact: K is a power of two)."""
    t = np.asarray(p, np.float32) * np.float32(K)
    return np.minimum(K - 1, np.maximum(t, 0).astype(np.int64))


def histograms(p, y):
    p, y = np.asarray(p, np.float32).ravel(), np.asarray(y, np.float32).ravel()
    ok = ~np.isnan(p)
    b, pos = bins_of(p[ok]), y[ok] >= 0.5
    return (np.bincount(b[pos], minlength=K).astype(np.uint64), np.bincount(b[~pos], minlength=K).astype(np.uint64))


def auc_formula(hp, hn):
    """numpy restatement of ffh_auc_from_histograms."""
    hp, hn = hp.astype(np.float64), hn.astype(np.float64)
    P, N = hp.sum(), hn.sum()
    if P == 0 or N == 0:
        return float("nan")
    below = np.concatenate([[0.0], np.cumsum(hn)[:-1]])
    return float((hp * (below + 0.5 * hn)).sum() / (P * N))


def auc_pairs(p, y):
    """Exact pair-counting AUC (Mann-Whitney U, ties one half) in float64 from average ranks."""
    p, pos = np.asarray(p, np.float64).ravel(), np.asarray(y).ravel() >= 0.5
    P, N = int(pos.sum()), int((~pos).sum())
    if P == 0 or N == 0:
        return float("nan")
    _, inv, cnt = np.unique(p, return_inverse=True, return_counts=True)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])            # 0-based rank of the first member of each tie group
    avg_rank = first + (cnt + 1) / 2.0                            # 1-based average rank
    r = avg_rank[inv]
    return float((r[pos].sum() - P * (P + 1) / 2.0) / (float(P) * float(N)))


@contextlib.contextmanager
def compile_as(loss, metrics, comp_mode=ffmodel.COMP_MODE_TRAINING):
    """H.build_golden_dlrm calls compile() with its defaults: inside this block the defaults are `loss` / `metrics`."""
    orig = ffmodel.FFModel.compile

    def patched(self, *a, **k):
        return orig(self, loss, metrics, comp_mode)
    ffmodel.FFModel.compile = patched
    try:
        yield
    finally:
        ffmodel.FFModel.compile = orig


BCE_METRICS = (ffmodel.METRICS_ACCURACY, ffmodel.METRICS_BCE)


def build_bce_dlrm(backend, **kw):
    with compile_as(ffmodel.LOSS_BCE, BCE_METRICS):
        return H.build_golden_dlrm(backend, **kw)


def torch_bce_sgd_reference(g, steps, lr=0.01):
    """The golden DLRM in torch on the CPU with binary_cross_entropy (sum / global batch) and plain SGD; records like H.run_steps()."""
    import torch
    import torch.nn.functional as F
    rows, bot, top = list(g["rows"]), list(g["bot"]), list(g["top"])
    B = int(g["B"])
    P = {}
    for i in range(len(bot) - 1):
        P[f"bot.{i}.weight"] = g[f"init/bot.{i}.weight"]; P[f"bot.{i}.bias"] = g[f"init/bot.{i}.bias"]
    for i in range(len(top) - 1):
        P[f"top.{i}.weight"] = g[f"init/top.{i}.weight"]; P[f"top.{i}.bias"] = g[f"init/top.{i}.bias"]
    for t in range(len(rows)):
        P[f"emb.{t}.weight"] = g[f"init/emb.{t}.weight"]
    P = {k: torch.tensor(np.array(v, np.float32), requires_grad=True) for k, v in P.items()}
    dense, label = torch.from_numpy(g["dense"]), torch.from_numpy(g["label"])
    sparse = [torch.from_numpy(g[f"sparse{t}"]) for t in range(len(rows))]
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
        for v in P.values():
            v.grad = None
        loss = F.binary_cross_entropy(z, label.reshape(z.shape), reduction="sum")
        (loss / B).backward()
        with torch.no_grad():
            for w in P.values():
                w -= lr * w.grad
        rec = {"pred": z.detach().numpy().copy(), "bce_sum": float(loss.detach())}
        rec.update({k: v.detach().numpy().copy() for k, v in P.items()})
        out.append(rec)
    return out


def train_then_evaluate(m, train_steps, eval_calls=2):
    """`train_steps` steps, then `eval_calls` eval_batch() calls on the resident inputs; the global figures and histograms as arrays."""
    for _ in range(train_steps):
        m.forward(); m.zero_gradients(); m.backward(); m.update()
    m.reset_eval_metrics()
    for _ in range(eval_calls):
        m.eval_batch()
    e = m.eval_metrics(histograms=True)
    return {"counts": np.array([e["samples"], e["positives"], e["correct"], e["nan_predictions"]], np.uint64),
            "logloss_sum": np.array(e["logloss_sum"]), "auc": np.array(e["auc"]), "hist_pos": e["hist_pos"], "hist_neg": e["hist_neg"]}
