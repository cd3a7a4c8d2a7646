"""Shared by the learning-rate schedule tests: the schedule of include/ff_hip_lr.h restated in numpy float64, and a runner of the tiny golden
DLRM (tests/dlrm_helpers.py) that records the scheduled rate before every step, the predictions and the final parameters."""
import numpy as np

import dlrm_helpers as H


def schedule_f64(k, base, W, S, N):
    """The table of the header, in float64: warm-up, base, quadratic decay with the 1e-7 floor, then the last decayed value."""
    k, base = int(k), np.float64(base)
    if k < W:
        return float(base * (np.float64(k + 1) / np.float64(W)))
    if N > 0 and k >= S:
        kk = min(k, S + N - 1)
        r = np.float64(S + N - kk) / np.float64(N)
        return float(max(np.float64(1e-7), base * r * r))
    return float(base)


def schedule_f32(k, base, W, S, N):
    return float(np.float32(schedule_f64(k, base, W, S, N)))


# name -> (extra flags, (optimizer kind, base rate))
VARIANTS = {
    "sgd_fp32": (["--deterministic"], ("sgd", 0.01)),
    "sgd_bf16_nearest": (["--deterministic", "--embedding-dtype", "bf16", "--embedding-rounding", "nearest"], ("sgd", 0.01)),
    "sgd_sparse_opt": (["--deterministic", "--sparse-embedding-optimizer"], ("sgd", 0.01)),
    "momentum_sparse_opt": (["--deterministic", "--sparse-embedding-optimizer"], ("momentum", 0.05)),
}


def build(backend, sched, device_lr, flags=(), optimizer=("sgd", 0.01), enable_graph=False, overlap=True, lr_argv=True):
    W, S, N = sched
    argv = list(flags)
    overlap = overlap and "--no-overlap" not in argv
    if lr_argv and (W or S or N):
        argv += ["--lr-num-warmup-steps", str(W), f"--lr-decay-start-step={S}", "--lr-num-decay-steps", str(N)]
    if device_lr is True:
        argv += ["--device-lr"]
    elif device_lr is False:
        argv += ["--host-lr-schedule"]
    kind, base = optimizer
    kw = {}
    if kind == "adam":
        kw["adam"] = dict(H.ADAM_HP, alpha=base)
    elif kind == "momentum":
        kw["sgd"] = dict(H.MOM_HP, lr=base)
    else:
        kw["sgd"] = dict(lr=base)
    return H.build_golden_dlrm(backend, enable_graph=enable_graph, overlap=overlap, extra_argv=argv, **kw)


def params(m, h):
    out = {}
    for k, li in h["names"].items():
        out[f"{k}.weight"] = m.parameter(li, 0).get_weights()
        if not k.startswith("emb"):
            out[f"{k}.bias"] = m.parameter(li, 1).get_weights()
    return out


def step(m, trace=False):
    if trace:
        m.begin_trace(7)
    m.forward(); m.zero_gradients(); m.backward(); m.update()
    if trace:
        m.end_trace(7)
    m.sync()


def run_model(backend, steps, sched, device_lr, flags=(), optimizer=("sgd", 0.01), trace=False, eval_between=False, per_step_state=False):
    m, h = build(backend, sched, device_lr, flags, optimizer, enable_graph=trace)
    out = {"route": m.counter("lr_route"), "uses_graph": bool(m.uses_graph), "lrs": [], "preds": [], "states": []}
    for _ in range(steps):
        out["lrs"].append(m.current_lr())
        step(m, trace)
        out["preds"].append(m.layer_output(h["final"]).get())
        if per_step_state:
            out["states"].append(params(m, h))
        if eval_between:
            m.eval_batch()
            m.sync()
    out["lr_steps"] = m.counter("lr_steps")
    out["replays"] = m.counter("graph_replays")
    out["state"] = params(m, h)
    return out
