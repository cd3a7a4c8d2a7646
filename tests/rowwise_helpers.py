"""Shared by tests/test_gpu_rowwise_model.py, tests/test_gpu_rowwise_ranks.py and tests/_dist_worker_rowwise.py: the driver's DLRM of
tests/adagrad_helpers.py run with --adagrad-rowwise beside a torch float64 twin whose dense parameters are under torch.optim.Adagrad and whose
tables follow the row-wise rule written out here; and how a test reads the tables' row state (a checkpoint's sparse_state0 records)."""
import os

import numpy as np

from dlrm_flexflow_amd import ffmodel
import adagrad_helpers as A


def row_states(m, directory):
    """{operator name: S, float32 [rows]} of the tables this rank holds, from a checkpoint of `m` written to `directory`"""
    m.save_checkpoint(str(directory))
    files = [f for f in os.listdir(str(directory)) if f.endswith(".ffck")]
    assert len(files) == 1, files
    ck = ffmodel.read_checkpoint(os.path.join(str(directory), files[0]))
    assert ck["meta"]["optimizer"] == "adagrad-rowwise", ck["meta"]["optimizer"]
    out = {}
    for name, r in ck["meta"]["records"].items():
        if name.startswith("sparse_state0/"):
            assert r["cols"] == 1 and r["type"] == "f32", (name, r)
            out[name.split("/")[1]] = np.array(ck[name]).reshape(-1)
    assert not any(n.startswith("sparse_state1/") for n in ck["meta"]["records"])
    return out


class RowwiseTwin(A.TorchTwin):
    """adagrad_helpers.TorchTwin with the tables taken out of torch.optim.Adagrad and updated by the row-wise rule in float64: S[row] += mean_j g^2,
    w -= lr * g / (sqrt(S) + eps).  A row the batch did not touch has g = 0 and keeps w and S, so the rule runs over every row."""

    def __init__(self, m, interaction, lr, eps, acc):
        import torch
        super().__init__(m, interaction, lr, eps, acc)
        self.lr, self.eps = lr, eps
        dense = [v for k, v in self.P.items() if not k.startswith("Embedding")]
        self.opt = torch.optim.Adagrad(dense, lr=lr, lr_decay=0, weight_decay=0, initial_accumulator_value=acc, eps=eps)
        self.S = {n: torch.full((self.P[n + "/0"].shape[0],), acc, dtype=torch.float64) for n in self.emb}

    def step(self, dense, sparse, label):
        import torch
        for n in self.emb:
            self.P[n + "/0"].grad = None
        pred = super().step(dense, sparse, label)
        with torch.no_grad():
            for n in self.emb:
                w = self.P[n + "/0"]
                g = w.grad
                self.S[n] += (g * g).mean(dim=1)
                w -= self.lr * g / (torch.sqrt(self.S[n]) + self.eps)[:, None]
        return pred


def run_driver_model(backend, interaction, steps, trace, want_torch, directory, acc=0.0, eps=1e-10, lr=0.01, extra=()):
    """adagrad_helpers.run_driver_model with --adagrad-rowwise: (got, exp), parameters after `steps` optimizer steps, the tables' row state as
    "S/<operator>" and the prediction of the last forward, from the host layer (float32) and from the twin (float64; None unless want_torch)."""
    import torch
    args = A.driver_args(backend, interaction, ["--lr", str(lr), "--adagrad-eps", str(eps), "--adagrad-initial-accumulator", str(acc), "--adagrad-rowwise",
                                                *extra])
    app = ffmodel.DLRM(args)
    m = app.model
    tm = RowwiseTwin(m, interaction, lr, eps, acc) if want_torch else None
    app.warmup()
    app.train_steps(steps - 1, trace=trace)
    m.sync()
    got = {f"{m.layer_name(l)}/{i}": m.parameter(l, i).get_weights() for l in range(m.num_layers) for i in range(m.layer_num_weights(l))}
    got["pred"] = m.layer_output(m.num_layers - 1).get()
    for name, S in row_states(m, directory).items():
        got["S/" + name] = S
    exp = None
    if want_torch:
        dense = torch.from_numpy(app.dense_input().get().astype(np.float64))
        sparse = [torch.from_numpy(app.sparse_input(t).get(np.int64)) for t in range(len(A.DRV_ROWS))]
        label = torch.from_numpy(m.label_tensor.get().astype(np.float64))
        for _ in range(steps):
            pred = tm.step(dense, sparse, label)
        exp = {k: v.detach().numpy() for k, v in tm.P.items()}
        exp.update({"S/" + n: s.numpy() for n, s in tm.S.items()})
        exp["pred"] = pred
    app.close()
    return got, exp
