"""GPU tests (-m gpu) of the shuffled data order (--data-randomize total): the gather entry of include/ff_hip_data.h against a numpy
restatement of include/ffh_perm.h bit for bit, and the driver's epochs -- every training sample once, in the restatement's order, the
held-out tail never; shuffling as a pure reordering of the training run; two ranks; eager and replayed steps.  Everything is compared
exactly: a gather moves bits."""
import itertools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
from dlrm_flexflow_amd import capi, ffmodel
import shuffle_helpers as SH

pytestmark = pytest.mark.gpu

HIP = capi.HIP_LIB_PATH
SENTINEL = -7
LOCAL, GLOBAL = capi.GATHER_LOCAL_ROWS, capi.GATHER_GLOBAL_ROWS


# ---- 1. the entry ------------------------------------------------------------------------------------------------------------------------
class _Case:
    """Sources of `tables` id tables, the dense features and the labels for a stripe of n_local rows with `tail` held-out rows behind it,
    destinations with `pad` rows behind the batch, everything on the GPU; one null segment (a table this rank does not hold)."""

    def __init__(self, rng, n_local, Bl, bag, dense_dim, tables, world, rank, tail=5, pad=3, offset=0):
        import torch
        self.n_local, self.Bl, self.world, self.rank, self.pad = n_local, Bl, world, rank, pad
        B = Bl * world
        dev = "cuda:0"

        def shifted(t):
            """`t` behind `offset` elements of its own: a base address that is only element-aligned"""
            if not offset:
                return t
            return torch.cat([torch.zeros(offset, dtype=t.dtype, device=dev), t.reshape(-1)])[offset:].reshape(t.shape)

        self.ids = [rng.integers(0, 1 << 40, (n_local * world + tail * world, bag)).astype(np.int64) for _ in range(tables)]
        self.dense = rng.standard_normal((n_local + tail, dense_dim)).astype(np.float32)
        self.label = rng.standard_normal((n_local + tail, 1)).astype(np.float32)
        self.d_ids = [shifted(torch.from_numpy(a).to(dev)) for a in self.ids]
        self.d_dense, self.d_label = shifted(torch.from_numpy(self.dense).to(dev)), shifted(torch.from_numpy(self.label).to(dev))
        self.o_ids = [shifted(torch.full((B + pad, bag), SENTINEL, dtype=torch.int64, device=dev)) for _ in range(tables)]
        self.o_dense = shifted(torch.full((Bl + pad, dense_dim), float(SENTINEL), dtype=torch.float32, device=dev))
        self.o_label = shifted(torch.full((Bl + pad, 1), float(SENTINEL), dtype=torch.float32, device=dev))
        self.segments = [(s, d, 8 * bag, GLOBAL) for s, d in zip(self.d_ids, self.o_ids)]
        self.segments.insert(min(1, tables), (self.d_ids[0], None, 8 * bag, GLOBAL))        # the null segment, not at the end
        self.segments += [(self.d_dense, self.o_dense, 4 * dense_dim, LOCAL), (self.d_label, self.o_label, 4, LOCAL)]

    def check(self, seed, epoch, step, what):
        import torch
        torch.cuda.synchronize()
        Bl, world = self.Bl, self.world
        p = SH.perm(seed, epoch, self.n_local, np.arange(step * Bl, (step + 1) * Bl))
        g = np.concatenate([SH.global_sample(p, Bl, world, r) for r in range(world)])
        for t, (src, out) in enumerate(zip(self.ids, self.o_ids)):
            got = out.cpu().numpy()
            assert np.array_equal(got[:Bl * world], src[g]), f"{what}: ids of table {t}"
            assert (got[Bl * world:] == SENTINEL).all(), f"{what}: rows behind the batch of table {t} were written"
            assert np.array_equal(self.d_ids[t].cpu().numpy(), src), f"{what}: the source of table {t} changed"
        for name, src, dsrc, out in (("dense", self.dense, self.d_dense, self.o_dense), ("label", self.label, self.d_label, self.o_label)):
            got = out.cpu().numpy()
            assert np.array_equal(got[:Bl].view(np.uint32), src[p].view(np.uint32)), f"{what}: {name}"
            assert (got[Bl:] == SENTINEL).all(), f"{what}: {name} rows behind the batch were written"
            assert np.array_equal(dsrc.cpu().numpy().view(np.uint32), src.view(np.uint32)), f"{what}: the {name} source changed"


def test_batch_gather_equals_the_restatement_bit_for_bit(hip):
    """One launch per case, all in this process.  Stripes of 8, 17, 48, 1028 and 4096 rows (17 and 257 * 4 = 4^k + 1 rows and 4 (4^k + 1): the
    longest walks), one workgroup and several, partial workgroups (Bl = 1, 4, 8, 16), 8- and 24-byte id rows, the 52-byte dense row, 4-byte
    labels, 1 / 3 / 26 tables and a null segment, one rank and the last of two and four.  The last step of the epoch and the first alternate."""
    api = capi.data_api(hip)
    rng = np.random.default_rng(2024)
    shapes = [(8, 8), (17 * 1, 1), (48, 16), (257 * 4, 4), (4096, 2048)]
    n = 0
    for (n_local, Bl), bag, tables, (world, rank) in itertools.product(shapes, [1, 3], [1, 3, 26], [(1, 0), (2, 1), (4, 3)]):
        c = _Case(rng, n_local, Bl, bag, 13, tables, world, rank)
        seed, epoch = 1000 + n, n % 3
        step = (n_local // Bl - 1) if n % 2 == 0 else 0
        api.batch_gather(c.segments, seed, epoch, step, Bl, n_local, world, rank)
        c.check(seed, epoch, step, f"n_local {n_local} Bl {Bl} bag {bag} tables {tables} world {world} rank {rank} step {step}")
        n += 1
    assert n == 90


def test_batch_gather_unit_widths_base_alignment_and_long_segment_lists(hip):
    """What the main sweep's shapes never reach: 16-byte units (bag 2, a 64-byte dense row), bases that are only element-aligned (so an
    8-byte id row sits on an odd 8-byte address and a 64-byte dense row moves in 4-byte units), and more segments than one launch carries."""
    api = capi.data_api(hip)
    rng = np.random.default_rng(7)
    for k, (bag, dense_dim, tables, offset) in enumerate([(2, 16, 3, 0), (2, 16, 3, 1), (1, 13, 3, 1), (1, 13, capi.GATHER_MAX_SEGMENTS + 6, 0)]):
        c = _Case(rng, 130, 65, bag, dense_dim, tables, 2, 0, offset=offset)
        api.batch_gather(c.segments, 99, 4, 1, 65, 130, 2, 0)
        c.check(99, 4, 1, f"case {k}")


def test_batch_gather_refuses_bad_arguments_without_launching(hip):
    api = capi.data_api(hip)
    rng = np.random.default_rng(3)
    c = _Case(rng, 48, 16, 1, 13, 1, 1, 0)
    ok = dict(seed=1, epoch=0, step=0, local_batch=16, n_local=48, world=1, rank=0)
    bad = [dict(step=3), dict(step=-1), dict(rank=1), dict(world=0), dict(n_local=40), dict(local_batch=0), dict(epoch=-1)]
    for change in bad:
        assert api.batch_gather_rc(c.segments, **dict(ok, **change)) == capi.FFH_ERR_BAD_ARG, change
    odd = [(c.d_dense, c.o_dense, 6, LOCAL)]
    assert api.batch_gather_rc(odd, **ok) == capi.FFH_ERR_BAD_ARG
    assert api.batch_gather_rc([(c.d_dense, c.o_dense, 52, 2)], **ok) == capi.FFH_ERR_BAD_ARG
    assert api.batch_gather_rc([(None, c.o_dense, 52, LOCAL)], **ok) == capi.FFH_ERR_BAD_ARG
    import torch
    torch.cuda.synchronize()
    assert (c.o_dense.cpu().numpy() == SENTINEL).all()
    assert api.batch_gather_rc([], **ok) == capi.FFH_OK


# ---- 2. the driver's epochs ----------------------------------------------------------------------------------------------------------------
ROWS = (50, 7, 300)
B, NB_TRAIN, NB_EVAL, SEED = 48, 7, 2, 5
EPOCH_ARGS = ["-b", str(B), "--arch-sparse-feature-size", "8", "--arch-embedding-size", "-".join(map(str, ROWS)), "--arch-mlp-bot", "13-16-8",
              "--arch-mlp-top", "32-16-1", "--eval-batches", str(NB_EVAL), "--seed", str(SEED), "--lr", "1e-6", "--data-randomize", "total"]


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    """(path, arrays) of a file whose label is the sample index: 7 training batches of 48 and 2 held out."""
    data = SH.indexed_dataset((NB_TRAIN + NB_EVAL) * B, ROWS)
    return SH.write_hdf5(str(tmp_path_factory.mktemp("shuffle") / "indexed.h5"), data), data


def _check_epoch(app, data, epoch, trace):
    """One epoch of single steps: after each, the inputs hold the restatement's samples.  Returns the order that was trained on."""
    order = SH.epoch_order(SEED, epoch, NB_TRAIN, B)
    for k in range(NB_TRAIN):
        app.train_steps(1, trace=trace)
        app.model.sync()
        labels = app.label_input().get().reshape(-1)
        idx = labels.astype(np.int64)
        assert np.array_equal(idx, order[k]), f"epoch {epoch} step {k}: trained on {idx[:8]}..., the order says {order[k][:8]}..."
        assert np.array_equal(app.dense_input().get(), data["X_int"][idx])
        for t in range(len(ROWS)):
            assert np.array_equal(app.sparse_input(t).get(np.int64).reshape(-1), data["X_cat"][idx, t])
    assert np.array_equal(np.sort(order.reshape(-1)), np.arange(NB_TRAIN * B))        # every training sample once, no held-out index
    return order


@pytest.mark.parametrize("second_epoch_traced", [False, True], ids=["eager", "traced"])
def test_an_epoch_visits_every_training_sample_once_in_the_stated_order(hip, indexed, second_epoch_traced):
    """Epoch 0 eager, epoch 1 eager or as replayed steps (the batch is loaded outside the trace): labels, ids and dense rows of every step are
    those of the restatement's order, each epoch is a permutation of the 336 training samples, the two orders differ."""
    path, data = indexed
    app = ffmodel.DLRM(["--backend", HIP] + EPOCH_ARGS + ["--dataset", path])
    assert app.num_samples == (NB_TRAIN + NB_EVAL) * B
    first = _check_epoch(app, data, 0, trace=False)
    second = _check_epoch(app, data, 1, trace=second_epoch_traced)
    if second_epoch_traced:
        assert app.model.counter("graph_replays") > 0
    assert not np.array_equal(first, second)
    app.close()


def _parameters(app):
    m = app.model
    out = {}
    for l in range(m.num_layers):
        for i in range(m.layer_num_weights(l)):
            out[f"p{l}.{i}"] = m.parameter(l, i).get_weights()
    return out


def test_shuffling_is_only_a_reordering(hip, tmp_path):
    """--deterministic, one epoch on the golden DLRM shape: `total` on file F leaves every parameter (the whole of every table included) bit-identical
    to `none` on a file that holds F's training samples in epoch 0's order, with the same held-out tail."""
    g = golden("dlrm_step_torch")
    Bg, D, L = int(g["B"]), int(g["D"]), int(g["L"])
    rows, bot, top = [int(r) for r in g["rows"]], [int(x) for x in g["bot"]], [int(x) for x in g["top"]]
    nb, held, seed = 6, 2, 21
    n = (nb + held) * Bg
    rng = np.random.default_rng(8)
    F = {"X_int": rng.uniform(0, 3, (n, bot[0])).astype(np.float32),
         "X_cat": np.stack([rng.integers(0, r, n) for r in rows for _ in range(L)], 1).astype(np.int64),
         "y": rng.integers(0, 2, n).astype(np.float32)}
    order = np.concatenate([SH.epoch_order(seed, 0, nb, Bg).reshape(-1), np.arange(nb * Bg, n)])
    assert not np.array_equal(order, np.arange(n))
    F2 = {k: np.ascontiguousarray(v[order]) for k, v in F.items()}
    argv = ["--backend", HIP, "-b", str(Bg), "--arch-sparse-feature-size", str(D), "--arch-embedding-size", "-".join(map(str, rows)),
            "--embedding-bag-size", str(L), "--arch-mlp-bot", "-".join(map(str, bot)), "--arch-mlp-top", "-".join(map(str, top)),
            "--eval-batches", str(held), "--seed", str(seed), "--deterministic", "--epochs", "1"]
    res = {}
    for name, data, mode in (("total", F, "total"), ("none", F2, "none")):
        path = SH.write_hdf5(str(tmp_path / f"{name}.h5"), data)
        app = ffmodel.DLRM(argv + ["--dataset", path, "--data-randomize", mode])
        app.run_epochs()
        app.model.sync()
        res[name] = _parameters(app)
        app.close()
    assert res["total"].keys() == res["none"].keys() and len(res["total"]) >= len(rows) + 2 * (len(bot) + len(top) - 2)
    for k in res["total"]:
        assert np.array_equal(res["total"][k].view(np.uint32), res["none"][k].view(np.uint32)), k
    # ... and the run did train: F in file order ends elsewhere
    path = SH.write_hdf5(str(tmp_path / "file_order.h5"), F)
    app = ffmodel.DLRM(argv + ["--dataset", path, "--data-randomize", "none"])
    app.run_epochs()
    app.model.sync()
    other = _parameters(app)
    app.close()
    assert any(not np.array_equal(other[k], res["total"][k]) for k in other)


def test_two_ranks_sharing_the_gpu_follow_the_stripe_rule(hip, indexed, tmp_path):
    """Two ranks sharing the GPU (host-staged test transport, as tests/test_gpu_ctr_ranks.py), one epoch of `total` with --deterministic: each rank's
    labels and dense rows are its stripe in the shared order, a table's owner holds the ids of the whole global batch, and the ranks together
    train on every training sample once."""
    path, data = indexed
    world, Bl = 2, B // 2
    worker = os.path.join(ROOT, "tests", "_dist_worker_shuffle.py")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path), path, str(NB_TRAIN)] + EPOCH_ARGS, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    assert "[DLRM] data order: total (seed 5, a new order every epoch, per-rank stripes)" in outs[0]
    z = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    order = SH.epoch_order(SEED, 0, NB_TRAIN, B, world)                   # [step][row of the global batch]
    owners = 0
    for r in range(world):
        labels = z[r]["label"].astype(np.int64)                           # [step][Bl]
        assert np.array_equal(labels, order[:, r * Bl:(r + 1) * Bl]), f"rank {r}"
        assert (labels % B // Bl == r).all()                              # a sample never changes rank
        assert np.array_equal(z[r]["dense"], data["X_int"][labels])
        for t in range(len(ROWS)):
            if f"sparse{t}" in z[r].files:
                owners += 1
                assert np.array_equal(z[r][f"sparse{t}"], data["X_cat"][order, t]), f"rank {r} table {t}"
    assert owners >= len(ROWS)
    trained = np.concatenate([z[r]["label"].reshape(-1) for r in range(world)]).astype(np.int64)
    assert np.array_equal(np.sort(trained), np.arange(NB_TRAIN * B))
