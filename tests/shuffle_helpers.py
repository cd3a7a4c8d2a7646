"""Shared by the shuffle tests (--data-randomize total): a numpy restatement of include/ffh_perm.h -- the counter hash of
include/ffh_rng.h, the cycle-walked Feistel network, the stripe rule -- and the small data sets the tests train on.  Nothing here calls
the code under test."""
import numpy as np

U = np.uint64
SEED_XOR = 0x53485546464C4531          # FFH_PERM_SEED_XOR


def _mix64(z):
    with np.errstate(over="ignore"):
        z = z + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def ffh_hash(seed, i):
    """ffh_hash(seed, i) on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        return _mix64(_mix64(np.atleast_1d(np.asarray(seed, U))) + np.atleast_1d(np.asarray(i, U)))


def perm(seed, epoch, n, positions=None):
    """ffh_perm_index(seed, epoch, i, n) for every i of `positions` (default: all of [0, n)) as int64."""
    pos = np.arange(max(n, 1), dtype=U) if positions is None else np.asarray(positions, U)
    if n <= 1:
        return np.zeros(pos.shape, np.int64)
    w = 1
    while (1 << (2 * w)) < n:
        w += 1
    mask = U((1 << w) - 1)
    keys = [ffh_hash((seed ^ SEED_XOR) & (2**64 - 1), 4 * epoch + r)[0] for r in range(4)]
    x = pos.copy()
    walking = np.ones(x.shape, bool)                  # every position takes at least one step
    while walking.any():
        xs = x[walking]
        left, right = xs >> U(w), xs & mask
        for k in keys:
            left, right = right, left ^ (ffh_hash(k, right) & mask)
        x[walking] = (left << U(w)) | right
        walking &= x >= U(n)
    return x.astype(np.int64)


def global_sample(p, Bl, world, rank):
    """ffh_perm_global_sample: the sample whose ids go with row p of rank `rank`'s stripe."""
    p = np.asarray(p, np.int64)
    return (p // Bl) * (Bl * world) + rank * Bl + p % Bl


def epoch_order(seed, epoch, nb, B, world=1):
    """Global sample index of every row of every training batch of one epoch: [nb][B] (row r * Bl + i of a batch belongs to rank r)."""
    Bl = B // world
    p = perm(seed, epoch, nb * Bl).reshape(nb, Bl)
    return np.concatenate([global_sample(p, Bl, world, r) for r in range(world)], axis=1)


def indexed_dataset(n, rows, dense=13, seed=11):
    """A data set whose label is the sample index (exact in fp32 below 2^24) and whose other columns are random: X_int float32 [n][dense],
    X_cat int64 [n][tables], y float32 [n]."""
    rng = np.random.default_rng(seed)
    return {"X_int": rng.uniform(0.0, 4.0, (n, dense)).astype(np.float32),
            "X_cat": np.stack([rng.integers(0, r, n) for r in rows], 1).astype(np.int64),
            "y": np.arange(n, dtype=np.float32)}


def write_hdf5(path, data):
    from dlrm_flexflow_amd import hdf5_lite
    hdf5_lite.write(path, data)
    return path
