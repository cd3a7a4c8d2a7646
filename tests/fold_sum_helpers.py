"""Shared by the tests of the wide-row segmented sum behind ffh_fold_segment_sum (csrc/fold_sum.hip): the seeded inputs and their references, computed
once per (bag, id kind) at the full width -- a narrower call reads the leading columns of the same dy, and the sum of a column does not depend on its
neighbours, so its reference is a column slice."""
import functools

import numpy as np

import fold_helpers as FH
import fold_dw_helpers as DH

ROWS = DH.ROWS                   # 1, 3, 300 and 5000 rows in one call
KINDS = DH.KINDS                 # random, equal, last
N = 2500                         # lookups per table: three 1024-blocks, the last one ragged, its last 32-block holds 4 entries
SHAPES = {1: 2500, 2: 1250}      # bag -> batch
WIDTH = 1024                     # the widest call; 256 and 192 read its leading columns
LD = WIDTH + 8                   # floats between rows of dy


@functools.lru_cache(maxsize=None)
def inputs(bag, kind):
    """dy [batch][LD] (the pad columns hold a large value that no sum may pick up) and the ids of the four tables [batch][bag]."""
    batch = SHAPES[bag]
    rng = np.random.default_rng(7000 + 10 * bag + KINDS.index(kind))
    dy = np.full((batch, LD), 1e30, np.float32)
    dy[:, :WIDTH] = rng.uniform(-1, 1, (batch, WIDTH)).astype(np.float32)
    ids = [FH.make_ids(rng, kind, batch, bag, r) for r in ROWS]
    for a in [dy] + ids:
        a.setflags(write=False)
    return dy, ids


@functools.lru_cache(maxsize=None)
def references(bag, kind):
    """Per table: (canonical fp32 sum, float64 sum, float64 term mass), all [rows][WIDTH]."""
    dy, ids = inputs(bag, kind)
    out = []
    for t, r in enumerate(ROWS):
        can = DH.segment_sum_canonical_f32(ids[t], dy[:, :WIDTH], r)
        ref, mass = DH.segment_sum_f64(ids[t], dy[:, :WIDTH], r)
        for a in (can, ref, mass):
            a.setflags(write=False)
        out.append((can, ref, mass))
    return out


def sorted_ids(ids):
    """The row ids in the order of the sorted (row, position) list."""
    return np.sort(ids.reshape(-1), kind="stable")


def runs(s):
    """(row, first index, last index) of every run of the sorted list."""
    cut = np.flatnonzero(np.diff(s)) + 1
    a = np.concatenate([[0], cut])
    b = np.concatenate([cut, [len(s)]]) - 1
    return [(int(s[i]), int(i), int(j)) for i, j in zip(a, b)]
