"""The inputs of tests/test_gpu_fold_sum.py on numpy alone: they hold every case the wide-row segmented sum (csrc/fold_sum.hip) treats differently -- runs
inside a 32-block, runs across 32-blocks, a run across two 1024-block boundaries, rows that are not hit in front of, between and behind hit ones, the
ragged tail -- and the canonical fp32 order itself meets the project's bound against float64 on them."""
import numpy as np
import pytest

import fold_helpers as FH
import fold_sum_helpers as SH

CASES = [(bag, kind) for bag in SH.SHAPES for kind in SH.KINDS]


def all_runs():
    for bag, kind in CASES:
        _, ids = SH.inputs(bag, kind)
        for t, r in enumerate(SH.ROWS):
            s = SH.sorted_ids(ids[t])
            yield bag, kind, r, s, SH.runs(s)


def test_shape_of_the_list():
    for bag, kind, r, s, _ in all_runs():
        assert len(s) == SH.N == SH.SHAPES[bag] * bag
    assert -(-SH.N // 1024) == 3 and SH.N % 1024 != 0, "three 1024-blocks, the last one ragged"
    assert SH.N % 32 == 4, "the last 32-block holds 4 entries"


def test_runs_inside_and_across_blocks():
    inside32 = across32 = across1024_twice = 0
    for bag, kind, r, s, rr in all_runs():
        for row, i, j in rr:
            if i // 32 == j // 32 and j > i:
                inside32 += 1
            if i // 32 != j // 32 and i // 1024 == j // 1024:
                across32 += 1
            if j // 1024 - i // 1024 >= 2:
                across1024_twice += 1
    assert inside32 and across32 and across1024_twice
    # the table of one row is one run over the whole list in every case
    for bag, kind, r, s, rr in all_runs():
        if r == 1:
            assert rr == [(0, 0, SH.N - 1)]


def test_open_partials_of_every_kind():
    """A 32-block entered from the left and left to the right by different rows, and one a single row passes through."""
    two_open = through = first_of_1024_open = 0
    for bag, kind, r, s, rr in all_runs():
        for b in range(32, len(s) - 32, 32):
            enters, leaves = s[b - 1] == s[b], s[b + 31] == s[b + 32]
            if enters and leaves and s[b] != s[b + 31] and b % 1024 and (b + 32) % 1024:
                two_open += 1
            if enters and leaves and s[b] == s[b + 31]:
                through += 1
        for b in range(1024, len(s), 1024):
            if s[b - 1] == s[b]:
                first_of_1024_open += 1
    assert two_open and through and first_of_1024_open


def test_rows_not_hit():
    between = front = behind = 0
    for bag, kind, r, s, rr in all_runs():
        hit = np.zeros(r, bool)
        hit[s] = True
        if r > 1 and not hit[0]:
            front += 1
        if r > 1 and not hit[-1]:
            behind += 1
        h = np.flatnonzero(hit)
        if len(h) >= 2 and np.any(np.diff(h) > 1):
            between += 1
    assert between and front and behind


@pytest.mark.parametrize("bag,kind", CASES)
def test_canonical_order_meets_the_bound(bag, kind):
    for t, r in enumerate(SH.ROWS):
        can, ref, mass = SH.references(bag, kind)[t]
        FH.assert_within(can, ref, mass, f"canonical fp32 order, {r} rows, bag {bag}, ids {kind}")
        dy, ids = SH.inputs(bag, kind)
        hit = np.zeros(r, bool)
        hit[ids[t].reshape(-1)] = True
        assert not can[~hit].any()
