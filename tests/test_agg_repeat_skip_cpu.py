"""The property the grouped reduce relies on when it does not load a row its segment has already folded
(glx_aggregate.hip agg_first_occurrences): Max folds with (l < r) ? r : l from -37 and Min with (r < l) ? r : l from
FLT_MAX, so folding only the FIRST occurrence of every row, in the same order, gives the same bits as folding every
position -- NaN, +-inf, +-0, subnormals and values at or below the start value included.  numpy float32, compared bit
for bit: every index sequence of length 1-5 with a repeat over thirteen values, and random long sequences over three
rows, whole and in the 64-position pieces the kernel works in."""
import itertools

import numpy as np
import pytest

F32 = np.finfo(np.float32)
VALUES = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -37.0, -38.0, -36.5, 1.0, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)
INIT = {"max": np.float32(-37.0), "min": F32.max}


def fold(op, x, take):
    """Left-to-right select fold of x[N, L(, D)] over axis 1; take[N, L] = the positions that are folded at all."""
    acc = np.full(x.shape[:1] + x.shape[2:], INIT[op], np.float32)
    with np.errstate(invalid="ignore"):
        for j in range(x.shape[1]):
            r = x[:, j]
            sel = (acc < r) if op == "max" else (r < acc)
            t = take[:, j].reshape((-1,) + (1,) * (r.ndim - 1))
            acc = np.where(sel & t, r, acc)
    return acc


def first_occurrences(seq, piece=None):
    """first[N, L]: position j holds a row that no earlier position (of the same piece of `piece` positions) holds."""
    n, length = seq.shape
    first = np.ones((n, length), bool)
    for j in range(length):
        lo = 0 if piece is None else (j // piece) * piece
        for i in range(lo, j):
            first[:, j] &= seq[:, i] != seq[:, j]
    return first


def beq(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("op", ["max", "min"])
def test_every_short_sequence_with_a_repeat(op):
    assert VALUES.size == 13 and np.isnan(VALUES[0]) and np.signbit(VALUES[4]) and VALUES[9] > 0 and VALUES[10] < 0
    cases = 0
    for length in range(1, 6):
        seq = np.array(list(itertools.product(range(13), repeat=length)), np.int32)
        first = first_occurrences(seq)
        rep = ~first.all(axis=1)
        seq, first = seq[rep], first[rep]
        cases += seq.shape[0]
        if seq.shape[0] == 0:
            continue
        x = VALUES[seq]
        assert beq(fold(op, x, first), fold(op, x, np.ones_like(first))), length
    assert cases == 228748  # 13^L sequences less the repeat-free ones, L = 1..5


@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("length", [25, 130])
def test_random_sequences_over_three_rows(op, length):
    rng = np.random.default_rng(length)
    n, d = 400, 16
    rows = rng.standard_normal((n, 3, d)).astype(np.float32) * 30
    special = rng.random((n, 3, d)) < 0.4
    rows[special] = VALUES[rng.integers(0, 13, int(special.sum()))]
    seq = rng.integers(0, 3, (n, length)).astype(np.int32)
    x = rows[np.arange(n)[:, None], seq]
    every = fold(op, x, np.ones(seq.shape, bool))
    assert beq(fold(op, x, first_occurrences(seq)), every)
    assert beq(fold(op, x, first_occurrences(seq, piece=64)), every)  # a repeat across two pieces is folded again
    assert (first_occurrences(seq).sum(axis=1) <= 3).all()
