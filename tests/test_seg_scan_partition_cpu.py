"""The partition of glx_seg_scan_kernel -- workgroups, tiles, load instructions, lanes -- restated in Python
(seg_scan_partition.py) and checked against a computation that knows no partition: the first violation, a searchsorted
and the three levels.  No GPU."""
import itertools

import numpy as np
import pytest

import seg_scan_partition as ssp

# (quad, wave, threads, loads, grid, run_max): sizes at which six ids cross every kind of boundary
SMALL = {
    "one lane per wave: every quad asks memory": ssp.Partition(1, 1, 1, 2, 3, 64),
    "two-id tiles, one workgroup that wraps": ssp.Partition(1, 2, 2, 1, 1, 64),
    "wave, workgroup and tile boundaries": ssp.Partition(1, 2, 4, 1, 2, 1),
    "quads of two, two loads per tile": ssp.Partition(2, 2, 2, 2, 1, 64),
    "quads of four, a wrap inside six ids": ssp.Partition(4, 2, 2, 1, 1, 1),
    "three workgroups, the last two idle or short": ssp.Partition(2, 1, 1, 1, 3, 2),
}
ALPHABET = (-1, 0, 1, 2, 3)
S = 3


def check(seg, num_segments, p):
    want_level, want_valid, want_start = ssp.plain(seg, num_segments, p.run_max)
    r = ssp.scan(seg, num_segments, p)
    assert r["counters_ok"], "the carried (i / f, i % f) left the position"
    assert r["level"] == want_level
    assert r["valid_len"] == want_valid
    n = len(seg)
    if n == 0:  # never launched: the host's floor (level 2) sends the request to the fix-up
        return
    # the id before a quad: from the lane below, except in a wave's first lane; never a load in front of position 0
    for i0, src in r["sources"].items():
        lane = (i0 % p.span) // p.quad % p.wave
        assert src == ("lane" if lane else ("memory" if i0 > 0 else "none")), (i0, src)
    assert sorted(r["sources"]) == list(range(0, n, p.quad))  # every quad that has ids is visited exactly once
    # position i writes seg_start[s] for the s in (seg[i - 1], seg[i]], the last position the segments behind seg[n - 1]
    for s, value, i0 in r["writes"]:
        assert 0 <= s <= num_segments and i0 <= value <= min(i0 + p.quad, n)
        if value < n:
            assert seg[value] >= s and (value == 0 or seg[value - 1] < s)
    if want_level < 2:  # a complete table: every entry written exactly once, by one position
        assert sorted(s for s, _, _ in r["writes"]) == list(range(num_segments + 1))
    got_level, got_valid, got_start = ssp.seg_start_after(seg, num_segments, p)
    assert got_start.tolist() == want_start.tolist()
    # a quad behind an out-of-range id writes nothing
    for s, value, i0 in r["writes"]:
        assert i0 == 0 or 0 <= seg[i0 - 1] < num_segments


@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_short_sequence(name):
    """all 19,531 sequences of at most six ids over {-1, 0, 1, 2, 3} with three segments (3 is out of range)"""
    p = SMALL[name]
    for n in range(7):
        for seg in itertools.product(ALPHABET, repeat=n):
            check(list(seg), S, p)


def test_no_ids_at_all():
    r = ssp.scan([], 3, SMALL["quads of two, two loads per tile"])
    assert r["level"] == 0 and r["writes"] == []  # the host's floor makes it level 2: the fix-up writes zeros


@pytest.mark.parametrize("grid", [1, 3, 1000])
def test_seeded_long_sequences_at_the_kernels_own_sizes(grid):
    T = ssp.kernel_partition(1).tile
    rng = np.random.default_rng(grid)
    for n in (T - 1, T + 1, 3 * T + 1, 2 * T + 3):
        p = ssp.kernel_partition(min(grid, (n + T - 1) // T))  # the launch never has more workgroups than tiles
        assert (p.span, p.tile) == (p.threads * 4, p.threads * 4 * p.loads)
        num_segments = 300
        ragged = np.sort(rng.integers(0, num_segments, n))
        check(ragged.tolist(), num_segments, p)
        gaps = np.sort(rng.choice([0, 1, 2, 70, 71, 140, 299 - 65], n))  # runs of 67, 68 and 93 empty segments; 65 behind the last id
        check(gaps.tolist(), num_segments, p)
        if n not in (T + 1, 3 * T + 1):
            continue
        for at in (0, 255, 256, p.span - 1, p.span, T - 1, T, n - 1):
            for what in ("decrease", "negative", "too large"):
                bad = ragged.copy()
                bad[at] = {"decrease": bad[at - 1] - 1 if at else -1, "negative": -1, "too large": num_segments}[what]
                if what == "decrease" and at and bad[at] < 0:
                    continue
                check(bad.tolist(), num_segments, p)
    # the dense layout spelled out, and one adjacent pair swapped across a segment border
    for f in (1, 3, 10):
        num_segments = (2 * T + f - 1) // f
        p = ssp.kernel_partition(min(grid, (num_segments * f + T - 1) // T))
        dense = np.arange(num_segments * f) // f
        check(dense.tolist(), num_segments, p)
        r = ssp.scan(dense.tolist(), num_segments, p)
        assert r["level"] == 0
        if f > 1:
            for border in (f, (T // f) * f, (p.span // f + 1) * f):
                moved = dense.copy()
                moved[border - 1] = moved[border]  # one id moves to its neighbour segment: still non-decreasing
                check(moved.tolist(), num_segments, p)
                assert ssp.scan(moved.tolist(), num_segments, p)["level"] == 1
