"""scripts/l2_stripe_sim.cc (the per-XCD L2 model behind the XCD-stripe mapping of the grouped reduce) on streams whose
line fetches can be counted by hand.  D = 32 floats -> one 128-byte line per row, 8-lane groups, 32 segments per
workgroup; fanout 1 -> one 8-byte id per segment, 16 segments' ids per line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import l2_stripe_sim  # noqa: E402


def _fetched(out):
    rows = [ln.split() for ln in out.splitlines() if not ln.startswith("#")]
    return {r[0]: (int(r[1]), int(r[2])) for r in rows}


def test_one_row_read_by_two_workgroups():
    # 64 segments = 2 workgroups -> XCDs 0 and 1: row 0 is fetched into both L2s, each XCD fetches its 2 id lines
    got = _fetched(l2_stripe_sim.run(np.zeros(64, np.int32), ["rr:1"], 1, 32, 100))
    assert got["rr:1"] == (2 + 4, 64 + 64)


def test_stripes_keep_neighbouring_blocks_on_one_xcd():
    # 16 workgroups; blocks 2k and 2k + 1 read the same row k.  Round robin puts them on two XCDs (16 row fetches),
    # stripes of 2 blocks put both on XCD k (8).  The 32 id lines are fetched once either way.
    ids = (np.arange(16 * 32) // 64).astype(np.int32)
    got = _fetched(l2_stripe_sim.run(ids, ["rr:1", "stripe:1:2"], 1, 32, 100))
    assert got["rr:1"] == (16 + 32, 512 + 512)
    assert got["stripe:1:2"] == (8 + 32, 512 + 512)


def test_unknown_ids_read_row_zero_and_a_permutation_is_applied():
    ids = np.full(64, -1, np.int32)
    ids[32:] = 5
    got = _fetched(l2_stripe_sim.run(ids, ["rr:1"], 1, 32, 100))
    assert got["rr:1"] == (2 + 4, 128)
    # reversed segment order: the same two rows, the same id lines
    order = np.arange(64)[::-1].copy()
    got = _fetched(l2_stripe_sim.run(ids, ["perm:1:@ORDER"], 1, 32, 100, order=order))
    assert got["perm:1"] == (2 + 4, 128)
