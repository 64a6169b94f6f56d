"""The compact EdgeWeight record layout and its selection rule (tests/ew_compact_layout.py restates
csrc/glx_common.h glx_ew20_offset / glx_ew20_table_bytes / glx_ew_record_bytes_rule).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ew_compact_layout as lay  # noqa: E402

I32MAX, I32MIN = 2 ** 31 - 1, -2 ** 31
WINDOWS = [(0, 200000), (2 ** 31 - 1 - 3000, 2 ** 31 - 1 + 3000)]


@pytest.mark.parametrize("lo,hi", WINDOWS, ids=["from_zero", "around_2_31"])
def test_records_are_aligned_disjoint_and_inside_one_sector(lo, hi):
    g = np.arange(lo, hi, dtype=np.uint64)
    off = (g // np.uint64(3)) * np.uint64(64) + (g % np.uint64(3)) * np.uint64(20)
    assert [lay.offset(int(x)) for x in g[:9]] == [int(x) for x in off[:9]]  # the vector form is the scalar one
    assert lay.offset(int(g[-1])) == int(off[-1])
    assert (off % np.uint64(4) == 0).all()
    assert (off[1:] >= off[:-1] + np.uint64(20)).all()  # ascending and no two records overlap
    assert (off // np.uint64(64) == (off + np.uint64(19)) // np.uint64(64)).all()  # none crosses a 64-byte boundary
    assert (off % np.uint64(64) <= np.uint64(40)).all()  # the last 4 bytes of every sector stay unused


def test_offsets_at_the_start_are_the_ones_written_out():
    assert [lay.offset(g) for g in range(7)] == [0, 20, 40, 64, 84, 104, 128]


@pytest.mark.parametrize("E", [1, 2, 3, 4, 5, 6, 97, 98, 99, 375, 376, 377, 10 ** 8, 10 ** 8 + 1, 10 ** 8 + 2,
                               2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31])
def test_last_record_ends_inside_the_table(E):
    assert lay.offset(E - 1) + 20 <= lay.table_bytes(E)
    assert lay.table_bytes(E) % 64 == 0
    assert lay.table_bytes(E) - lay.offset(E - 1) <= 64  # and the table holds no sector without a record
    assert {e % 3 for e in (1, 2, 3, 97, 98, 99, 10 ** 8, 10 ** 8 + 1, 10 ** 8 + 2)} == {0, 1, 2}


def test_offsets_beyond_32_bits_are_exact():
    # 10^8 slots end 14 MB short of 2^31 bytes, which slot 100,663,296 passes; 2^32 bytes is passed from slot 201,326,592
    assert lay.offset(10 ** 8 - 1) == 2133333312 and lay.table_bytes(10 ** 8) == 2133333376 < 2 ** 31
    assert lay.offset(100663296 - 1) == 2 ** 31 - 64 + 40 and lay.offset(100663296) == 2 ** 31
    g = 201326592
    assert lay.offset(g - 1) == 2 ** 32 - 64 + 40 and lay.offset(g) == 2 ** 32
    assert lay.offset(2 ** 31 - 1) == 715827882 * 64 + 20 == 45812984468
    assert lay.table_bytes(2 ** 31) == 715827883 * 64
    for g in (2 ** 31 - 1, 2 ** 31, 2 ** 32 + 1, 3 * 2 ** 40 + 2):
        q, r = divmod(g, 3)
        assert lay.offset(g) == q * 64 + r * 20


# (eid_min, eid_max, nbr_min, nbr_max, E, env) -> bytes per record
RULE_CASES = [
    ((0, 99, 0, 9, 100, None), 20),
    ((0, 99, 0, 9, 100, ""), 20),
    ((0, 99, 0, 9, 100, "1"), 20),
    ((0, 99, 0, 9, 100, "20"), 20),
    ((0, 99, 0, 9, 100, "32"), 32),
    ((0, 99, 0, 9, 100, "0"), 0),
    ((I32MIN, I32MAX, I32MIN, I32MAX, 100, None), 20),  # negative ids are legal and stay signed
    ((I32MIN, I32MAX, I32MIN, I32MAX, 100, "32"), 32),
    ((0, 99, 0, I32MAX + 1, 100, None), 32),  # one neighbour id of 2^31
    ((0, 99, I32MIN - 1, 9, 100, None), 32),
    ((0, 99, 0, 2 ** 40, 100, "32"), 32),
    ((0, 99, 0, 2 ** 40, 100, "0"), 0),
    ((0, I32MAX + 1, 0, 9, 100, None), 0),  # one edge id beyond int32: neither table
    ((I32MIN - 1, 99, 0, 9, 100, None), 0),
    ((0, I32MAX + 1, 0, 9, 100, "32"), 0),
    ((0, I32MAX + 1, 0, 2 ** 40, 100, None), 0),
    ((0, 99, 0, 9, 2 ** 31, None), 20),  # slot indices up to 2^31 - 1
    ((0, 99, 0, 9, 2 ** 31 + 1, None), 32),
    ((0, 99, 0, 9, 2 ** 31 + 1, "0"), 0),
    ((0, 0, 0, 0, 0, None), 0),  # no edges, no records
    ((0, 0, 0, 0, 0, "32"), 0),
]


@pytest.mark.parametrize("args,want", RULE_CASES)
def test_selection_rule(args, want):
    assert lay.record_bytes(*args) == want
