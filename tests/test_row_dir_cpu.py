"""The samplers' row directory: which form a graph keeps, the two entry layouts, the absent sentinel and hashed16
probing (tests/row_dir_layout.py restates csrc/glx_common.h glx_row_dir_form_rule / GlxRowDirEntry / GlxRowDirSlot /
glx_row_span and glx_idmap_build's capacity).  No GPU; tests/test_gpu_row_dir.py asks the library itself for the form
at the same boundaries."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import row_dir_layout as lay  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "graph-learn_amd", "csrc")
I64MAX, I64MIN = 2 ** 63 - 1, -2 ** 63


def header():
    with open(os.path.join(CSRC, "glx_common.h")) as fh:
        return fh.read()


def test_constants_are_the_header_s():
    text = header()
    assert "enum { GLX_ROW_DIR_NONE = 0, GLX_ROW_DIR_DIRECT = 1, GLX_ROW_DIR_HASHED16 = 2 };" in text
    assert "#define GLX_ROW_DIR_ABSENT 0xffffffffu" in text and lay.ABSENT == 0xffffffff
    assert "#define GLX_EMPTY_KEY INT64_MIN" in text and lay.EMPTY_KEY == I64MIN
    assert "sizeof(GlxRowDirEntry) == 8 && sizeof(GlxRowDirSlot) == 16" in text
    assert re.search(r"struct GlxRowDirEntry \{\s*uint32_t start, deg;\s*\};", text)
    assert re.search(r"struct alignas\(16\) GlxRowDirSlot \{\s*int64_t key;\s*uint32_t start, deg;\s*\};", text)
    # the rule's three decisions, as written
    assert ("constexpr bool kRowDirDefaultOn = %s;" % ("true" if lay.DEFAULT_ON else "false")) in text
    assert "(env ? env[0] == '0' : !kRowDirDefaultOn)" in text
    assert "if (num_edges >= (int64_t)0xffffffffll) return GLX_ROW_DIR_NONE;" in text and lay.E_LIMIT == 0xffffffff
    assert 'strcmp(env, "hash") == 0' in text
    assert "min_id >= 0 && (uint64_t)max_id < cap * 2u) return GLX_ROW_DIR_DIRECT;" in text
    # and the hash is glx_mix64's
    assert "x *= 0xff51afd7ed558ccdULL;" in text and "x *= 0xc4ceb9fe1a85ec53ULL;" in text


def test_entry_layouts():
    assert lay.ENTRY.itemsize == 8 and lay.ENTRY.fields["start"][1] == 0 and lay.ENTRY.fields["deg"][1] == 4
    assert lay.SLOT.itemsize == 16
    assert [lay.SLOT.fields[n][1] for n in ("key", "start", "deg")] == [0, 8, 12]
    # one 8-byte word of an entry: start in the low half, degree in the high half (little endian)
    e = np.array([(7, 3)], lay.ENTRY)
    assert int(e.view("<u8")[0]) == (3 << 32) | 7
    s = np.array([(-5, 7, 3)], lay.SLOT)
    assert s.view("<u4").tolist() == [0xfffffffb, 0xffffffff, 7, 3]


def test_capacity_is_the_id_map_s():
    assert [lay.capacity(n) for n in (0, 1, 32, 33, 64, 65, 10 ** 7)] == [64, 64, 64, 128, 128, 256, 2 ** 25]


@pytest.mark.parametrize("rows", [1, 7, 32, 33, 5000, 10 ** 7])
def test_form_rule_at_its_boundary(rows):
    cap = lay.capacity(rows)
    edge = 2 * cap - 1  # (max_id + 1) * 8 == cap * 16
    assert (edge + 1) * 8 == cap * 16
    assert lay.form(rows, 100, 0, edge, cap, "1") == lay.DIRECT
    assert lay.form(rows, 100, 0, edge + 1, cap, "1") == lay.HASHED16
    assert lay.form(rows, 100, 0, edge - 1, cap, "1") == lay.DIRECT
    assert lay.table_bytes(lay.DIRECT, edge, cap) == lay.table_bytes(lay.HASHED16, edge, cap)  # never the larger one
    assert lay.form(rows, 100, edge, edge, cap, "1") == lay.DIRECT  # only the largest id counts
    assert lay.form(rows, 100, 0, I64MAX, cap, "1") == lay.HASHED16


def test_negative_smallest_id_forces_hashed16():
    assert lay.form(4, 100, -1, 10, 64, "1") == lay.HASHED16
    assert lay.form(4, 100, I64MIN + 1, I64MAX, 64, "1") == lay.HASHED16
    assert lay.form(4, 100, 0, 10, 64, "1") == lay.DIRECT


def test_knob_values():
    for env, want in ((None, lay.DIRECT if lay.DEFAULT_ON else lay.NONE), ("", lay.DIRECT), ("1", lay.DIRECT), ("direct", lay.DIRECT), ("hash", lay.HASHED16),
                      ("0", lay.NONE)):
        assert lay.form(7, 100, 0, 100, 64, env) == want, env
    for env, want in ((None, lay.HASHED16 if lay.DEFAULT_ON else lay.NONE), ("1", lay.HASHED16), ("hash", lay.HASHED16), ("0", lay.NONE)):
        assert lay.form(7, 100, 0, 1000, 64, env) == want, env  # nothing forces the direct form past its bound


def test_edge_count_limit_by_numbers():
    cap = lay.capacity(10 ** 9)
    for env in ("hash", "1"):
        assert lay.form(10 ** 9, 2 ** 32 - 2, 0, 10 ** 9, cap, env) != lay.NONE
        assert lay.form(10 ** 9, 2 ** 32 - 1, 0, 10 ** 9, cap, env) == lay.NONE  # start = 2^32 - 1 would be the sentinel
        assert lay.form(10 ** 9, 2 ** 40, 0, 10 ** 9, cap, env) == lay.NONE
    assert lay.form(0, 0, 0, 0, 64) == lay.NONE  # no rows, no directory
    assert lay.form(3, 0, 0, 2, 64, "1") == lay.DIRECT  # rows without edges (CSR-built) keep one


def test_direct_table_tells_absent_from_empty():
    ids, start, deg = [0, 3, 4, 9], [0, 4, 4, 9], [4, 0, 5, 2]  # id 3 is a KNOWN row of degree 0
    t = lay.build_direct(ids, start, deg)
    assert t.shape[0] == 10 and t.nbytes == 80
    assert lay.lookup(t, lay.DIRECT, 3)[:3] == (True, 4, 0)
    assert lay.lookup(t, lay.DIRECT, 9)[:3] == (True, 9, 2)
    for unknown in (1, 2, 5, 8, 10, 11, -1, I64MIN, I64MAX):
        assert lay.lookup(t, lay.DIRECT, unknown)[:3] == (False, 0, 0), unknown
    assert (t["start"][[1, 2, 5, 6, 7, 8]] == lay.ABSENT).all()
    assert lay.lookup(t, lay.DIRECT, 10)[3] == 0 and lay.lookup(t, lay.DIRECT, -1)[3] == 0  # out of range: no load at all


def test_mix64_known_values():
    # fmix64 of MurmurHash3 (public domain): 0 is a fixed point; the others were computed with 64-bit integer steps
    assert lay.mix64(0) == 0
    x = 1
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) % 2 ** 64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) % 2 ** 64
    x ^= x >> 33
    assert lay.mix64(1) == x == 0xb456bcfc34c2cb2c
    assert lay.mix64(-1) == lay.mix64(2 ** 64 - 1)  # negative ids hash by their two's-complement bits
    assert lay.mix64(I64MIN) == lay.mix64(2 ** 63)


def test_hashed16_probing_wraps_and_stops_at_a_free_slot():
    cap = 64
    a, b, c, d = lay.colliding_ids(cap, cap - 1, 4, first=128)
    assert {lay.home_slot(x, cap) for x in (a, b, c, d)} == {cap - 1}
    others = [x for x in (-5, 7, 2 ** 40, I64MAX - 1) if lay.home_slot(x, cap) not in (cap - 1, 0, 1, 2)]
    ids = [a, b, c] + others
    start = list(range(10, 10 + len(ids)))
    deg = [3, 0, 5] + [1] * len(others)
    t = lay.build_hashed16(ids, start, deg, cap)
    assert t.nbytes == cap * 16
    assert [int(t["key"][h]) for h in (cap - 1, 0, 1)] == [a, b, c] and int(t["key"][2]) == lay.EMPTY_KEY
    assert lay.lookup(t, lay.HASHED16, a) == (True, 10, 3, 1)
    assert lay.lookup(t, lay.HASHED16, b) == (True, 11, 0, 2)  # wrapped to slot 0; a known row of degree 0
    assert lay.lookup(t, lay.HASHED16, c) == (True, 12, 5, 3)
    assert lay.lookup(t, lay.HASHED16, d) == (False, 0, 0, 4)  # same home slot, walks 63, 0, 1 and stops at the free 2
    assert lay.lookup(t, lay.HASHED16, lay.EMPTY_KEY) == (False, 0, 0, 0)  # the reserved key never probes
    for i, x in enumerate(others):
        assert lay.lookup(t, lay.HASHED16, x)[:3] == (True, 13 + i, 1)
    # every lookup agrees with a dict, whatever order the table was filled in
    rng = np.random.default_rng(5)
    ids = [int(x) for x in rng.integers(-2 ** 62, 2 ** 62, 30)] + [a, b, c]
    want = {x: (i, i % 4) for i, x in enumerate(ids)}
    for order in (ids, ids[::-1]):
        t = lay.build_hashed16(order, [want[x][0] for x in order], [want[x][1] for x in order], cap)
        for x in ids + [d, 0, -1, I64MAX]:
            got = lay.lookup(t, lay.HASHED16, x)[:3]
            assert got == ((True,) + want[x] if x in want else (False, 0, 0)), x
