"""The chunked order of the row gradients without a GPU: the numpy restatement
(agg_chunked_ref.py) against the two contracts it sits between -- the ascending-position order for lists of at most
one chunk, glx_rows_coalesce's order for Sum -- the proof that the two orders CAN be told apart, and the two new entry
points: declared, exported, listed, and refusing a float16 grad_x before they touch a device."""
import ctypes
import os

import numpy as np
import pytest

import agg_backward_ref as ref
import agg_chunked_ref as cref
import agg_weighted_ref as wref
import embedding_ref as eref
import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 3
NEW = ["glx_aggregate_backward_chunked", "glx_aggregate_weighted_backward_x_chunked"]
OPS = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}


def _short_request(op, seed=0, dim=6):
    """600 positions over 12 rows, no list beyond 256 entries (the longest has exactly 256); ids -1 and num_rows; a
    ragged layout with an unconsumed tail"""
    rng = np.random.default_rng(seed)
    num_rows = 12
    pool = np.array([r for r in range(num_rows) if r != 5], np.int64)
    rows = np.concatenate([np.full(256, 5, np.int64), rng.choice(pool, 344)])
    rows[300:302] = (-1, num_rows)
    rng.shuffle(rows)
    cnt = np.array([0, 100, 7, 0, 250, 1, 200, 22], np.int32)  # sums to 580: 20 positions are never consumed
    S = len(cnt)
    arg = None
    if op in (ref.MAX, ref.MIN):
        grad_out = rng.integers(-3, 4, (S, dim)).astype(np.float32)
        X = rng.integers(-2, 3, (num_rows, dim)).astype(np.float32)
        arg = ref.fold_arg(op, X, rows, ref.segment_starts(cnt, len(rows), S))[1]
    else:
        grad_out = rng.standard_normal((S, dim)).astype(np.float32)
    return rows, cnt, grad_out, num_rows, arg


@pytest.mark.parametrize("op", sorted(OPS))
def test_lists_of_at_most_one_chunk_get_the_ascending_order(op):
    rows, cnt, grad_out, num_rows, arg = _short_request(OPS[op])
    lengths = cref.list_lengths(rows, cnt, len(cnt), num_rows)
    assert lengths.max() <= cref.CHUNK and lengths[5] >= 200
    got = cref.backward(OPS[op], rows, cnt, grad_out, num_rows, arg)
    assert ref.same_bits(got, ref.backward(OPS[op], rows, cnt, grad_out, num_rows, arg))


@pytest.mark.parametrize("op", ["sum", "mean"])
def test_weighted_lists_of_at_most_one_chunk_get_the_ascending_order(op):
    rows, cnt, grad_out, num_rows, _ = _short_request(OPS[op])
    w = np.random.default_rng(3).standard_normal((len(rows), 2)).astype(np.float32)
    got = cref.backward_weighted_x(OPS[op], rows, w, cnt, grad_out, num_rows)
    assert wref.same_bits(got, wref.backward_x(OPS[op], rows, w, cnt, grad_out, num_rows))


def _hub_request(seed=1, dim=5):
    """one position per segment; row 2 is named 700 times, row 4 exactly 257 times, row 0 by nobody"""
    rng = np.random.default_rng(seed)
    num_rows = 7
    rows = np.concatenate([np.full(700, 2, np.int64), np.full(257, 4, np.int64), rng.choice([1, 3, 5, 6, -1, 7], 200)])
    rng.shuffle(rows)
    return rows, rng.standard_normal((len(rows), dim)).astype(np.float32), num_rows


def test_sum_is_the_coalesce_of_the_gathered_rows():
    rows, grad_out, num_rows = _hub_request()
    got = cref.backward(ref.SUM, rows, None, grad_out, num_rows)
    urows, ug, U = eref.coalesce(rows, grad_out, num_rows)  # one position per segment: g[p] = grad_out[p]
    want = np.zeros_like(got)
    want[urows[:U]] = ug[:U]
    assert ref.same_bits(got, want)
    assert not got[0].view(np.uint32).any()
    # a ragged layout: g[p] = grad_out[segment(p)] over the consumed positions
    cnt = np.array([400, 0, 300, 57, 300], np.int32)  # 1057 of 1157 positions
    go = np.random.default_rng(2).standard_normal((len(cnt), 5)).astype(np.float32)
    seg = np.repeat(np.arange(len(cnt)), cnt)
    got = cref.backward(ref.SUM, rows, cnt, go, num_rows)
    urows, ug, U = eref.coalesce(rows[:len(seg)], go[seg], num_rows)
    want = np.zeros_like(got)
    want[urows[:U]] = ug[:U]
    assert ref.same_bits(got, want)


def test_the_two_orders_can_be_told_apart():
    """700 random-normal terms: the chunked sum (256 + 256 + 188) and the ascending sum differ in at least one bit"""
    rows, grad_out, num_rows = _hub_request()
    chunked = cref.backward(ref.SUM, rows, None, grad_out, num_rows)
    plain = ref.backward(ref.SUM, rows, None, grad_out, num_rows)
    assert (chunked[2].view(np.uint32) != plain[2].view(np.uint32)).any()
    short = [1, 3, 5, 6, 0]
    assert ref.same_bits(chunked[short], plain[short])
    w = np.random.default_rng(4).standard_normal((len(rows), 1)).astype(np.float32)
    chunked = cref.backward_weighted_x(wref.SUM, rows, w, None, grad_out, num_rows)
    plain = wref.backward_x(wref.SUM, rows, w, None, grad_out, num_rows)
    assert (chunked[2].view(np.uint32) != plain[2].view(np.uint32)).any()
    assert wref.same_bits(chunked[short], plain[short])


def test_chunk_boundaries_count_entries_not_selected_terms():
    """Max over one row named 600 times by segments of one position each, arg selecting only the entries from the 300th
    on: the second chunk starts at entry 256, so the terms split 44 + 256, not 256 + 44"""
    n, dim = 600, 3
    rows = np.zeros(n, np.int64)
    grad_out = np.random.default_rng(6).standard_normal((n, dim)).astype(np.float32)
    arg = np.full((n, dim), -1, np.int32)
    arg[300:] = np.arange(300, n, dtype=np.int32)[:, None]
    got = cref.backward(ref.MAX, rows, None, grad_out, 1, arg)
    with np.errstate(all="ignore"):
        parts = []
        for a, b in ((300, 512), (512, 600)):
            acc = np.zeros(dim, np.float32)
            for p in range(a, b):
                acc = (acc + grad_out[p]).astype(np.float32)
            parts.append(acc)
        want = ((np.zeros(dim, np.float32) + np.zeros(dim, np.float32)) + parts[0]).astype(np.float32)
        want = (want + parts[1]).astype(np.float32)
    assert ref.same_bits(got[0], want)


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_exported_and_listed(name):
    header = open(os.path.join(ROOT, "include", "glx.h")).read()
    assert "GLX_API int {}(".format(name) in header
    assert name in glx.EXPORTS
    assert hasattr(ctypes.CDLL(glx.LIB_PATH), name)


def _call(name, dt):
    """a well-formed one-row request with host pointers, but for the dtype id"""
    L = glx.lib()
    rows = np.zeros(1, np.int64)
    f4 = np.zeros(4, np.float32)
    tab = np.zeros(4, np.float32)
    w = np.ones(1, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    if name == "glx_aggregate_backward_chunked":
        return L.glx_aggregate_backward_chunked(0, glx.SUM, p(rows), None, None, 1, 1, 1, 4, p(f4), p(tab), dt,
                                                glx.PTR_HOST, None)
    return L.glx_aggregate_weighted_backward_x_chunked(0, glx.SUM, p(rows), p(w), 1, None, 1, 1, 1, 4, p(f4), p(tab), dt,
                                                       glx.PTR_HOST, None)


@pytest.mark.parametrize("name", NEW)
def test_a_float16_grad_x_is_refused_before_any_device_use(name):
    dt = glx.FEATURE_DTYPES["float16"]
    assert _call(name, dt) == INVALID_ARGUMENT
    msg = glx.lib().glx_last_error().decode()
    assert name in msg and "bfloat16" in msg and str(dt) in msg, msg


def test_wrappers_take_the_flag():
    """the flag is a keyword of both wrappers; a bad output dtype is still refused before the call"""
    rows = np.zeros(1, np.int64)
    g = np.zeros((1, 4), np.float32)
    with pytest.raises(ValueError):
        glx.aggregate_backward(glx.SUM, rows, None, g, 1, out_dtype="float16", chunked=True)
    with pytest.raises(ValueError):
        glx.aggregate_weighted_backward_x(glx.SUM, rows, np.ones(1, np.float32), None, g, 1, out_dtype="float16",
                                          chunked=True)
