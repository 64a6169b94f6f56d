"""The CHUNKED order of the row gradients (glx_aggregate_backward_chunked and
glx_aggregate_weighted_backward_x_chunked) restated in numpy, shared by test_agg_chunked_cpu.py,
test_gpu_agg_chunked.py and test_gpu_agg_chunked_autograd.py.

The terms are the default order's -- agg_backward_ref.terms, and agg_weighted_ref's two-rounding product -- and only the
order of the additions differs: the list of a row (its consumed, in-range positions, ascending) is cut into chunks of
CHUNK entries, whether a Max / Min arg selects an entry or not; a chunk's partial is +0.0f plus its selected terms in
ascending position; the row is +0.0f plus its partials in ascending chunk.  float32 arithmetic throughout."""
import numpy as np

import agg_backward_ref as ref
import agg_weighted_ref as wref

CHUNK = 256  # GLX_COALESCE_CHUNK


def chunked_sum(r, g, sel, num_rows, chunk=CHUNK):
    """grad_x[num_rows, D] from the list entries in ascending position: r[k] the row of entry k, g[k, D] its term,
    sel[k, D] whether the term is added"""
    D = g.shape[1]
    gx = np.zeros((num_rows, D), np.float32)
    if len(r) == 0:
        return gx
    order = np.argsort(r, kind="stable")  # by (row, position)
    r, g, sel = r[order], g[order], sel[order]
    rank = np.arange(len(r)) - np.searchsorted(r, r, side="left")  # k-th entry of its row's list
    chunk_of, within = rank // chunk, rank % chunk
    span = int(chunk_of.max()) + 1
    slots, slot_of = np.unique(r * span + chunk_of, return_inverse=True)  # one partial per (row, chunk)
    partial = np.zeros((len(slots), D), np.float32)
    with np.errstate(all="ignore"):
        for k in range(int(within.max()) + 1):
            at = np.flatnonzero(within == k)  # at most one entry per partial: a plain fancy-indexed update
            cur = partial[slot_of[at]]
            partial[slot_of[at]] = np.where(sel[at], (cur + g[at]).astype(np.float32), cur)
        slot_row, slot_chunk = slots // span, slots % span
        for k in range(span):
            at = np.flatnonzero(slot_chunk == k)  # at most one partial per row
            gx[slot_row[at]] = (gx[slot_row[at]] + partial[at]).astype(np.float32)
    return gx


def backward(op, rows, cnt, grad_out, num_rows, arg=None, chunk=CHUNK):
    """glx_aggregate_backward_chunked: agg_backward_ref.backward's terms in the chunked order"""
    _, r, g, sel = ref.terms(op, rows, cnt, grad_out, num_rows, arg)
    return chunked_sum(r, g, sel, num_rows, chunk)


def weighted_terms(op, rows, w, cnt, grad_out, num_rows):
    """(row of each consumed, in-range position in ascending order, term[., D]): round(w[p, head] * t), t = grad_out[s(p)]
    (Sum) or round(grad_out[s(p)] / count) (Mean) -- agg_weighted_ref.backward_x's"""
    rows = np.asarray(rows, np.int64)
    S, D = grad_out.shape
    w, C = wref._weights(w, D)
    start = wref.starts(cnt, len(rows), S)
    p = np.arange(int(start[-1]), dtype=np.int64)
    seg = np.searchsorted(start, p, side="right") - 1
    keep = (rows[p] >= 0) & (rows[p] < num_rows)
    p, seg = p[keep], seg[keep]
    with np.errstate(all="ignore"):
        t = grad_out[seg].astype(np.float32)
        if op == wref.MEAN:
            t = (t / (start[1:] - start[:-1])[seg].astype(np.float32)[:, None]).astype(np.float32)
        term = (np.repeat(w[p].astype(np.float32), C, axis=1) * t).astype(np.float32)
    return rows[p], term


def backward_weighted_x(op, rows, w, cnt, grad_out, num_rows, chunk=CHUNK):
    """glx_aggregate_weighted_backward_x_chunked"""
    r, term = weighted_terms(op, rows, w, cnt, grad_out, num_rows)
    return chunked_sum(r, term, np.ones(term.shape, bool), num_rows, chunk)


def list_lengths(rows, cnt, num_segments, num_rows):
    """entries of every row's list: the consumed, in-range positions that name it"""
    rows = np.asarray(rows, np.int64)
    total = int(wref.starts(cnt, len(rows), num_segments)[-1])
    r = rows[:total]
    return np.bincount(r[(r >= 0) & (r < num_rows)], minlength=num_rows)
