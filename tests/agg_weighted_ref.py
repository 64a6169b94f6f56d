"""The contracts of glx_aggregate_weighted and its two gradients restated in numpy, shared by
test_agg_weighted_cpu.py, test_gpu_agg_weighted.py and test_gpu_weighted_segment_aggregate.py.

forward and backward_x are loops with a separately rounded multiply and add per term (numpy's float32 multiply and add
are the correctly rounded IEEE operations; nothing here can fuse them); dtype=np.float64 runs the same loops in double
for the finite-difference check.  backward_w is computed in float64 and comes with the bound its contract states."""
import numpy as np

import agg_backward_ref as ref

SUM, MEAN = ref.SUM, ref.MEAN


def starts(cnt, num_ids, num_segments):
    """start[num_segments + 1] of the consumed positions: prefix sums of the counts clamped at 0 (None: the implied
    layout), never beyond num_ids"""
    if cnt is not None:
        cnt = np.maximum(np.asarray(cnt, np.int64), 0)
    return np.minimum(ref.segment_starts(cnt, num_ids, num_segments), num_ids)


def _weights(w, dim):
    """w[n] or w[n, H] -> (w[n, H], C)"""
    w = np.asarray(w)
    w = w.reshape(len(w), -1)
    assert dim % w.shape[1] == 0
    return w, dim // w.shape[1]


def _row(X, r, default_attr, dtype):
    if 0 <= r < X.shape[0]:
        return X[r].astype(dtype)
    return np.full(X.shape[1], default_attr, dtype)


def forward(op, X, rows, w, cnt, num_segments, default_attr=0.0, dtype=np.float32):
    """emb[num_segments, D]: acc = 0; acc = round(acc + round(w[p, head] * xrow(p))) in ascending p; Mean: / count"""
    D = X.shape[1]
    w, C = _weights(w, D)
    start = starts(cnt, len(rows), num_segments)
    emb = np.empty((num_segments, D), dtype)
    with np.errstate(all="ignore"):
        for s in range(num_segments):
            a, b = int(start[s]), int(start[s + 1])
            if a == b:
                emb[s] = default_attr
                continue
            acc = np.zeros(D, dtype)
            for p in range(a, b):
                term = (np.repeat(w[p].astype(dtype), C) * _row(X, rows[p], default_attr, dtype)).astype(dtype)
                acc = (acc + term).astype(dtype)
            if op == MEAN:
                acc = (acc / dtype(b - a)).astype(dtype)
            emb[s] = acc
    return emb


def backward_x(op, rows, w, cnt, grad_out, num_rows, dtype=np.float32):
    """grad_x[num_rows, D]: +0.0 plus round(w[p, head] * t) per consumed position with rows[p] == r, in ascending p;
    t = grad_out[s(p)] (Sum) or round(grad_out[s(p)] / count) (Mean)"""
    rows = np.asarray(rows, np.int64)
    S, D = grad_out.shape
    w, C = _weights(w, D)
    start = starts(cnt, len(rows), S)
    gx = np.zeros((num_rows, D), dtype)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = int(start[s]), int(start[s + 1])
            for p in range(a, b):  # ascending p overall: every row sees its positions in order
                r = rows[p]
                if not 0 <= r < num_rows:
                    continue
                t = grad_out[s].astype(dtype)
                if op == MEAN:
                    t = (t / dtype(b - a)).astype(dtype)
                term = (np.repeat(w[p].astype(dtype), C) * t).astype(dtype)
                gx[r] = (gx[r] + term).astype(dtype)
    return gx


def backward_w(op, X, rows, heads, cnt, grad_out, default_attr=0.0):
    """(grad_w[n, heads] float64, bound[n, heads] float64): the exact dot products and, for any order of a C-term
    float32 dot product, |got - exact| <= C * 2^-23 * sum_c |grad_out * x| + 2^-126 (gamma_C with a factor 2 of slack,
    which covers FMA or no FMA and Mean's one division).  A position that was not consumed: 0 with bound 0."""
    n = len(rows)
    S, D = grad_out.shape
    C = D // heads
    start = starts(cnt, n, S)
    gw = np.zeros((n, heads), np.float64)
    bound = np.zeros((n, heads), np.float64)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = int(start[s]), int(start[s + 1])
            for p in range(a, b):
                prod = grad_out[s].astype(np.float64) * _row(X, rows[p], default_attr, np.float64)
                if op == MEAN:
                    prod = prod / float(b - a)
                prod = prod.reshape(heads, C)
                gw[p] = prod.sum(1)
                bound[p] = C * 2.0 ** -23 * np.abs(prod).sum(1) + 2.0 ** -126
    return gw, bound


def same_bits(a, b):
    """bit equality, except that a NaN matches any NaN: an invalid operation's NaN has no contracted sign or payload
    (x86 produces the negative quiet NaN, the GPU the positive one)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def within_bound(got, want, bound):
    """grad_w against its float64 reference: inside the bound where the reference is finite, the same non-finite value
    elsewhere"""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(want) & np.isfinite(bound)
    ok = np.all(np.abs(got[fin] - want[fin]) <= bound[fin])
    rest_g, rest_w = got[~fin], want[~fin]
    nan = np.isnan(rest_w)
    return bool(ok and np.array_equal(np.isnan(rest_g), nan) and np.array_equal(rest_g[~nan], rest_w[~nan]))
