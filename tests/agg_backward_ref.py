"""The contract of glx_aggregate_arg / glx_aggregate_backward restated in numpy, shared by
test_agg_backward_cpu.py, test_gpu_agg_backward.py and test_gpu_segment_aggregate.py.  float32 arithmetic throughout:
numpy's float32 add and divide are the correctly rounded IEEE operations the kernels use (-ffp-contract=off, the
correctly rounded divide)."""
import numpy as np

SUM, MEAN, MAX, MIN, PROD = 0, 1, 2, 3, 4
FLT_MAX = np.float32(np.finfo(np.float32).max)
MAX_INIT = np.float32(-37.0)  # max_aggregator.cc:28: float(FLT_MIN_10_EXP)


def segment_starts(cnt, num_ids, num_segments):
    """start[num_segments + 1]: segment s is positions [start[s], start[s + 1]) -- the prefix sums of the forward's
    counts, or the implied layout (num_ids // num_segments positions each) for cnt=None."""
    if cnt is None:
        f = num_ids // num_segments if num_segments > 0 else 0
        cnt = np.full(num_segments, f, np.int64)
    start = np.zeros(num_segments + 1, np.int64)
    np.cumsum(np.asarray(cnt, np.int64), out=start[1:])
    return start


def cursor_counts(segment_ids, num_segments):
    """cnt[num_segments] of the forward's cursor (aggregating_request.cc:86-105): ids are handed out while the
    sequence stays non-decreasing and inside [0, num_segments); the first violation stalls it for good."""
    seg = np.asarray(segment_ids, np.int64)
    valid = len(seg)
    prev = -1
    for i, s in enumerate(seg):
        if s < 0 or s >= num_segments or s < prev:
            valid = i
            break
        prev = s
    return np.bincount(seg[:valid], minlength=num_segments).astype(np.int32)


def _row_of(X, r, default_attr):
    if 0 <= r < X.shape[0]:
        return X[r].astype(np.float32)
    return np.full(X.shape[1], default_attr, np.float32)


def fold(op, X, ids, start, default_attr=0.0):
    """The forward: emb[num_segments, D], every element folded left to right in float32."""
    S, D = len(start) - 1, X.shape[1]
    emb = np.empty((S, D), np.float32)
    for s in range(S):
        a, b = int(start[s]), int(start[s + 1])
        if a == b:
            emb[s] = default_attr
            continue
        acc = np.full(D, {MAX: MAX_INIT, MIN: FLT_MAX}.get(op, np.float32(0.0)), np.float32)
        for p in range(a, b):
            x = _row_of(X, ids[p], default_attr)
            if op == MAX:
                acc = np.where(acc < x, x, acc)
            elif op == MIN:
                acc = np.where(x < acc, x, acc)
            else:
                acc = (acc + x).astype(np.float32)
        if op == MEAN:
            acc = (acc / np.float32(b - a)).astype(np.float32)
        emb[s] = acc
    return emb


def fold_arg(op, X, ids, start, default_attr=0.0):
    """(emb, arg) of Max / Min: arg[s, c] = the position whose element the select last took, -1 if it took none."""
    S, D = len(start) - 1, X.shape[1]
    emb = np.empty((S, D), np.float32)
    arg = np.full((S, D), -1, np.int32)
    for s in range(S):
        a, b = int(start[s]), int(start[s + 1])
        acc = np.full(D, MAX_INIT if op == MAX else FLT_MAX, np.float32)
        for p in range(a, b):
            x = _row_of(X, ids[p], default_attr)
            take = (acc < x) if op == MAX else (x < acc)
            acc = np.where(take, x, acc)
            arg[s] = np.where(take, p, arg[s])
        emb[s] = acc if b > a else default_attr
    return emb, arg


def terms(op, rows, cnt, grad_out, num_rows, arg=None):
    """(positions, row of each, term[len(positions), D], selected[len(positions), D]): the consumed, in-range
    positions in ascending order and what each adds (where `selected`) to its row."""
    rows = np.asarray(rows, np.int64)
    n = len(rows)
    S, D = grad_out.shape
    start = segment_starts(cnt, n, S)
    total = min(int(start[-1]), n)
    p = np.arange(total, dtype=np.int64)
    seg = np.searchsorted(start, p, side="right") - 1
    keep = (rows[:total] >= 0) & (rows[:total] < num_rows)
    p, seg = p[keep], seg[keep]
    g = grad_out[seg].astype(np.float32)
    sel = np.ones(g.shape, bool)
    if op == MEAN:
        div = (start[1:] - start[:-1])[seg].astype(np.float32)
        g = (g / div[:, None]).astype(np.float32)
    elif op in (MAX, MIN):
        sel = arg[seg] == p[:, None].astype(np.int32)
    return p, rows[p], g, sel


def backward(op, rows, cnt, grad_out, num_rows, arg=None):
    """grad_x[num_rows, D]: +0.0f plus one float32 term per consumed position with rows[p] == r, in ascending p."""
    p, r, g, sel = terms(op, rows, cnt, grad_out, num_rows, arg)
    gx = np.zeros((num_rows, grad_out.shape[1]), np.float32)
    order = np.argsort(r, kind="stable")  # by (row, position)
    r, g, sel = r[order], g[order], sel[order]
    first = np.searchsorted(r, r, side="left")
    rank = np.arange(len(r)) - first  # k-th reference of its row
    for k in range(int(rank.max()) + 1 if len(r) else 0):
        at = np.flatnonzero(rank == k)  # at most one entry per row: a plain fancy-indexed update
        cur = gx[r[at]]
        gx[r[at]] = np.where(sel[at], (cur + g[at]).astype(np.float32), cur)
    return gx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
