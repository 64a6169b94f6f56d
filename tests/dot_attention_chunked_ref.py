"""The CHUNKED order of dot-product attention (glx_dot_attention_chunked and
glx_dot_attention_backward_chunked) restated in numpy, shared by test_dot_attention_chunked_cpu.py,
test_gpu_dot_attention_chunked.py and test_gpu_dot_attention_chunked_autograd.py.

Only the two segment sums change their order: a segment of more than CHUNK consumed positions is cut into chunks of
CHUNK positions, a chunk's partial is +0.0f plus its terms in ascending position, the segment is +0.0f plus its
partials in ascending chunk; a shorter segment keeps the default fold.  float32 step by step, as dot_attention_ref.out.
The logits, the softmax bound, ga, grad_e and grad_edge are dot_attention_ref's; grad_k and grad_v are
agg_chunked_ref.backward_weighted_x."""
import numpy as np

import agg_chunked_ref as cref
import dot_attention_ref as dref

CHUNK = cref.CHUNK  # GLX_COALESCE_CHUNK
SUM = dref.SUM
list_lengths = cref.list_lengths  # entries of every row's list


def long_segments(cnt, num_ids, num_segments, chunk=CHUNK):
    """bool[num_segments]: more than `chunk` consumed positions"""
    return np.diff(dref.starts(cnt, num_ids, num_segments)) > chunk


def _fold(w, x, cnt, num_segments, chunk=CHUNK):
    """[S, D] float32: the terms round(w[p, h] * x[p]) of segment sg summed in the chunked order"""
    x = np.asarray(x, np.float32)
    n, D = x.shape
    res = np.zeros((num_segments, D), np.float32)
    if n == 0:
        return res
    w = np.asarray(w, np.float32).reshape(n, -1)
    C = D // w.shape[1]
    start = dref.starts(cnt, n, num_segments)
    with np.errstate(all="ignore"):
        term = (np.repeat(w, C, axis=1) * x).astype(np.float32)
        for s in range(num_segments):
            a, b = int(start[s]), int(start[s + 1])
            if b - a <= chunk:  # short: the default order
                acc = np.zeros(D, np.float32)
                for p in range(a, b):
                    acc = (acc + term[p]).astype(np.float32)
                res[s] = acc
                continue
            acc = np.zeros(D, np.float32)
            for c0 in range(a, b, chunk):
                part = np.zeros(D, np.float32)
                for p in range(c0, min(c0 + chunk, b)):
                    part = (part + term[p]).astype(np.float32)
                acc = (acc + part).astype(np.float32)
            res[s] = acc
    return res


def out(alpha, vv, cnt, num_segments, chunk=CHUNK):
    """out[S, D] float32 from the engine's own alpha, in the chunked order; an empty segment is +0.0"""
    return _fold(alpha, vv, cnt, num_segments, chunk)


def grad_q(grad_e, kk, cnt, num_segments, chunk=CHUNK):
    """grad_q[S, D] float32 from the engine's own grad_e, in the chunked order"""
    return _fold(grad_e, kk, cnt, num_segments, chunk)


def grad_rows(w, rows, cnt, grad_out, num_rows, chunk=CHUNK):
    """grad_k (w = grad_e, grad_out = q) or grad_v (w = alpha, grad_out = grad_out) in the chunked row order"""
    grad_out = np.asarray(grad_out, np.float32)
    if len(rows) == 0:
        return np.zeros((num_rows, grad_out.shape[1]), np.float32)
    return cref.backward_weighted_x(SUM, rows, np.asarray(w, np.float32), cnt, grad_out, num_rows, chunk)


# ---- the requests the CPU and the GPU tests share ---------------------------------------------------------------

class Request:
    """one dot_attention request in numpy: q [S, D], k, v [M, D], rows [n], edge [n, D] or None, cnt [S] or None, and
    the gradient g [S, D] of out"""

    def __init__(self, dim, heads, cnt, n, S, num_rows, seed, with_edge):
        rng = np.random.default_rng(seed)
        self.dim, self.heads, self.cnt, self.n, self.S, self.num_rows = dim, heads, cnt, n, S, num_rows
        self.q = rng.standard_normal((S, dim)).astype(np.float32)
        self.k = rng.standard_normal((num_rows, dim)).astype(np.float32)
        self.v = rng.standard_normal((num_rows, dim)).astype(np.float32)
        self.rows = rng.integers(0, num_rows, n).astype(np.int64)
        self.edge = rng.standard_normal((n, dim)).astype(np.float32) if with_edge else None
        self.g = rng.standard_normal((S, dim)).astype(np.float32)
        self.scale = float(dref.default_scale(dim, heads))


# The ragged request.  Lengths on both sides of the 256-position boundary (255 | 256 | 257), two chunks exactly (512),
# one position past them (513) and a third chunk that is not full (700); empty segments at both ends and two adjacent
# ones; three more long segments carry the planted values.
HUB_LENGTHS = [0, 7, 255, 0, 0, 256, 257, 1, 512, 40, 513, 700, 300, 260, 270, 33, 0]
SEG_255, SEG_256, SEG_257, SEG_512, SEG_513, SEG_700 = 2, 5, 6, 8, 10, 11
SEG_ZERO, SEG_NAN, SEG_INF, SEG_LAST = 12, 13, 14, 15
HUB_ROWS = 64
ROW_257, ROW_700, ROW_ZERO, ROW_INF, ROW_NAN = 56, 57, 58, 59, 60  # rows 0 .. 55 are ordinary


def hub_seed(dim, heads, with_edge):
    """the seed of the GPU test's hub_request for one shape: test_dot_attention_chunked_cpu.py checks that the two
    orders differ under it"""
    return 1000 + 4 * dim + 2 * heads + int(with_edge)


def hub_request(dim, heads, with_edge, seed, cut=False):
    """HUB_LENGTHS with 5 positions behind them that nobody consumes (cut: the last counts promise 20 positions more
    than the request has).  Planted:
      SEG_700   q = 0: 700 equal logits, soft is exactly 1.0f / 700
      SEG_513   its position 300 names ROW_INF, whose k is -inf in the first column of every head, under a q that is
                positive there: a -inf logit among finite ones, soft is +0.0f
      SEG_INF   every position names ROW_INF: only -inf logits, a NaN column
      SEG_NAN   its position 100 names ROW_NAN (k is NaN in column 0): head 0 is a NaN column
      SEG_ZERO  every position names ROW_ZERO, whose v is -0.0f: without an edge term every term of out is -0.0f, and
                out is +0.0f only because every partial and the combine start at +0.0f
      ROW_257, ROW_700   named by 257 and by 700 positions: grad_k / grad_v cross the row-chunk boundary
      ids -1 and num_rows among the rows"""
    rng = np.random.default_rng(seed)
    cnt = np.array(HUB_LENGTHS, np.int32)
    total = int(cnt.sum())
    n = total - 20 if cut else total + 5
    r = Request(dim, heads, cnt, n, len(cnt), HUB_ROWS, seed, with_edge)
    start = np.concatenate([[0], np.cumsum(cnt)])
    C = dim // heads
    rows = rng.integers(0, 56, total).astype(np.int64)
    ordinary = np.ones(total, bool)
    for sg, row in ((SEG_ZERO, ROW_ZERO), (SEG_INF, ROW_INF)):
        rows[start[sg]:start[sg + 1]] = row
        ordinary[start[sg]:start[sg + 1]] = False
    for sg in (SEG_NAN, SEG_LAST):
        ordinary[start[sg]:start[sg + 1]] = False
    rows[start[SEG_513] + 300] = ROW_INF
    rows[start[SEG_NAN] + 100] = ROW_NAN
    ordinary[start[SEG_513] + 300] = False
    free = rng.permutation(np.flatnonzero(ordinary))
    rows[free[:257]] = ROW_257
    rows[free[257:957]] = ROW_700
    rows[free[957]] = -1
    rows[free[958]] = HUB_ROWS
    r.rows[:min(n, total)] = rows[:min(n, total)]
    r.q[SEG_700] = 0.0
    for sg in (SEG_513, SEG_INF):
        r.q[sg, ::C] = np.abs(r.q[sg, ::C]) + np.float32(0.1)
    r.k[ROW_INF, ::C] = -np.inf
    r.k[ROW_NAN, 0] = np.nan
    r.v[ROW_ZERO] = np.float32(-0.0)
    return r


def implied_request(dim, heads, with_edge, seed, num_segments, fanout, num_rows=97):
    """cnt=None: num_segments segments of `fanout` positions each"""
    return Request(dim, heads, None, num_segments * fanout, num_segments, num_rows, seed, with_edge)
