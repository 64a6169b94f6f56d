"""The contracts of glx_rows_coalesce / glx_embedding_update restated in numpy, shared by
test_embedding_cpu.py, test_gpu_embedding.py and test_gpu_sparse_embedding.py.  With dtype=float32 every numpy operation
below is one correctly rounded IEEE operation on float32 operands -- what the kernels do (-ffp-contract=off, the correctly
rounded divide and square root); dtype=float64 is the same arithmetic in double, for comparison with torch's optimizers."""
import math

import numpy as np

SGD, ADAGRAD, ADAM = 0, 1, 2
CHUNK = 256


def coalesce(rows, g, num_rows, dtype=np.float32, chunk=CHUNK):
    """(urows[n] int64, ug[U, D], U): positions outside [0, num_rows) dropped; urows[:U] the distinct rows ascending,
    urows[U:] = -1.  Row u's positions, ascending, are cut into chunks of `chunk` list entries; a chunk's partial is
    +0.0 plus its g rows in ascending position, ug[u] is +0.0 plus the partials in ascending chunk."""
    rows = np.asarray(rows, np.int64)
    g = np.asarray(g, dtype)
    n, D = len(rows), g.shape[1]
    p = np.flatnonzero((rows >= 0) & (rows < num_rows))
    order = np.argsort(rows[p], kind="stable")  # by (row, position)
    p = p[order]
    r = rows[p]
    uniq, first = np.unique(r, return_index=True)
    U = len(uniq)
    urows = np.full(n, -1, np.int64)
    urows[:U] = uniq
    u_of = np.searchsorted(uniq, r)
    rank = np.arange(len(r)) - first[u_of]  # k-th reference of its row
    ck, within = rank // chunk, rank % chunk
    num_chunks = np.zeros(U, np.int64)
    np.maximum.at(num_chunks, u_of, ck + 1)
    slot0 = np.concatenate([[0], np.cumsum(num_chunks)])[:-1] if U else np.zeros(0, np.int64)
    partial = np.zeros((int(num_chunks.sum()), D), dtype)
    slot = slot0[u_of] + ck
    for k in range(int(within.max()) + 1 if len(r) else 0):
        at = np.flatnonzero(within == k)  # at most one entry per chunk: a plain fancy-indexed update
        partial[slot[at]] = (partial[slot[at]] + g[p[at]]).astype(dtype)
    ug = np.zeros((U, D), dtype)
    for k in range(int(num_chunks.max()) if U else 0):
        at = np.flatnonzero(num_chunks > k)
        ug[at] = (ug[at] + partial[slot0[at] + k]).astype(dtype)
    return urows, ug, U


def plain_sum(rows, g, num_rows, dtype=np.float32):
    """coalesce without the chunk rule: every list in plain ascending order"""
    return coalesce(rows, g, num_rows, dtype, chunk=1 << 62)


def adam_scalars(lr, betas, eps, t):
    """(alpha, eps, beta1, c1, beta2, c2) of global step t (1-based), computed in double"""
    b1, b2 = float(betas[0]), float(betas[1])
    alpha = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return alpha, float(eps), b1, 1.0 - b1, b2, 1.0 - b2


def update(algo, W, urows, ug, state1=None, state2=None, alpha=0.0, eps=0.0, beta1=0.0, c1=0.0, beta2=0.0, c2=0.0,
           dtype=np.float32):
    """One step IN PLACE on W (and the state tables): entries of urows outside [0, num_rows) are skipped, ug[u] is entry
    u's gradient (ug may have fewer rows than urows has entries: the tail of a coalesce is -1).  The scalars are rounded
    to `dtype` once; every operation after that is one rounding."""
    urows = np.asarray(urows, np.int64)
    u = np.flatnonzero((urows >= 0) & (urows < W.shape[0]))
    r = urows[u]
    assert len(np.unique(r)) == len(r), "the valid entries must name distinct rows"
    f = dtype
    alpha, eps, beta1, c1, beta2, c2 = (f(x) for x in (alpha, eps, beta1, c1, beta2, c2))
    g = np.asarray(ug, f)[u]
    w = W[r].astype(f)
    if algo == SGD:
        w = (w - (alpha * g).astype(f)).astype(f)
    elif algo == ADAGRAD:
        s = (state1[r].astype(f) + (g * g).astype(f)).astype(f)
        state1[r] = s
        w = (w - (alpha * (g / (np.sqrt(s).astype(f) + eps).astype(f)).astype(f)).astype(f)).astype(f)
    else:
        m = ((beta1 * state1[r].astype(f)).astype(f) + (c1 * g).astype(f)).astype(f)
        v = ((beta2 * state2[r].astype(f)).astype(f) + (c2 * (g * g).astype(f)).astype(f)).astype(f)
        state1[r], state2[r] = m, v
        w = (w - (alpha * (m / (np.sqrt(v).astype(f) + eps).astype(f)).astype(f)).astype(f)).astype(f)
    W[r] = w


def same_bits(a, b):
    """bit equality of two float32 arrays, except that a NaN matches a NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))
