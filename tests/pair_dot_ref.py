"""The contracts of glx_pair_dot and glx_pair_dot_backward restated in numpy, shared by
test_pair_dot_cpu.py, test_gpu_pair_dot.py and test_gpu_pair_score.py.

forward is computed in float64 and comes with the bound its contract states.  backward is a loop over the pairs in
ascending p with a separately rounded multiply and add per term (numpy's float32 multiply and add are the correctly
rounded IEEE operations; nothing here can fuse them); dtype=np.float64 runs the same loop in double for the gradient
checks."""
import numpy as np

from agg_weighted_ref import same_bits, within_bound  # noqa: F401  (re-exported for the tests)


def _row(X, r, default_attr, dtype):
    if 0 <= r < X.shape[0]:
        return X[r].astype(dtype)
    return np.full(X.shape[1], default_attr, dtype)


def forward(xa, ia, xb, ib, heads=1, repeat=1, default_attr=0.0):
    """(out[n, heads] float64, bound[n, heads] float64): the exact dot products of row ia[p // repeat] of xa with row
    ib[p] of xb over each head's columns and, for any order of a C-term float32 dot product,
    |got - exact| <= C * 2^-23 * sum_c |a * b| + 2^-126 (gamma_C with a factor 2 of slack: FMA or no FMA)."""
    ia, ib = np.asarray(ia, np.int64).reshape(-1), np.asarray(ib, np.int64).reshape(-1)
    n, D = len(ib), xa.shape[1]
    assert xb.shape[1] == D and D % heads == 0 and len(ia) * repeat == n
    C = D // heads
    out = np.zeros((n, heads), np.float64)
    bound = np.zeros((n, heads), np.float64)
    with np.errstate(all="ignore"):
        for p in range(n):
            prod = _row(xa, ia[p // repeat], default_attr, np.float64) * _row(xb, ib[p], default_attr, np.float64)
            prod = prod.reshape(heads, C)
            out[p] = prod.sum(1)
            bound[p] = C * 2.0 ** -23 * np.abs(prod).sum(1) + 2.0 ** -126
    return out, bound


def backward(side, ia, ib, g, x_other, num_rows_self, repeat=1, default_attr=0.0, dtype=np.float32):
    """grad_self[num_rows_self, D]: +0.0 plus round(g[p, head] * other_row(p)) per pair p whose own index (side 0:
    ia[p // repeat], side 1: ib[p]) is the row, in ascending p; an own index outside the table gets nothing, an
    other-side index outside its table multiplies a row of default_attr"""
    ia, ib = np.asarray(ia, np.int64).reshape(-1), np.asarray(ib, np.int64).reshape(-1)
    n, D = len(ib), x_other.shape[1]
    g = np.asarray(g)
    g = g.reshape(n, g.shape[-1] if g.ndim > 1 else 1)
    assert side in (0, 1) and len(ia) * repeat == n and D % g.shape[1] == 0
    C = D // g.shape[1]
    grad = np.zeros((num_rows_self, D), dtype)
    with np.errstate(all="ignore"):
        for p in range(n):
            own, other = (ia[p // repeat], ib[p]) if side == 0 else (ib[p], ia[p // repeat])
            if not 0 <= own < num_rows_self:
                continue
            term = (np.repeat(g[p].astype(dtype), C) * _row(x_other, other, default_attr, dtype)).astype(dtype)
            grad[own] = (grad[own] + term).astype(dtype)
    return grad
