"""The contracts of glx_segment_softmax and glx_segment_softmax_backward (include/glx.h) restated
in numpy float64, shared by test_segment_softmax_cpu.py, test_gpu_segment_softmax.py and
test_gpu_segment_softmax_autograd.py.  Both functions return the float64 value computed from the float32 inputs and
the bound the contract states around it; the layout, within_bound and same_bits are agg_weighted_ref's."""
import numpy as np

import agg_weighted_ref as wref

starts, within_bound, same_bits = wref.starts, wref.within_bound, wref.same_bits

# The error of the platform's float32 exp in ulp, as the tests use it: ceil(measured) + 1, and at least 2.  The
# measurement is part (a) of scripts/r13/segment_softmax_probe.py (torch.exp on the device against float64 numpy.exp)
# and its figure belongs in profiles/r13/segment_softmax.txt; until that file exists this is the floor of 2, which
# stands for a measured maximum of at most 1 ulp.  Never taken from the kernel under test.
E = 2


def _two_d(a, dtype):
    a = np.asarray(a, dtype)
    return a.reshape(len(a), -1), a.shape


def forward(e, cnt, num_segments):
    """(alpha float64, bound float64), both of e's shape.  Per (segment, head) over the k consumed positions:
    alpha = exp(d) / sum exp(d), d = e - max e;  |got - alpha| <= alpha (2 |d| + 2 k + 4 E + 4) 2^-24 + 2^-126.
    Exact rules: a position that is not consumed is 0 with bound 0; a -inf logit among finite ones is 0 with bound 0;
    a column with a NaN or +inf logit, or with -inf only, is NaN."""
    e2, shape = _two_d(e, np.float32)
    n, H = e2.shape
    start = starts(cnt, n, num_segments)
    alpha, bound = np.zeros((n, H), np.float64), np.zeros((n, H), np.float64)
    with np.errstate(all="ignore"):
        for s in range(num_segments):
            a, b = int(start[s]), int(start[s + 1])
            if a == b:
                continue
            x = e2[a:b].astype(np.float64)
            bad = np.isnan(x).any(0) | (x == np.inf).any(0) | (x == -np.inf).all(0)
            d = x - np.where(bad, 0.0, x.max(0))
            t = np.exp(d)
            al = t / t.sum(0)
            bd = al * (2 * np.abs(d) + 2 * (b - a) + 4 * E + 4) * 2.0 ** -24 + 2.0 ** -126
            bd[np.isinf(d)] = 0.0  # the mask: exactly +0.0
            al[:, bad], bd[:, bad] = np.nan, np.nan
            alpha[a:b], bound[a:b] = al, bd
    return alpha.reshape(shape), bound.reshape(shape)


def backward(alpha, grad_alpha, cnt, num_segments):
    """(grad_e float64, bound float64), both of alpha's shape.  Per (segment, head) over the k consumed positions:
    grad_e = alpha (g - sum_q alpha_q g_q);  |got - grad_e| <= |alpha| (k + 2) 2^-23 (|g| + sum_q |alpha_q g_q|) + 2^-126.
    A position that is not consumed is 0 with bound 0; non-finite inputs give the IEEE result of the formula."""
    a2, shape = _two_d(alpha, np.float32)
    g2, gshape = _two_d(grad_alpha, np.float32)
    assert shape == gshape
    n, H = a2.shape
    start = starts(cnt, n, num_segments)
    grad, bound = np.zeros((n, H), np.float64), np.zeros((n, H), np.float64)
    with np.errstate(all="ignore"):
        for s in range(num_segments):
            a, b = int(start[s]), int(start[s + 1])
            if a == b:
                continue
            al, g = a2[a:b].astype(np.float64), g2[a:b].astype(np.float64)
            prod = al * g
            grad[a:b] = al * (g - prod.sum(0))
            bound[a:b] = np.abs(al) * (b - a + 2) * 2.0 ** -23 * (np.abs(g) + np.abs(prod).sum(0)) + 2.0 ** -126
    return grad.reshape(shape), bound.reshape(shape)
