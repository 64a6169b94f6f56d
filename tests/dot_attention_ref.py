"""The contracts of glx_dot_attention and glx_dot_attention_backward (include/glx.h) restated
in numpy, shared by test_dot_attention_cpu.py, test_gpu_dot_attention.py and test_gpu_transformer_conv.py.

Where the contract is bit-exact the restatement is float32 step by step (numpy's float32 add and multiply are the
correctly rounded IEEE operations; nothing here can fuse them): kk and vv, the dropout of soft, out, grad_q, grad_edge,
grad_k and grad_v.  Where it is a tolerance it is float64 plus the bound: the logits, soft, ga and grad_e.  Each stage
takes the engine's own previous output, as the GAT tests do: logit -> soft -> out, and grad_e -> grad_q / grad_edge /
grad_k / grad_v.

The bounds are derived, not measured:
  logit   a C-term float32 dot product in any order lies within C * 2^-23 * sum |terms| + 2^-126 of the exact value
          (agg_weighted_ref.backward_w's bound, which has a factor 2 of slack over gamma_C); e = fmul_rn(dot, scale)
          scales that by |scale| and rounds once more: + 2^-24 |e| + 2^-126
  soft    segment_softmax_ref.forward's bound, with its E
  ga      delta' = dropscale * (C * 2^-23 * sum |terms| + 2^-126) around dropscale * the exact dot product (the one
          rounding of fmul_rn(ga_raw, dropscale) is inside the slack of the softmax gradient's (k + 2) * 2^-23, which
          needs (k + 2) * 2^-24 to first order); a dropped element is +0.0 exactly
  grad_e  d = soft (ga - sum_q soft_q ga_q) computed from a ga that is off by at most delta':
            segment_softmax_ref.backward's bound at |ga| + delta':  |soft| (k + 2) 2^-23 (|ga| + delta' + sum_q |soft_q| (|ga_q| + delta'_q))
            the propagated term:                                    |soft_p| (delta'_p + sum_q |soft_q| delta'_q)
          and grad_e = fmul_rn(d, scale): the whole times |scale| (1 + 2^-23), + 2^-126
"""
import numpy as np

import agg_weighted_ref as wref
import gat_attention_ref as gref
import segment_softmax_ref as sref

SUM = wref.SUM
starts, within_bound, same_bits = wref.starts, wref.within_bound, wref.same_bits
keep_mask, drop, segment_of = gref.keep_mask, gref.drop, gref.segment_of


def default_scale(dim, heads):
    """1 / sqrt(C) rounded to float32"""
    return np.float32(1.0) / np.sqrt(np.float32(dim // heads))


def gathered(x, rows, edge, default_attr=0.0, dtype=np.float32):
    """kk or vv [n, D]: x[rows[p]] (a row of default_attr outside the table) plus edge[p], one add per element"""
    x = np.asarray(x)
    rows = np.asarray(rows, np.int64)
    inside = (rows >= 0) & (rows < len(x))
    out = np.full((len(rows), x.shape[1]), default_attr, dtype)
    out[inside] = x[rows[inside]].astype(dtype)
    if edge is not None:
        with np.errstate(all="ignore"):
            out = (out + np.asarray(edge).astype(dtype)).astype(dtype)
    return out


def logits(q, kk, cnt, num_segments, heads, scale):
    """(e float64, bound float64) [n, heads] from the float32 q and kk: e = scale * sum_c q[sg, c] kk[p, c]; a position
    nobody consumed is 0 with bound 0"""
    dot, bound = wref.backward_w(SUM, kk, np.arange(len(kk)), heads, cnt, np.asarray(q, np.float32))
    sc = float(np.float32(scale))
    with np.errstate(all="ignore"):
        e = dot * sc
        b = bound * abs(sc) + 2.0 ** -24 * np.abs(e) + 2.0 ** -126
    b[segment_of(cnt, len(kk), num_segments) == num_segments] = 0.0
    return e, b


def softmax(e, cnt, num_segments):
    """(soft float64, bound float64) of the engine's own float32 logits: segment_softmax_ref.forward"""
    e = np.asarray(e, np.float32)
    if e.size == 0:  # no positions
        return np.zeros(e.shape), np.zeros(e.shape)
    return sref.forward(e, cnt, num_segments)


def _fold(w, x, cnt, num_segments):
    """agg_weighted_ref.forward(Sum) with one table row per position; an empty segment is +0.0"""
    if len(x) == 0:  # no positions: every segment is empty
        return np.zeros((num_segments, x.shape[1]), np.float32)
    return wref.forward(SUM, x, np.arange(len(x)), np.asarray(w, np.float32), cnt, num_segments, 0.0)


def out(alpha, vv, cnt, num_segments):
    """out[S, D] float32 from the engine's own alpha: +0.0, then fadd(out, fmul(alpha[p, h], vv[p])) in ascending p; an
    empty segment is +0.0"""
    return _fold(alpha, vv, cnt, num_segments)


def grad_e(soft, grad_out, vv, cnt, num_segments, heads, scale, keep=None, drop_p=0.0):
    """(grad_e float64, bound float64) [n, heads] from the engine's own float32 soft; the module docstring derives the
    bound"""
    soft = np.asarray(soft, np.float32)
    n = len(soft)
    soft = soft.reshape(n, heads).astype(np.float64)
    raw, delta = wref.backward_w(SUM, vv, np.arange(n), heads, cnt, np.asarray(grad_out, np.float32))
    if drop_p != 0:
        ds = float(gref.scale(drop_p))
        ga, delta = np.where(keep, raw * ds, 0.0), np.where(keep, delta * ds, 0.0)
    else:
        ga = raw
    sc = abs(float(np.float32(scale)))
    start = starts(cnt, n, num_segments)
    grad, bound = np.zeros_like(ga), np.zeros_like(ga)
    with np.errstate(all="ignore"):
        for s in range(num_segments):
            a, b = int(start[s]), int(start[s + 1])
            if a == b:
                continue
            al, g, dl = soft[a:b], ga[a:b], delta[a:b]
            grad[a:b] = al * (g - (al * g).sum(0)) * float(np.float32(scale))
            mag = np.abs(g) + dl
            own = np.abs(al) * (b - a + 2) * 2.0 ** -23 * (mag + (np.abs(al) * mag).sum(0))
            prop = np.abs(al) * (dl + (np.abs(al) * dl).sum(0))
            bound[a:b] = (own + prop) * sc * (1 + 2.0 ** -23) + 2.0 ** -126
    return grad, bound


def grad_q(grad_e, kk, cnt, num_segments):
    """grad_q[S, D] float32 from the engine's own grad_e: the fold of out() over grad_e and kk"""
    return _fold(grad_e, kk, cnt, num_segments)


def grad_edge(grad_e, alpha, q, grad_out, cnt, num_segments):
    """grad_edge[n, D] float32: fadd(fmul(grad_e[p, h], q[sg]), fmul(alpha[p, h], grad_out[sg])); +0.0 for a position
    nobody consumed"""
    ge, al = np.asarray(grad_e, np.float32), np.asarray(alpha, np.float32)
    q, go = np.asarray(q, np.float32), np.asarray(grad_out, np.float32)
    n, H = ge.shape
    C = q.shape[1] // H
    seg = segment_of(cnt, n, num_segments)
    used = seg < num_segments
    res = np.zeros((n, q.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        a = (np.repeat(ge[used], C, 1) * q[seg[used]]).astype(np.float32)
        b = (np.repeat(al[used], C, 1) * go[seg[used]]).astype(np.float32)
        res[used] = (a + b).astype(np.float32)
    return res


def grad_rows(w, rows, cnt, grad_out, num_rows):
    """grad_k (w = grad_e, grad_out = q) or grad_v (w = alpha, grad_out = grad_out): agg_weighted_ref.backward_x(Sum)"""
    grad_out = np.asarray(grad_out, np.float32)
    if len(rows) == 0:  # no positions: no row is named
        return np.zeros((num_rows, grad_out.shape[1]), np.float32)
    return wref.backward_x(SUM, rows, np.asarray(w, np.float32), cnt, grad_out, num_rows)


# ---- the whole function in float64, for finite differences and for the composite's tolerance --------------------

def forward64(q, k, v, rows, edge, cnt, num_segments, heads, scale, default_attr=0.0, keep_scale=None):
    """(out [S, D], soft [n, heads], alpha [n, heads]) in float64; keep_scale[n, heads] multiplies soft (the dropout mask
    times its scale), None: ones"""
    q = np.asarray(q, np.float64)
    kk = gathered(k, rows, edge, default_attr, np.float64)
    vv = gathered(v, rows, edge, default_attr, np.float64)
    n, D = kk.shape
    C = D // heads
    start = starts(cnt, n, num_segments)
    soft = np.zeros((n, heads))
    res = np.zeros((num_segments, D))
    ks = np.ones((n, heads)) if keep_scale is None else np.asarray(keep_scale, np.float64)
    for s in range(num_segments):
        a, b = int(start[s]), int(start[s + 1])
        if a == b:
            continue
        e = (kk[a:b] * q[s]).reshape(b - a, heads, C).sum(2) * float(scale)
        t = np.exp(e - e.max(0))
        soft[a:b] = t / t.sum(0)
        res[s] = (np.repeat(soft[a:b] * ks[a:b], C, 1) * vv[a:b]).sum(0)
    return res, soft, soft * ks


def backward64(q, k, v, rows, edge, cnt, num_segments, heads, scale, grad_out, default_attr=0.0, keep_scale=None):
    """(grad_q, grad_k, grad_v, grad_edge) in float64 by the contract's own formulas"""
    q, go = np.asarray(q, np.float64), np.asarray(grad_out, np.float64)
    kk = gathered(k, rows, edge, default_attr, np.float64)
    vv = gathered(v, rows, edge, default_attr, np.float64)
    _, soft, alpha = forward64(q, k, v, rows, edge, cnt, num_segments, heads, scale, default_attr, keep_scale)
    n, D = kk.shape
    C = D // heads
    ks = np.ones((n, heads)) if keep_scale is None else np.asarray(keep_scale, np.float64)
    seg = segment_of(cnt, n, num_segments)
    used = seg < num_segments
    ga = np.zeros((n, heads))
    ga[used] = (go[seg[used]] * vv[used]).reshape(-1, heads, C).sum(2) * ks[used]
    start = starts(cnt, n, num_segments)
    ge = np.zeros((n, heads))
    gq = np.zeros((num_segments, D))
    for s in range(num_segments):
        a, b = int(start[s]), int(start[s + 1])
        ge[a:b] = soft[a:b] * (ga[a:b] - (soft[a:b] * ga[a:b]).sum(0)) * float(scale)
        gq[s] = (np.repeat(ge[a:b], C, 1) * kk[a:b]).sum(0)
    gkk, gvv = np.zeros((n, D)), np.zeros((n, D))
    gkk[used] = np.repeat(ge[used], C, 1) * q[seg[used]]
    gvv[used] = np.repeat(alpha[used], C, 1) * go[seg[used]]
    gk, gv = np.zeros(np.shape(k)), np.zeros(np.shape(v))
    rows = np.asarray(rows, np.int64)
    inside = used & (rows >= 0) & (rows < len(gk))
    np.add.at(gk, rows[inside], gkk[inside])
    np.add.at(gv, rows[inside], gvv[inside])
    return gq, gk, gv, (gkk + gvv if edge is not None else None)
