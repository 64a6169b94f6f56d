"""The contracts of glx_gat_attention and glx_gat_attention_backward (include/glx.h) restated in
numpy, shared by test_gat_attention_cpu.py, test_gpu_gat_attention.py and test_gpu_gat_conv.py.

The logit is float32 step by step (numpy's float32 add and multiply are the correctly rounded IEEE operations), the
softmax and its gradient are float64 with the bounds of segment_softmax_ref, and the dropout mask is Philox4x32-10
restated here word for word."""
import numpy as np

import segment_softmax_ref as sref

starts, within_bound, same_bits = sref.starts, sref.within_bound, sref.same_bits

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) of ctr[..., 4] uint32 under key (k0, k1) -> [..., 4] uint32"""
    c = [np.asarray(ctr, np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def threshold(drop_p):
    """T: an element is kept iff its word >= T = floor(float32(drop_p) * 2^32), in double"""
    return int(np.floor(float(np.float32(drop_p)) * 4294967296.0))


def scale(drop_p):
    """1.0f / (1.0f - drop_p): one float32 subtraction and one float32 division"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(drop_p))


def keep_mask(n, heads, drop_p, seed, call):
    """keep[n, heads]: element i = p * heads + h draws word i & 3 of block i >> 2, counter (block, 0, call lo, call hi),
    key (seed lo, seed hi)"""
    count = n * heads
    blocks = (count + 3) // 4
    ctr = np.zeros((blocks, 4), np.uint32)
    ctr[:, 0] = np.arange(blocks, dtype=np.uint32)
    ctr[:, 2], ctr[:, 3] = call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:count]
    return (words.astype(np.uint64) >= np.uint64(threshold(drop_p))).reshape(n, heads)


def drop(x, keep, drop_p):
    """keep ? fmul(x, scale) : +0.0f, float32; drop_p == 0: x itself"""
    x = np.asarray(x, np.float32)
    if drop_p == 0:
        return x.copy()
    with np.errstate(all="ignore"):
        return np.where(keep, x * scale(drop_p), np.float32(0.0)).astype(np.float32)


def segment_of(cnt, n, num_segments):
    """seg[n]: the segment that consumed each position, num_segments for a position nobody consumed"""
    start = starts(cnt, n, num_segments)
    seg = np.full(n, num_segments, np.int64)
    for sg in range(num_segments):
        seg[int(start[sg]):int(start[sg + 1])] = sg
    return seg


def logits(s, t, rows, cnt, num_segments, negative_slope=0.2, default_attr=0.0):
    """(pre, e) float32 [n, heads]: pre = fadd(s[segment], t[rows] or default_attr), e = pre > 0 ? pre :
    fmul(pre, negative_slope); a position nobody consumed is 0 in both"""
    s = np.asarray(s, np.float32).reshape(num_segments, -1)
    t = np.asarray(t, np.float32).reshape(len(t), -1)
    rows = np.asarray(rows, np.int64)
    n, H = len(rows), s.shape[1]
    seg = segment_of(cnt, n, num_segments)
    used = seg < num_segments
    pre = np.zeros((n, H), np.float32)
    with np.errstate(all="ignore"):
        inside = (rows >= 0) & (rows < len(t))
        tv = np.full((n, H), np.float32(default_attr), np.float32)
        tv[inside] = t[rows[inside]]
        pre[used] = s[seg[used]] + tv[used]
        e = np.where(pre > 0, pre, pre * np.float32(negative_slope)).astype(np.float32)
    e[~used] = 0
    return pre, e


def forward(s, t, rows, cnt, num_segments, negative_slope=0.2, default_attr=0.0):
    """(soft float64, bound float64, pre float32), all [n, heads]: segment_softmax_ref.forward of the logits"""
    pre, e = logits(s, t, rows, cnt, num_segments, negative_slope, default_attr)
    soft, bound = sref.forward(e, cnt, num_segments)
    return soft, bound, pre


def backward(soft, grad_alpha, pre, cnt, num_segments, negative_slope=0.2, keep=None, drop_p=0.0):
    """(grad_e float64, bound float64) from the engine's own float32 `soft`: ga = drop(grad_alpha) in float32,
    d = segment_softmax_ref.backward(soft, ga), grad_e = pre > 0 ? d : d * negative_slope.  The bound is the softmax
    gradient's, scaled like the value: its (k + 2) * 2^-23 has room for the one more rounding of the last multiply
    (the softmax gradient itself needs (k + 2) * 2^-24 to first order)."""
    soft = np.asarray(soft, np.float32)
    ga = drop(np.asarray(grad_alpha, np.float32).reshape(soft.shape), keep, drop_p)
    d, bound = sref.backward(soft, ga, cnt, num_segments)
    with np.errstate(all="ignore"):
        mult = np.where(np.asarray(pre).reshape(soft.shape) > 0, 1.0, float(np.float32(negative_slope)))
        return d * mult, bound * mult + 2.0 ** -126


def grad_s(grad_e, cnt, num_segments):
    """(sum float64, bound float64) [num_segments, heads] of the engine's own grad_e: any order of a k-term float32
    sum lies within k * 2^-24 * sum |terms| of the exact sum, to first order; an empty segment is 0 with bound 0"""
    g = np.asarray(grad_e, np.float32)
    g = g.reshape(len(g), -1).astype(np.float64)
    start = starts(cnt, len(g), num_segments)
    out, bound = np.zeros((num_segments, g.shape[1])), np.zeros((num_segments, g.shape[1]))
    for sg in range(num_segments):
        a, b = int(start[sg]), int(start[sg + 1])
        out[sg] = g[a:b].sum(0)
        bound[sg] = (b - a) * 2.0 ** -24 * np.abs(g[a:b]).sum(0)
    return out, bound


def grad_t(grad_e, rows, cnt, num_segments, num_rows):
    """grad_t[num_rows, heads] float32: +0.0 plus grad_e[p] over the consumed, in-range positions with rows[p] == r in
    ascending p, one float32 add each"""
    g = np.asarray(grad_e, np.float32)
    g = g.reshape(len(g), -1)
    out = np.zeros((num_rows, g.shape[1]), np.float32)
    seg = segment_of(cnt, len(g), num_segments)
    with np.errstate(all="ignore"):
        for p in np.flatnonzero(seg < num_segments):
            r = int(rows[p])
            if 0 <= r < num_rows:
                out[r] = out[r] + g[p]
    return out
