"""glx_gat_attention and glx_gat_attention_backward on the GPU against the numpy restatement of their contract
(gat_attention_ref.py): every output starts as a NaN canary, every call is made twice and must repeat its bits, the
softmax and its gradient lie inside the stated bounds around the float64 values, and the exact rules, the dropout mask
and the row gradient hold bit for bit."""
import numpy as np
import pytest

import gat_attention_ref as gref
import glx
from test_gpu_segment_softmax import LENGTHS, _bits, _cuda

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
HEADS = [1, 2, 3, 4, 8]  # FLAT (a power of two) and head by head
M = 257                  # rows of t
INF = float("inf")


def _canary(shape, host, offset=False):
    a = np.full(shape, NAN, np.float32)
    return a if host else _cuda(a, offset)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _dev(host, offset, *arrays):
    if host:
        return arrays
    return tuple(_cuda(a, offset and a is not None and a.dtype == np.float32) for a in arrays)


def gpu_forward(s, t, rows, cnt, host=False, offset=False, want_soft=True, **kw):
    """(alpha, soft) of the first of two calls into NaN canaries; the second call must repeat the bits"""
    ds, dt, drows, dcnt = _dev(host, offset, s, t, rows, cnt)
    shape = (len(rows), s.shape[1])
    res = []
    for _ in range(2):
        out = _canary(shape, host, offset)
        soft_out = _canary(shape, host, offset) if want_soft else None
        alpha, soft = glx.gat_attention(ds, dt, drows, cnt=dcnt, out=out, soft_out=soft_out, want_soft=want_soft, **kw)
        res.append((_np(alpha), None if soft is None else _np(soft)))
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])), "alpha differs between two calls"
    if want_soft:
        assert np.array_equal(_bits(res[0][1]), _bits(res[1][1])), "soft differs between two calls"
    return res[0]


def gpu_backward(soft, g, s, t, rows, cnt, host=False, offset=False, want_s=True, want_t=True, **kw):
    """(grad_e, grad_s, grad_t) of the first of two calls into NaN canaries"""
    dsoft, dg, ds, dt, drows, dcnt = _dev(host, offset, soft, g, s, t, rows, cnt)
    H = s.shape[1]
    res = []
    for _ in range(2):
        out = _canary((len(rows), H), host, offset)
        out_s = _canary(s.shape, host, offset) if want_s else None
        out_t = _canary(t.shape, host, offset) if want_t else None
        got = glx.gat_attention_backward(dsoft, dg, ds, dt, drows, cnt=dcnt, out=out, out_s=out_s, out_t=out_t,
                                         want_s=want_s, want_t=want_t, **kw)
        res.append([None if x is None else _np(x) for x in got])
    for a, b in zip(*res):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b)), "a gradient differs between two calls"
    return res[0]


def _unconsumed(cnt, n, S):
    start = gref.starts(cnt, n, S)
    mask = np.ones(n, bool)
    mask[:int(start[-1])] = False
    return mask


def check(s, t, rows, cnt, g, host=False, offset=False, slope=0.2, default_attr=0.0, drop_p=0.0, seed=0, call=0):
    """one request through both entry points and the restatement -> (soft, alpha, grad_e, grad_s, grad_t)"""
    S, n, H = len(s), len(rows), s.shape[1]
    kw = dict(negative_slope=slope, default_attr=default_attr, drop_p=drop_p, seed=seed, call=call)
    alpha, soft = gpu_forward(s, t, rows, cnt, host, offset, **kw)
    want, bound, pre = gref.forward(s, t, rows, cnt, S, slope, default_attr)
    assert np.array_equal(np.isnan(soft), np.isnan(want)), "an element of soft was not written, or a NaN is misplaced"
    assert gref.within_bound(soft, want, bound)
    rest = _unconsumed(cnt, n, S)
    zeros = np.zeros((int(rest.sum()), H), np.float32)
    assert gref.same_bits(soft[rest], zeros) and gref.same_bits(alpha[rest], zeros)  # +0.0, not -0.0
    keep = gref.keep_mask(n, H, drop_p, seed, call) if drop_p else None
    assert gref.same_bits(alpha, gref.drop(soft, keep, drop_p)), "alpha is not the dropout of the engine's own soft"
    grad_e, grad_s, grad_t = gpu_backward(soft, g, s, t, rows, cnt, host, offset, **kw)
    want, bound = gref.backward(soft, g, pre, cnt, S, slope, keep, drop_p)
    assert np.array_equal(np.isnan(grad_e), np.isnan(want)), "an element of grad_e was not written"
    assert gref.within_bound(grad_e, want, bound)
    assert gref.same_bits(grad_e[rest], zeros)
    want, bound = gref.grad_s(grad_e, cnt, S)
    assert grad_s.shape == s.shape and gref.within_bound(grad_s, want, bound)
    empty = np.diff(gref.starts(cnt, n, S)) == 0
    assert gref.same_bits(grad_s[empty], np.zeros((int(empty.sum()), H), np.float32))
    if host:
        want_t = glx.aggregate_backward(glx.SUM, rows, None, grad_e, len(t))
    else:
        want_t = glx.aggregate_backward(glx.SUM, _cuda(rows), None, _cuda(grad_e), len(t)).cpu().numpy()
    assert grad_t.shape == t.shape and gref.same_bits(grad_t, want_t)
    return soft, alpha, grad_e, grad_s, grad_t


def _tables(rng, S, n, heads, num_rows=M):
    s = (rng.standard_normal((S, heads)) * 2).astype(np.float32)
    t = (rng.standard_normal((num_rows, heads)) * 2).astype(np.float32)
    rows = rng.integers(0, num_rows, n).astype(np.int64)
    g = rng.standard_normal((n, heads)).astype(np.float32)
    return s, t, rows, g


def _lengths_request(heads, pad, cut, seed):
    """test_gpu_segment_softmax's request: LENGTHS with a leading and a trailing empty segment, a negative count and
    `pad` more empty segments (group width 64 without them, 8 with 10,000).  cut False: 5 positions behind sum(cnt)
    that nobody consumes; True: the counts promise 20 positions more than the request has."""
    rng = np.random.default_rng(seed)
    body = LENGTHS[1:]
    rng.shuffle(body)
    cnt = [0] * (1 + pad // 2) + body[:9] + [-4] + body[9:] + ([33, 7] if cut else []) + [0] * (1 + pad - pad // 2)
    cnt = np.array(cnt, np.int32)
    n = int(np.maximum(cnt, 0).sum()) + (-20 if cut else 5)
    return _tables(rng, len(cnt), n, heads) + (cnt,)


@pytest.mark.parametrize("pad", [0, 10000])
@pytest.mark.parametrize("heads", HEADS)
def test_segment_lengths_at_every_group_and_chunk_boundary(heads, pad):
    s, t, rows, g, cnt = _lengths_request(heads, pad, cut=False, seed=heads + pad)
    check(s, t, rows, cnt, g)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_counts_that_promise_more_than_the_request_has(heads, host):
    s, t, rows, g, cnt = _lengths_request(heads, 0, cut=True, seed=50 + heads)
    check(s, t, rows, cnt, g, host=host, drop_p=0.5 if host else 0.0, seed=3, call=4)
    assert gref.starts(cnt, len(rows), len(cnt))[-1] == len(rows)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("fanout", [1, 10, 25])
def test_implied_layout(fanout, heads, host):
    """cnt=None; 37 segments are two workgroups at 8 lanes per segment"""
    S = 37
    rng = np.random.default_rng(fanout * 10 + heads)
    s, t, rows, g = _tables(rng, S, S * fanout, heads)
    soft, _, _, _, _ = check(s, t, rows, None, g, host=host)
    if fanout == 1:
        assert gref.same_bits(soft, np.ones((S, heads), np.float32))  # k = 1: exactly 1.0


@pytest.mark.parametrize("heads", HEADS)
def test_pointers_off_16_byte_alignment(heads):
    s, t, rows, g, cnt = _lengths_request(heads, 0, cut=False, seed=90 + heads)
    off = check(s, t, rows, cnt, g, offset=True, drop_p=0.1, seed=5, call=6)
    on = check(s, t, rows, cnt, g, drop_p=0.1, seed=5, call=6)
    for a, b in zip(off, on):
        assert np.array_equal(_bits(a), _bits(b))  # the same bits wherever the buffers start


VALUE_CNT = np.array([1, 7, 33, 70, 0, 300, 1500], np.int32)  # a group's registers, its loop, and the workgroup's walk


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_one_position_is_one_and_equal_logits_are_one_over_k(heads):
    ks = [1, 3, 8, 10, 64, 1500]
    cnt = np.array(ks, np.int32)
    rng = np.random.default_rng(heads)
    s, t, rows, g = _tables(rng, len(ks), sum(ks), heads)
    t[:] = t[0]  # every neighbour has the same half: the logits of a (segment, head) are equal
    soft, _, _, _, _ = check(s, t, rows, cnt, g)
    want = np.concatenate([np.full((k, heads), np.float32(1) / np.float32(k), np.float32) for k in ks])
    assert gref.same_bits(soft, want) and gref.same_bits(soft[:1], np.ones((1, heads), np.float32))


@pytest.mark.parametrize("default_attr", [0.0, -INF], ids=["zero", "minus_inf"])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_rows_outside_the_table_read_default_attr(heads, default_attr):
    """default_attr = -inf is the mask: the position is exactly +0.0 and neither it nor any row of t gets a gradient
    from it; default_attr = 0 makes it a neighbour whose half of the logit is 0"""
    rng = np.random.default_rng(21 + heads)
    n = int(VALUE_CNT.sum())
    s, t, rows, g = _tables(rng, len(VALUE_CNT), n, heads)
    start = gref.starts(VALUE_CNT, n, len(VALUE_CNT))
    out = [int(start[i]) + (int(start[i + 1]) - int(start[i])) // 2 for i in (1, 2, 3, 5, 6)]
    rows[out] = [-1, M, -2 ** 40, 2 ** 40, -1]
    soft, alpha, grad_e, grad_s, grad_t = check(s, t, rows, VALUE_CNT, g, default_attr=default_attr)
    assert np.isfinite(soft).all() and np.isfinite(grad_e).all()
    if default_attr == 0.0:
        assert (soft[out] > 0).all()
    else:
        assert gref.same_bits(soft[out], np.zeros((len(out), heads), np.float32))
        assert not grad_e[out].any()  # +0 * finite: a zero of either sign
    assert gref.same_bits(grad_t, gref.grad_t(grad_e, rows, VALUE_CNT, len(VALUE_CNT), M))  # and t gets nothing from them


@pytest.mark.parametrize("length", [70, 1500])
@pytest.mark.parametrize("where", ["s", "t"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_nan_or_infinite_half_takes_its_column_and_nothing_else(bad, where, length):
    heads = 2
    cnt = np.array([9, length, 9], np.int32)
    n = 18 + length
    rng = np.random.default_rng(length)
    s, t, rows, g = _tables(rng, 3, n, heads)
    rows[:] = np.arange(n) % (M - 1)           # row M - 1 is named by one position only
    clean, _, _, _, _ = check(s, t, rows, cnt, g)
    if where == "s":
        s[1, 0] = bad
    else:
        rows[9 + length // 2] = M - 1
        t[M - 1, 0] = bad
    soft, _, grad_e, _, _ = check(s, t, rows, cnt, g)
    assert np.isnan(soft[9:9 + length, 0]).all() and np.isnan(grad_e[9:9 + length, 0]).all()
    keep = np.ones(soft.shape, bool)
    keep[9:9 + length] = False
    assert np.array_equal(_bits(soft[keep]), _bits(clean[keep]))  # the neighbours: untouched
    assert np.isfinite(soft[:, 1]).all()                          # the other head too


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("heads", [1, 3])
def test_negative_slope_of_zero_and_of_one(heads, slope):
    rng = np.random.default_rng(int(slope) + heads)
    n = int(VALUE_CNT.sum())
    s, t, rows, g = _tables(rng, len(VALUE_CNT), n, heads)
    soft, _, grad_e, _, _ = check(s, t, rows, VALUE_CNT, g, slope=slope)
    pre, e = gref.logits(s, t, rows, VALUE_CNT, len(VALUE_CNT), slope)
    if slope == 0.0:
        assert (pre <= 0).any() and not grad_e[pre <= 0].any()  # relu: no gradient through a negative logit
    else:  # the identity: the softmax of pre itself
        assert gref.same_bits(e, pre) and gref.within_bound(soft, *gref.sref.forward(pre, VALUE_CNT, len(VALUE_CNT)))


@pytest.mark.parametrize("heads", [1, 3, 4])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_is_the_restated_one(p, heads):
    s, t, rows, g, cnt = _lengths_request(heads, 0, cut=False, seed=int(p * 10) + heads)
    seed, call = 2 ** 40 + 12345, 2 ** 33 + 7  # both halves of both words are used
    soft, alpha, _, _, _ = check(s, t, rows, cnt, g, drop_p=p, seed=seed, call=call)
    keep = gref.keep_mask(len(rows), heads, p, seed, call)
    used = ~_unconsumed(cnt, len(rows), len(cnt))
    assert 0 < (alpha[used] == 0).sum() and gref.same_bits(alpha[~keep], np.zeros_like(alpha[~keep]))
    assert gref.same_bits(alpha[keep], (soft[keep] * gref.scale(p)).astype(np.float32))
    kw = dict(negative_slope=0.2, drop_p=p, seed=seed)
    other, soft2 = gpu_forward(s, t, rows, cnt, call=call + 1, **kw)
    assert np.array_equal(_bits(soft2), _bits(soft))  # the softmax does not depend on the mask
    assert not np.array_equal(other == 0, alpha == 0), "another call must draw another mask"
    assert gref.same_bits(other, gref.drop(soft, gref.keep_mask(len(rows), heads, p, seed, call + 1), p))
    # no dropout and no second output: alpha is soft
    plain, none = gpu_forward(s, t, rows, cnt, want_soft=False, negative_slope=0.2)
    assert none is None and np.array_equal(_bits(plain), _bits(soft))


@pytest.mark.parametrize("num_rows", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_row_gradient_for_narrow_and_wide_tables(heads, num_rows):
    rng = np.random.default_rng(num_rows + heads)
    cnt = np.array([3, 0, 40, 1, 200, 17], np.int32)
    n = int(cnt.sum()) + 2
    s, t, rows, g = _tables(rng, len(cnt), n, heads, num_rows)
    _, _, grad_e, _, grad_t = check(s, t, rows, cnt, g, drop_p=0.5, seed=9, call=1)
    assert gref.same_bits(grad_t, gref.grad_t(grad_e, rows, cnt, len(cnt), num_rows))


@pytest.mark.parametrize("heads", [1, 4])
def test_a_hub_row_and_rows_nobody_names(heads):
    rng = np.random.default_rng(heads)
    cnt = np.array([1500, 30, 1700, 5], np.int32)
    n = int(cnt.sum())
    s, t, rows, g = _tables(rng, len(cnt), n, heads)
    rows[:] = rng.integers(100, 120, n)
    rows[rng.choice(n, 3000, replace=False)] = 7  # the hub: 3,000 positions
    _, _, grad_e, _, grad_t = check(s, t, rows, cnt, g)
    assert (rows == 7).sum() == 3000 and grad_t[7].all()
    named = np.zeros(M, bool)
    named[np.unique(rows)] = True
    assert gref.same_bits(grad_t[~named], np.zeros((int((~named).sum()), heads), np.float32))
    assert gref.same_bits(grad_t, gref.grad_t(grad_e, rows, cnt, len(cnt), M))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_gradients_that_are_not_asked_for(host):
    rng = np.random.default_rng(4)
    cnt = np.array([3, 0, 40, 1, 1200], np.int32)
    s, t, rows, g = _tables(rng, len(cnt), int(cnt.sum()), 2)
    soft, _, grad_e, grad_s, grad_t = check(s, t, rows, cnt, g, host=host)
    for want_s, want_t in ((False, True), (True, False), (False, False)):
        ge, gs, gt = gpu_backward(soft, g, s, t, rows, cnt, host, want_s=want_s, want_t=want_t, negative_slope=0.2)
        assert np.array_equal(_bits(ge), _bits(grad_e))
        assert (gs is None) == (not want_s) and (gt is None) == (not want_t)
        assert gs is None or np.array_equal(_bits(gs), _bits(grad_s))
        assert gt is None or np.array_equal(_bits(gt), _bits(grad_t))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_no_segments_and_no_positions(host):
    rng = np.random.default_rng(5)
    s, t, rows, g = _tables(rng, 3, 6, 2, num_rows=5)
    zeros = np.zeros((6, 2), np.float32)
    # no segments: nothing is consumed
    s0 = np.zeros((0, 2), np.float32)
    alpha, soft = gpu_forward(s0, t, rows, None, host, negative_slope=0.2)
    assert gref.same_bits(alpha, zeros) and gref.same_bits(soft, zeros)
    ge, gs, gt = gpu_backward(zeros, g, s0, t, rows, None, host, negative_slope=0.2)
    assert gref.same_bits(ge, zeros) and gs.shape == (0, 2) and gref.same_bits(gt, np.zeros_like(t))
    # counts that consume nothing
    cnt = np.array([0, -1, 0], np.int32)
    alpha, soft = gpu_forward(s, t, rows, cnt, host, negative_slope=0.2, drop_p=0.5, seed=1)
    assert gref.same_bits(alpha, zeros) and gref.same_bits(soft, zeros)
    ge, gs, gt = gpu_backward(zeros, g, s, t, rows, cnt, host, negative_slope=0.2)
    assert gref.same_bits(ge, zeros) and gref.same_bits(gs, np.zeros_like(s)) and gref.same_bits(gt, np.zeros_like(t))
    # no positions: the segments are empty and every row's gradient is zeros
    none = np.zeros(0, np.int64)
    cnt = np.array([0, 0, 0], np.int32)
    alpha, soft = gpu_forward(s, t, none, cnt, host, negative_slope=0.2)
    assert alpha.shape == (0, 2) and soft.shape == (0, 2)
    ge, gs, gt = gpu_backward(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), s, t, none, cnt, host,
                              negative_slope=0.2)
    assert ge.shape == (0, 2) and gref.same_bits(gs, np.zeros_like(s)) and gref.same_bits(gt, np.zeros_like(t))
