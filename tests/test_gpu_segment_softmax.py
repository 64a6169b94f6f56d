"""glx_segment_softmax and glx_segment_softmax_backward on the GPU against the numpy restatement of their contracts
(segment_softmax_ref.py): every output starts as a NaN canary, every call is made twice and must repeat its bits, the
results lie inside the stated bounds around the float64 values, and the exact rules hold bit for bit."""
import numpy as np
import pytest

import agg_weighted_ref as wref
import glx
import segment_softmax_ref as sref

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
HEADS = [1, 2, 3, 4, 6, 8]

# The issue's lengths, plus the +-1 neighbours of this kernel's own boundaries that they miss.  A lane group of G = 8, 16,
# 32 or 64 lanes keeps 4 items per lane in registers (4 G = 32, 64, 128, 256 items; an item is one logit when heads is a
# power of two, one position otherwise) and a segment of more than 1024 items goes to the whole workgroup: 127 .. 129
# for G = 32, and 128 | 129, 512 | 513, 1024 | 1025 for the 1024-item threshold at heads 8, 2 and 1 (3, 6) -- heads 4
# has it at 256 | 257.  5,000 positions are 20 .. 157 rounds of the 256-thread walk.
LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5000,
           127, 128, 129, 512, 513, 1024, 1025]


def _cuda(a, offset=False):
    """a CUDA copy of `a`; offset: 4 bytes into its buffer, so that it is not 16-byte aligned"""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a).cuda()
    assert a.dtype == np.float32
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_forward(e, cnt, S, host=False, offset=False):
    """alpha of two calls into NaN canaries"""
    if host:
        outs = [np.full(e.shape, NAN, np.float32) for _ in range(2)]
        for out in outs:
            glx.segment_softmax(e, S, cnt=cnt, out=out)
        return outs
    de, dcnt = _cuda(e, offset), _cuda(cnt)
    outs = [_cuda(np.full(e.shape, NAN, np.float32), offset) for _ in range(2)]
    for out in outs:
        glx.segment_softmax(de, S, cnt=dcnt, out=out)
    return [o.cpu().numpy() for o in outs]


def gpu_backward(alpha, g, cnt, S, host=False, offset=False):
    if host:
        outs = [np.full(alpha.shape, NAN, np.float32) for _ in range(2)]
        for out in outs:
            glx.segment_softmax_backward(alpha, g, cnt, S, out=out)
        return outs
    da, dg, dcnt = _cuda(alpha, offset), _cuda(g, offset), _cuda(cnt)
    outs = [_cuda(np.full(alpha.shape, NAN, np.float32), offset) for _ in range(2)]
    for out in outs:
        glx.segment_softmax_backward(da, dg, dcnt, S, out=out)
    return [o.cpu().numpy() for o in outs]


def _unconsumed(cnt, n, S):
    start = sref.starts(cnt, n, S)
    mask = np.ones(n, bool)
    mask[:int(start[-1])] = False
    return mask


def check(e, cnt, S, g, host=False, offset=False):
    """one request through both entry points and the restatement -> (alpha, grad_e)"""
    alpha, again = gpu_forward(e, cnt, S, host, offset)
    want, bound = sref.forward(e, cnt, S)
    assert np.array_equal(np.isnan(alpha), np.isnan(want)), "an element of alpha was not written, or a NaN is misplaced"
    assert np.array_equal(_bits(alpha), _bits(again)), "alpha differs between two calls"
    assert sref.within_bound(alpha, want, bound)
    rest = _unconsumed(cnt, len(e), S)
    assert sref.same_bits(alpha[rest], np.zeros_like(alpha[rest]))  # +0.0, not -0.0
    grad, again = gpu_backward(alpha, g, cnt, S, host, offset)
    want, bound = sref.backward(alpha, g, cnt, S)
    assert np.array_equal(np.isnan(grad), np.isnan(want)), "an element of grad_e was not written"
    assert np.array_equal(_bits(grad), _bits(again)), "grad_e differs between two calls"
    assert sref.within_bound(grad, want, bound)
    assert sref.same_bits(grad[rest], np.zeros_like(grad[rest]))
    return alpha, grad


def _const_per_segment(cnt, n, S, heads, rng):
    """a grad_alpha that is constant over each (segment, head): the exact gradient is 0"""
    start = sref.starts(cnt, n, S)
    g = rng.standard_normal((n, heads)).astype(np.float32)
    for s in range(S):
        g[int(start[s]):int(start[s + 1])] = rng.standard_normal(heads).astype(np.float32)
    return g


def _lengths_request(heads, pad, cut, seed):
    """LENGTHS with a leading and a trailing empty segment, a negative count and `pad` more empty segments (they lower
    the mean segment length, from which the launch picks its group width: 64 lanes without them, 8 with 10,000).
    cut False: 5 positions behind sum(cnt) that nobody consumes; True: the counts promise 20 positions more than the
    request has, which cuts the segment of 33 to 20 and the 7 behind it to nothing."""
    rng = np.random.default_rng(seed)
    body = LENGTHS[1:]
    rng.shuffle(body)
    cnt = [0] * (1 + pad // 2) + body[:9] + [-4] + body[9:] + ([33, 7] if cut else []) + [0] * (1 + pad - pad // 2)
    cnt = np.array(cnt, np.int32)
    n = int(np.maximum(cnt, 0).sum()) + (-20 if cut else 5)
    e = rng.standard_normal((n, heads)).astype(np.float32) * np.float32(3)
    g = rng.standard_normal((n, heads)).astype(np.float32)
    return e, cnt, g


@pytest.mark.parametrize("pad", [0, 300, 600, 1200, 10000])
@pytest.mark.parametrize("heads", HEADS)
def test_segment_lengths_at_every_group_and_chunk_boundary(heads, pad):
    e, cnt, g = _lengths_request(heads, pad, cut=False, seed=heads + pad)
    check(e, cnt, len(cnt), g)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("heads", HEADS)
def test_counts_that_promise_more_than_the_request_has(heads, host):
    e, cnt, g = _lengths_request(heads, 0, cut=True, seed=50 + heads)
    alpha, _ = check(e, cnt, len(cnt), g, host=host)
    start = sref.starts(cnt, len(e), len(cnt))
    assert start[-1] == len(e) and np.count_nonzero(np.diff(start)) == len(LENGTHS)  # 33 is 20 now, 7 is nothing
    assert np.diff(start)[np.flatnonzero(np.diff(start))[-1]] == 20


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_one_dimensional_logits_and_constant_gradients(heads):
    """grad_alpha constant over each (segment, head): the exact gradient is 0 and the bound must hold around it"""
    e, cnt, _ = _lengths_request(heads, 0, cut=False, seed=7)
    rng = np.random.default_rng(8)
    g = _const_per_segment(cnt, len(e), len(cnt), heads, rng)
    check(e, cnt, len(cnt), g)
    if heads == 1:  # e[n] instead of e[n, 1]
        a1, _ = check(e[:, 0].copy(), cnt, len(cnt), g[:, 0].copy())
        a2, _ = gpu_forward(e, cnt, len(cnt))
        assert a1.shape == (len(e),) and np.array_equal(_bits(a1), _bits(a2[:, 0]))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("fanout", [1, 10, 25])
def test_implied_layout(fanout, heads, host):
    """cnt=None; 37 segments (two workgroups at 8 lanes per segment); n = 37 fanout + 3 leaves a remainder that must
    read +0.0 (fan-out 1: a remainder needs n < 2 S, so 37 segments of 1 and 3 behind them is one case of it)"""
    S = 37
    n = S * fanout + 3
    rng = np.random.default_rng(fanout * 10 + heads)
    e = rng.standard_normal((n, heads)).astype(np.float32)
    g = rng.standard_normal((n, heads)).astype(np.float32)
    alpha, grad = check(e, None, S, g, host=host)
    assert sref.same_bits(alpha[-3:], np.zeros((3, heads), np.float32))
    if fanout == 1:
        assert sref.same_bits(alpha[:S], np.ones((S, heads), np.float32))  # k = 1: exactly 1.0
    # without a remainder too
    check(e[:S * fanout], None, S, g[:S * fanout], host=host)


@pytest.mark.parametrize("heads", HEADS)
def test_pointers_off_16_byte_alignment(heads):
    e, cnt, g = _lengths_request(heads, 0, cut=False, seed=90 + heads)
    a_off, g_off = check(e, cnt, len(cnt), g, offset=True)
    a, _ = gpu_forward(e, cnt, len(cnt))
    assert np.array_equal(_bits(a_off), _bits(a))  # the same bits wherever the buffers start
    rng = np.random.default_rng(heads)
    e = rng.standard_normal((40 * 10, heads)).astype(np.float32)
    check(e, None, 40, e[::-1].copy(), offset=True)


VALUE_CNT = np.array([1, 7, 33, 70, 0, 300, 1500], np.int32)  # a group's registers, its loop, and the workgroup's walk


@pytest.mark.parametrize("heads", [1, 3, 4])
@pytest.mark.parametrize("scale", [0.5, 30.0, 120.0])
def test_logit_scales_up_to_underflow_of_the_tail(scale, heads):
    rng = np.random.default_rng(int(scale) + heads)
    n = int(VALUE_CNT.sum())
    e = (rng.standard_normal((n, heads)) * scale).astype(np.float32)
    g = rng.standard_normal((n, heads)).astype(np.float32)
    alpha, _ = check(e, VALUE_CNT, len(VALUE_CNT), g)
    if scale == 120.0:
        assert (alpha == 0).any()  # exp underflowed somewhere: the 2^-126 of the bound was needed


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_equal_logits_are_exactly_one_over_k(heads):
    ks = [1, 3, 8, 10, 64, 1500]
    cnt = np.array(ks, np.int32)
    rng = np.random.default_rng(heads)
    e = np.concatenate([np.tile(rng.standard_normal(heads).astype(np.float32) * 20, (k, 1)) for k in ks])
    alpha, _ = check(e, cnt, len(ks), rng.standard_normal(e.shape).astype(np.float32))
    want = np.concatenate([np.full((k, heads), np.float32(1) / np.float32(k), np.float32) for k in ks])
    assert sref.same_bits(alpha, want)
    # -0.0 and +0.0 mixed are equal logits
    z = np.where(rng.integers(0, 2, e.shape) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    alpha, _ = check(z, cnt, len(ks), z)
    assert sref.same_bits(alpha, want)


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_an_exact_shift_changes_no_bit(heads):
    rng = np.random.default_rng(11 + heads)
    n = int(VALUE_CNT.sum())
    e = (rng.integers(-2048, 2048, (n, heads)) / 1024.0).astype(np.float32)  # multiples of 2^-10 in [-2, 2)
    shifted = e + np.float32(8.0)
    assert np.array_equal(shifted.astype(np.float64), e.astype(np.float64) + 8.0)  # exact in float32
    a, _ = check(e, VALUE_CNT, len(VALUE_CNT), e)
    b, _ = check(shifted, VALUE_CNT, len(VALUE_CNT), e)
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_minus_infinity_masks_a_position_exactly(heads):
    rng = np.random.default_rng(21 + heads)
    n = int(VALUE_CNT.sum())
    e = rng.standard_normal((n, heads)).astype(np.float32)
    start = sref.starts(VALUE_CNT, n, len(VALUE_CNT))
    masked = [int(start[s]) + (int(start[s + 1]) - int(start[s])) // 2 for s in (1, 2, 3, 5, 6)]
    e[masked, 0] = -np.inf
    e[masked[1] + 1, heads - 1] = -np.inf
    g = rng.standard_normal((n, heads)).astype(np.float32)
    alpha, grad = check(e, VALUE_CNT, len(VALUE_CNT), g)
    assert sref.same_bits(alpha[masked, 0], np.zeros(len(masked), np.float32))
    assert np.isfinite(alpha).all() and np.isfinite(grad).all()
    assert not grad[masked, 0].any()  # +0 * finite: a zero of either sign


@pytest.mark.parametrize("length", [70, 1500])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_nan_or_infinite_logit_takes_its_column_and_nothing_else(bad, where, length):
    """fmaxf drops a NaN: the kernel has to carry it to every position of the (segment, head)"""
    heads = 2
    cnt = np.array([9, length, 9], np.int32)
    rng = np.random.default_rng(length)
    e = rng.standard_normal((9 + length + 9, heads)).astype(np.float32)
    g = rng.standard_normal(e.shape).astype(np.float32)
    clean, _ = check(e, cnt, 3, g)
    at = 9 + {"first": 0, "middle": length // 2, "last": length - 1}[where]
    e[at, 0] = bad
    alpha, grad = check(e, cnt, 3, g)
    assert np.isnan(alpha[9:9 + length, 0]).all() and np.isnan(grad[9:9 + length, 0]).all()
    keep = np.ones(e.shape, bool)
    keep[9:9 + length, 0] = False
    assert np.array_equal(_bits(alpha[keep]), _bits(clean[keep]))  # the other head and the neighbours: untouched


@pytest.mark.parametrize("heads", [1, 3])
def test_a_segment_of_minus_infinity_only_is_nan(heads):
    cnt = np.array([4, 70, 1, 1500, 4], np.int32)
    rng = np.random.default_rng(3)
    e = rng.standard_normal((int(cnt.sum()), heads)).astype(np.float32)
    e[4:74, 0] = -np.inf
    e[74, heads - 1] = -np.inf  # k = 1
    e[75:1575, 0] = -np.inf
    alpha, _ = check(e, cnt, 5, rng.standard_normal(e.shape).astype(np.float32))
    assert np.isnan(alpha[4:74, 0]).all() and np.isnan(alpha[74, heads - 1]) and np.isnan(alpha[75:1575, 0]).all()
    assert np.isfinite(alpha[:4]).all() and np.isfinite(alpha[1575:]).all()


def test_no_segments_and_no_positions():
    e = np.ones((6, 2), np.float32)
    for host in (False, True):
        (alpha, _), (grad, _) = gpu_forward(e, None, 0, host), gpu_backward(e, e, None, 0, host)
        assert sref.same_bits(alpha, np.zeros_like(e)) and sref.same_bits(grad, np.zeros_like(e))  # nothing consumed
        cnt = np.array([0, -1, 0], np.int32)
        (alpha, _), (grad, _) = gpu_forward(e, cnt, 3, host), gpu_backward(e, e, cnt, 3, host)
        assert sref.same_bits(alpha, np.zeros_like(e)) and sref.same_bits(grad, np.zeros_like(e))
        empty = np.zeros((0, 2), np.float32)
        assert gpu_forward(empty, np.array([0], np.int32), 1, host)[0].shape == (0, 2)


@pytest.mark.parametrize("heads", [1, 2])
def test_composition_with_the_weighted_reduce_agrees_on_the_layout(heads):
    """segment_softmax, then glx.aggregate_weighted with the same cnt, fed the GPU's own alpha: the restatement of the
    weighted sum bit for bit -- both entry points cut the request into the same segments"""
    cnt = np.array([0, 3, 17, -2, 70, 0, 130, 9], np.int32)
    n, num_rows, D = int(np.maximum(cnt, 0).sum()) - 4, 11, 8  # the last segment is cut from 9 to 5
    rng = np.random.default_rng(heads)
    X = rng.standard_normal((num_rows, D)).astype(np.float32)
    rows = rng.integers(0, num_rows, n).astype(np.int64)
    e = rng.standard_normal((n, heads)).astype(np.float32)
    alpha = glx.segment_softmax(_cuda(e), len(cnt), cnt=_cuda(cnt))
    emb = glx.aggregate_weighted(glx.SUM, _cuda(X), _cuda(rows), alpha, len(cnt), cnt=_cuda(cnt))
    want = wref.forward(wref.SUM, X, rows, alpha.cpu().numpy(), cnt, len(cnt))
    assert wref.same_bits(emb.cpu().numpy(), want)
    # every non-empty segment's coefficients sum to one, so a table of one repeated row comes back as that row
    ones = np.tile(X[:1], (num_rows, 1))
    emb = glx.aggregate_weighted(glx.SUM, _cuda(ones), _cuda(rows), alpha, len(cnt), cnt=_cuda(cnt)).cpu().numpy()
    full = np.diff(sref.starts(cnt, n, len(cnt))) > 0
    assert np.allclose(emb[full], X[0], rtol=1e-5, atol=1e-6) and not emb[~full].any()
