"""glx_dot_attention_chunked and glx_dot_attention_backward_chunked on the GPU
against the default entry points and the numpy restatement of the chunked order (dot_attention_chunked_ref.py).  Every
output starts as a guard pattern, every call is made twice and must repeat its bits.  logit_out is the default call's
everywhere; a short segment (at most 256 positions) has the default call's bits in every output; a long one has soft
and grad_e inside the default contract's bounds and out / grad_q bit for bit the two-level fold of the engine's own
alpha / grad_e; grad_k / grad_v are the chunked row gradient of the same request."""
import numpy as np
import pytest

import dot_attention_chunked_ref as cref
import dot_attention_ref as dref
import glx
from test_gpu_dot_attention import _dev, _np
from test_gpu_segment_softmax import _bits, _cuda

pytestmark = pytest.mark.gpu

GUARD = 0x7FC01234  # a NaN no arithmetic produces: an element that still holds it was not written
# (dim, heads): VEC 1; one head of three float4 lanes; sub-groups; the flagship width; C % 4 != 0 past 256 columns; a
# second column tile at float4
SHAPES = [(6, 2), (12, 1), (16, 4), (256, 4), (260, 4), (520, 2)]


def _guard(shape, host, offset=False):
    a = np.full(shape, GUARD, np.uint32).view(np.float32)
    return a if host else _cuda(a, offset)


def _same(a, b):
    return (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


def forward(r, chunked, host=False, offset=False, same_kv=False, want_logit=True, **kw):
    """(out, soft, logit) of the first of two calls into guard patterns; the second call must repeat the bits"""
    q, k, v, rows, edge, cnt = _dev(host, offset, r.q, r.k, r.v, r.rows, r.edge, r.cnt)
    if same_kv:
        v = k
    res = []
    for _ in range(2):
        got = glx.dot_attention(q, k, v, rows, cnt=cnt, edge=edge, heads=r.heads, scale=r.scale,
                                out=_guard((r.S, r.dim), host, offset), soft_out=_guard((r.n, r.heads), host, offset),
                                logit_out=_guard((r.n, r.heads), host, offset) if want_logit else None, chunked=chunked,
                                **kw)
        res.append([_np(x) for x in got])
    for a, b in zip(*res):
        assert _same(a, b), "an output differs between two calls"
        assert a is None or not (_bits(a) == GUARD).any(), "an element was not written"
    return res[0]


def backward(r, soft, chunked, host=False, offset=False, same_kv=False, want=(True, True, True, True), **kw):
    """(grad_e, grad_q, grad_k, grad_v, grad_edge) of the first of two calls into guard patterns"""
    q, k, v, rows, edge, cnt, dsoft, g = _dev(host, offset, r.q, r.k, r.v, r.rows, r.edge, r.cnt, soft, r.g)
    if same_kv:
        v = k
    shapes = [(r.S, r.dim), (r.num_rows, r.dim), (r.num_rows, r.dim), (r.n, r.dim)]
    res = []
    for _ in range(2):
        outs = [_guard(s, host, offset) if w else None for s, w in zip(shapes, want)]
        if r.edge is None:
            outs[3] = None
        got = glx.dot_attention_backward(dsoft, g, q, k, v, rows, cnt=cnt, edge=edge, heads=r.heads, scale=r.scale,
                                         out=_guard((r.n, r.heads), host, offset), out_q=outs[0], out_k=outs[1],
                                         out_v=outs[2], out_edge=outs[3], want_q=want[0], want_k=want[1],
                                         want_v=want[2], want_edge=want[3], chunked=chunked, **kw)
        res.append([_np(x) for x in got])
    for a, b in zip(*res):
        assert _same(a, b), "a gradient differs between two calls"
        assert a is None or not (_bits(a) == GUARD).any(), "an element was not written"
    return res[0]


def engine_grad_rows(r, w, grad_out, host):
    """glx_aggregate_weighted_backward_x_chunked(Sum) of the same request"""
    if host:
        return glx.aggregate_weighted_backward_x(glx.SUM, r.rows, w, r.cnt, grad_out, r.num_rows, chunked=True)
    return glx.aggregate_weighted_backward_x(glx.SUM, _cuda(r.rows), _cuda(w), _cuda(r.cnt), _cuda(grad_out),
                                             r.num_rows, chunked=True).cpu().numpy()


def check(r, host=False, offset=False, same_kv=False, drop_p=0.0, seed=0, call=0):
    """one request through the chunked and the default entry points and the restatement -> dict of the chunked
    outputs"""
    n, S, H = r.n, r.S, r.heads
    kw = dict(drop_p=drop_p, seed=seed, call=call)
    opt = dict(host=host, offset=offset, same_kv=same_kv)
    v = r.k if same_kv else r.v
    kk, vv = dref.gathered(r.k, r.rows, r.edge), dref.gathered(v, r.rows, r.edge)
    seg_of = dref.segment_of(r.cnt, n, S)
    rest = seg_of == S
    long_seg = cref.long_segments(r.cnt, n, S)
    long_pos = np.zeros(n, bool)
    long_pos[~rest] = long_seg[seg_of[~rest]]
    zeros = np.zeros((int(rest.sum()), H), np.float32)
    empty = np.diff(dref.starts(r.cnt, n, S)) == 0

    d_out, d_soft, d_logit = forward(r, False, **opt, **kw)
    out, soft, logit = forward(r, True, **opt, **kw)
    assert _same(logit, d_logit), "logit_out is not the default entry point's"
    assert _same(soft[~long_pos], d_soft[~long_pos]), "soft of a short segment is not the default entry point's"
    want, bound = dref.softmax(logit, r.cnt, S)
    assert np.array_equal(np.isnan(soft), np.isnan(want)), "a NaN of soft is misplaced"
    assert dref.within_bound(soft, want, bound)
    assert dref.same_bits(logit[rest], zeros) and dref.same_bits(soft[rest], zeros)  # +0.0, not -0.0
    keep = dref.keep_mask(n, H, drop_p, seed, call) if drop_p else None
    alpha = dref.drop(soft, keep, drop_p)
    assert dref.same_bits(out, cref.out(alpha, vv, r.cnt, S)), "out is not the two-level fold of alpha over vv"
    assert _same(out[~long_seg], d_out[~long_seg]), "out of a short segment is not the default entry point's"
    assert dref.same_bits(out[empty], np.zeros((int(empty.sum()), r.dim), np.float32))

    d_grads = backward(r, soft, False, **opt, **kw)
    grad_e, grad_q, grad_k, grad_v, grad_edge = backward(r, soft, True, **opt, **kw)
    want, bound = dref.grad_e(soft, r.g, vv, r.cnt, S, H, r.scale, keep, drop_p)
    assert np.array_equal(np.isnan(grad_e), np.isnan(want)), "a NaN of grad_e is misplaced"
    assert dref.within_bound(grad_e, want, bound)
    assert dref.same_bits(grad_e[rest], zeros)
    assert _same(grad_e[~long_pos], d_grads[0][~long_pos]), "grad_e of a short segment is not the default's"
    assert dref.same_bits(grad_q, cref.grad_q(grad_e, kk, r.cnt, S)), "grad_q is not the two-level fold of grad_e"
    assert _same(grad_q[~long_seg], d_grads[1][~long_seg]), "grad_q of a short segment is not the default's"
    assert dref.same_bits(grad_q[empty], np.zeros((int(empty.sum()), r.dim), np.float32))
    if r.edge is not None:
        assert dref.same_bits(grad_edge, dref.grad_edge(grad_e, alpha, r.q, r.g, r.cnt, S))
        assert _same(grad_edge[~long_pos], d_grads[4][~long_pos]), "grad_edge of a short segment is not the default's"
    else:
        assert grad_edge is None
    assert grad_k.shape == r.k.shape and _same(grad_k, engine_grad_rows(r, grad_e, r.q, host))
    assert grad_v.shape == r.v.shape and _same(grad_v, engine_grad_rows(r, alpha, r.g, host))
    return dict(out=out, soft=soft, logit=logit, alpha=alpha, grad_e=grad_e, grad_q=grad_q, grad_k=grad_k,
                grad_v=grad_v, grad_edge=grad_edge, default_out=d_out, default_grads=d_grads)


def planted(r, got, plain_values):
    """the exact rules of the softmax in the long segments of hub_request, and the +0.0f starts of the fold"""
    start = dref.starts(r.cnt, r.n, r.S)
    soft = got["soft"]
    a, b = int(start[cref.SEG_700]), int(start[cref.SEG_700 + 1])
    assert b - a == 700 and dref.same_bits(soft[a:b], np.full((700, r.heads), np.float32(1.0) / np.float32(700)))
    p = int(start[cref.SEG_513]) + 300
    assert (got["logit"][p] == -np.inf).all() and dref.same_bits(soft[p], np.zeros(r.heads, np.float32))
    a, b = int(start[cref.SEG_513]), int(start[cref.SEG_513 + 1])
    assert np.isfinite(soft[a:b]).all() and (np.delete(soft[a:b], 300, 0) > 0).all()
    a, b = int(start[cref.SEG_NAN]), int(start[cref.SEG_NAN + 1])
    assert np.isnan(got["logit"][a + 100, 0]) and np.isnan(soft[a:b, 0]).all() and np.isfinite(soft[a:b, 1:]).all()
    a, b = int(start[cref.SEG_INF]), int(start[cref.SEG_INF + 1])
    assert (got["logit"][a:b] == -np.inf).all() and np.isnan(soft[a:b]).all()
    if plain_values:  # no edge term and v apart from k: every term of SEG_ZERO is -0.0f
        assert dref.same_bits(got["out"][cref.SEG_ZERO], np.zeros(r.dim, np.float32))


def differs(r, got):
    """the chunked order shows: the long segments the CPU test names have other bits than the default order's"""
    for sg in (cref.SEG_512, cref.SEG_513, cref.SEG_700):
        assert not _same(got["out"][sg], got["default_out"][sg]), sg


@pytest.mark.parametrize("drop_p", [0.0, 0.4])
@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_long_and_short_segments_and_long_rows(dim, heads, with_edge, drop_p):
    r = cref.hub_request(dim, heads, with_edge, cref.hub_seed(dim, heads, with_edge))
    got = check(r, drop_p=drop_p, seed=2 ** 40 + 11, call=2 ** 33 + 5)
    planted(r, got, plain_values=not with_edge)
    differs(r, got)


@pytest.mark.parametrize("dim,heads", SHAPES)
def test_key_and_value_in_one_buffer(dim, heads):
    r = cref.hub_request(dim, heads, True, cref.hub_seed(dim, heads, True))
    got = check(r, same_kv=True, drop_p=0.4, seed=9, call=1)
    planted(r, got, plain_values=False)


@pytest.mark.parametrize("dim,heads", [(16, 4), (256, 4), (520, 2)])
def test_every_pointer_one_float_off_16_byte_alignment(dim, heads):
    """the float4 path is refused in both directions"""
    r = cref.hub_request(dim, heads, True, cref.hub_seed(dim, heads, True))
    got = check(r, offset=True, drop_p=0.4, seed=5, call=6)
    planted(r, got, plain_values=False)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_counts_that_promise_more_than_the_request_has(host):
    r = cref.hub_request(16, 4, True, cref.hub_seed(16, 4, True), cut=True)
    assert dref.starts(r.cnt, r.n, r.S)[-1] == r.n
    check(r, host=host, drop_p=0.4, seed=3, call=4)


def test_host_pointers_give_the_device_call_bits():
    r = cref.hub_request(16, 4, True, cref.hub_seed(16, 4, True))
    kw = dict(drop_p=0.4, seed=7, call=8)
    dev, host = forward(r, True, **kw), forward(r, True, host=True, **kw)
    for a, b in zip(dev, host):
        assert _same(a, b)
    dev, host = backward(r, dev[1], True, **kw), backward(r, dev[1], True, host=True, **kw)
    for a, b in zip(dev, host):
        assert _same(a, b)


@pytest.mark.parametrize("dim,heads", [(6, 2), (256, 4)])
def test_long_segments_of_the_implied_layout(dim, heads):
    """cnt=None, three segments of 513 positions"""
    r = cref.implied_request(dim, heads, True, 40 + dim, 3, 513)
    got = check(r, drop_p=0.4, seed=1, call=2)
    assert not _same(got["out"], got["default_out"])


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("dim,heads", [(12, 1), (256, 4)])
def test_without_long_segments_and_long_rows_every_output_is_the_default_one(dim, heads, host):
    """37 segments of 40 positions over 97 rows"""
    r = cref.implied_request(dim, heads, True, 60 + dim, 37, 40)
    assert cref.list_lengths(r.rows, r.cnt, r.S, r.num_rows).max() <= cref.CHUNK
    got = check(r, host=host, drop_p=0.4, seed=3, call=9)
    assert _same(got["out"], got["default_out"])
    for a, b in zip((got["grad_e"], got["grad_q"], got["grad_k"], got["grad_v"], got["grad_edge"]),
                    got["default_grads"]):
        assert _same(a, b)


def test_dropout_with_the_row_gradients_asked_for():
    """the workspace case: alpha outlives the leases the chunked row gradient takes inside the call"""
    r = cref.hub_request(16, 4, True, cref.hub_seed(16, 4, True))
    kw = dict(drop_p=0.4, seed=21, call=22)
    out, soft, _ = forward(r, True, **kw)
    grad_e, _, grad_k, grad_v, _ = backward(r, soft, True, want=(False, True, True, False), **kw)
    alpha = dref.drop(soft, dref.keep_mask(r.n, r.heads, 0.4, 21, 22), 0.4)
    assert _same(grad_k, engine_grad_rows(r, grad_e, r.q, False))
    assert _same(grad_v, engine_grad_rows(r, alpha, r.g, False))
    assert dref.same_bits(grad_v, cref.grad_rows(alpha, r.rows, r.cnt, r.g, r.num_rows))
    used = dref.segment_of(r.cnt, r.n, r.S) < r.S
    assert 0 < (alpha[used] == 0).sum() < alpha[used].size


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_gradients_that_are_not_asked_for(host):
    r = cref.hub_request(12, 1, True, cref.hub_seed(12, 1, True))
    kw = dict(drop_p=0.4, seed=1, call=2)
    out, soft, logit = forward(r, True, host=host, **kw)
    full = backward(r, soft, True, host=host, **kw)
    for skip in range(4):
        want = tuple(i != skip for i in range(4))
        got = backward(r, soft, True, host=host, want=want, **kw)
        for i in range(5):
            if i == skip + 1:
                assert got[i] is None
            else:
                assert _same(got[i], full[i]), (skip, i)
    got = backward(r, soft, True, host=host, want=(False,) * 4, **kw)
    assert _same(got[0], full[0]) and all(x is None for x in got[1:])
    # and no logits going forward: the dot products are parked in soft_out
    out2, soft2, logit2 = forward(r, True, host=host, want_logit=False, **kw)
    assert logit2 is None and _same(out2, out) and _same(soft2, soft)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_no_positions_and_no_segments(host):
    """zeros, as the default entry points write them"""
    cases = [cref.Request(8, 2, np.array([0, 0, 0], np.int32), 0, 3, 5, 5, with_edge=True),
             cref.Request(8, 2, np.array([0, -1, 0], np.int32), 6, 3, 5, 5, with_edge=True),
             cref.Request(8, 2, None, 6, 0, 5, 5, with_edge=True)]
    for r in cases:
        got = check(r, host=host, drop_p=0.4, seed=1)
        assert _same(got["out"], np.zeros((r.S, 8), np.float32)) and _same(got["out"], got["default_out"])
        assert _same(got["soft"], np.zeros((r.n, 2), np.float32))
        for a, b in zip((got["grad_e"], got["grad_q"], got["grad_k"], got["grad_v"], got["grad_edge"]),
                        got["default_grads"]):
            assert _same(a, b) and not _bits(a).any()
