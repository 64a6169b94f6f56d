"""glx_dot_attention and glx_dot_attention_backward on the GPU against the numpy restatement of their contract
(dot_attention_ref.py): every output starts as a NaN canary, every call is made twice and must repeat its bits, each
stage is checked from the engine's own previous output -- logit -> soft -> out, grad_e -> grad_q / grad_edge / grad_k /
grad_v -- inside the stated bound where the contract is a tolerance and bit for bit where it is exact."""
import numpy as np
import pytest

import dot_attention_ref as dref
import glx
from test_gpu_segment_softmax import _bits, _cuda

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
# (dim, heads): C = 8 and 4 in sub-groups of float4 lanes; C = 12 is three float4 lanes to a head, not a power of two:
# the loop over heads; C = 50 reads float by float; 256 / 4 is the flagship width
SHAPES = [(8, 1), (8, 2), (36, 3), (100, 2), (256, 4)]
LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 1500]
M = 97  # rows of k and v


def _canary(shape, host, offset=False):
    a = np.full(shape, NAN, np.float32)
    return a if host else _cuda(a, offset)


def _np(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def _dev(host, offset, *arrays):
    if host:
        return arrays
    return tuple(_cuda(a, offset and a is not None and a.dtype == np.float32) for a in arrays)


class Request:
    def __init__(self, dim, heads, cnt, n, S, seed, with_edge, num_rows=M):
        rng = np.random.default_rng(seed)
        self.dim, self.heads, self.cnt, self.n, self.S, self.num_rows = dim, heads, cnt, n, S, num_rows
        self.q = rng.standard_normal((S, dim)).astype(np.float32)
        self.k = rng.standard_normal((num_rows, dim)).astype(np.float32)
        self.v = rng.standard_normal((num_rows, dim)).astype(np.float32)
        self.rows = rng.integers(0, num_rows, n).astype(np.int64)
        self.edge = rng.standard_normal((n, dim)).astype(np.float32) if with_edge else None
        self.g = rng.standard_normal((S, dim)).astype(np.float32)
        self.scale = float(dref.default_scale(dim, heads))


def lengths_request(dim, heads, with_edge, seed, cut=False):
    """LENGTHS shuffled behind a leading empty segment, with a negative count; cut False: 5 positions behind sum(cnt)
    that nobody consumes; True: the counts promise 20 positions more than the request has"""
    rng = np.random.default_rng(seed)
    body = LENGTHS[1:]
    rng.shuffle(body)
    cnt = np.array([0] + body[:4] + [-4] + body[4:] + ([33, 7] if cut else []) + [0], np.int32)
    n = int(np.maximum(cnt, 0).sum()) + (-20 if cut else 5)
    return Request(dim, heads, cnt, n, len(cnt), seed, with_edge)


def gpu_forward(r, host=False, offset=False, same_kv=False, want_logit=True, **kw):
    """(out, soft, logit) of the first of two calls into NaN canaries; the second call must repeat the bits"""
    q, k, v, rows, edge, cnt = _dev(host, offset, r.q, r.k, r.v, r.rows, r.edge, r.cnt)
    if same_kv:
        v = k
    res = []
    for _ in range(2):
        got = glx.dot_attention(q, k, v, rows, cnt=cnt, edge=edge, heads=r.heads, scale=r.scale,
                                out=_canary((r.S, r.dim), host, offset), soft_out=_canary((r.n, r.heads), host, offset),
                                logit_out=_canary((r.n, r.heads), host, offset) if want_logit else None, **kw)
        res.append([_np(x) for x in got])
    for a, b in zip(*res):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b)), "an output differs between two calls"
    return res[0]


def gpu_backward(r, soft, host=False, offset=False, same_kv=False, want=(True, True, True, True), **kw):
    """(grad_e, grad_q, grad_k, grad_v, grad_edge) of the first of two calls into NaN canaries"""
    q, k, v, rows, edge, cnt, dsoft, g = _dev(host, offset, r.q, r.k, r.v, r.rows, r.edge, r.cnt, soft, r.g)
    if same_kv:
        v = k
    shapes = [(r.S, r.dim), (r.num_rows, r.dim), (r.num_rows, r.dim), (r.n, r.dim)]
    res = []
    for _ in range(2):
        outs = [_canary(s, host, offset) if w else None for s, w in zip(shapes, want)]
        if r.edge is None:
            outs[3] = None
        got = glx.dot_attention_backward(dsoft, g, q, k, v, rows, cnt=cnt, edge=edge, heads=r.heads, scale=r.scale,
                                         out=_canary((r.n, r.heads), host, offset), out_q=outs[0], out_k=outs[1],
                                         out_v=outs[2], out_edge=outs[3], want_q=want[0], want_k=want[1],
                                         want_v=want[2], want_edge=want[3], **kw)
        res.append([_np(x) for x in got])
    for a, b in zip(*res):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b)), "a gradient differs between two calls"
    return res[0]


def engine_grad_rows(r, w, grad_out, host):
    """the existing glx_aggregate_weighted_backward_x(Sum) of the same request"""
    if host:
        return glx.aggregate_weighted_backward_x(glx.SUM, r.rows, w, r.cnt, grad_out, r.num_rows)
    return glx.aggregate_weighted_backward_x(glx.SUM, _cuda(r.rows), _cuda(w), _cuda(r.cnt), _cuda(grad_out),
                                             r.num_rows).cpu().numpy()


def check(r, host=False, offset=False, same_kv=False, default_attr=0.0, drop_p=0.0, seed=0, call=0):
    """one request through both entry points and the restatement -> dict of every output"""
    n, S, H = r.n, r.S, r.heads
    kw = dict(default_attr=default_attr, drop_p=drop_p, seed=seed, call=call)
    v = r.k if same_kv else r.v
    kk, vv = dref.gathered(r.k, r.rows, r.edge, default_attr), dref.gathered(v, r.rows, r.edge, default_attr)
    out, soft, logit = gpu_forward(r, host, offset, same_kv, **kw)
    rest = dref.segment_of(r.cnt, n, S) == S
    zeros = np.zeros((int(rest.sum()), H), np.float32)
    want, bound = dref.logits(r.q, kk, r.cnt, S, H, r.scale)
    assert not np.isnan(logit[~np.isnan(want)]).any(), "an element of logit_out was not written"
    assert dref.within_bound(logit, want, bound)
    want, bound = dref.softmax(logit, r.cnt, S)
    assert np.array_equal(np.isnan(soft), np.isnan(want)), "an element of soft was not written, or a NaN is misplaced"
    assert dref.within_bound(soft, want, bound)
    assert dref.same_bits(logit[rest], zeros) and dref.same_bits(soft[rest], zeros)  # +0.0, not -0.0
    keep = dref.keep_mask(n, H, drop_p, seed, call) if drop_p else None
    alpha = dref.drop(soft, keep, drop_p)
    assert dref.same_bits(out, dref.out(alpha, vv, r.cnt, S)), "out is not the fold of the restated alpha over vv"
    empty = np.diff(dref.starts(r.cnt, n, S)) == 0
    assert dref.same_bits(out[empty], np.zeros((int(empty.sum()), r.dim), np.float32))
    grad_e, grad_q, grad_k, grad_v, grad_edge = gpu_backward(r, soft, host, offset, same_kv, **kw)
    want, bound = dref.grad_e(soft, r.g, vv, r.cnt, S, H, r.scale, keep, drop_p)
    assert np.array_equal(np.isnan(grad_e), np.isnan(want)), "an element of grad_e was not written"
    assert dref.within_bound(grad_e, want, bound)
    assert dref.same_bits(grad_e[rest], zeros)
    assert dref.same_bits(grad_q, dref.grad_q(grad_e, kk, r.cnt, S))
    assert dref.same_bits(grad_q[empty], np.zeros((int(empty.sum()), r.dim), np.float32))
    if r.edge is not None:
        assert dref.same_bits(grad_edge, dref.grad_edge(grad_e, alpha, r.q, r.g, r.cnt, S))
    else:
        assert grad_edge is None
    assert grad_k.shape == r.k.shape and dref.same_bits(grad_k, engine_grad_rows(r, grad_e, r.q, host))
    assert grad_v.shape == r.v.shape and dref.same_bits(grad_v, engine_grad_rows(r, alpha, r.g, host))
    return dict(out=out, soft=soft, logit=logit, alpha=alpha, grad_e=grad_e, grad_q=grad_q, grad_k=grad_k, grad_v=grad_v,
                grad_edge=grad_edge)


@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_segment_lengths_and_an_unconsumed_tail(dim, heads, with_edge):
    check(lengths_request(dim, heads, with_edge, seed=dim + heads))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("dim,heads", [(8, 2), (36, 3)])
def test_counts_that_promise_more_than_the_request_has(dim, heads, host):
    r = lengths_request(dim, heads, True, seed=50 + dim, cut=True)
    check(r, host=host, drop_p=0.25 if host else 0.0, seed=3, call=4)
    assert dref.starts(r.cnt, r.n, r.S)[-1] == r.n


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("dim,heads", [(8, 1), (36, 3), (256, 4)])
@pytest.mark.parametrize("fanout", [1, 10])
def test_implied_layout(fanout, dim, heads, host):
    """cnt=None; 37 segments are two workgroups at 8 lanes per segment"""
    S = 37
    r = Request(dim, heads, None, S * fanout, S, fanout * 10 + heads, with_edge=dim != 36)
    got = check(r, host=host)
    if fanout == 1:
        assert dref.same_bits(got["soft"], np.ones((S, heads), np.float32))  # k = 1: exactly 1.0


@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_every_pointer_one_float_off_16_byte_alignment(dim, heads, with_edge):
    check(lengths_request(dim, heads, with_edge, seed=90 + dim + heads), offset=True, drop_p=0.25, seed=5, call=6)


@pytest.mark.parametrize("default_attr", [0.0, 0.5])
@pytest.mark.parametrize("dim,heads", [(8, 2), (100, 2)])
def test_rows_outside_the_table_read_default_attr(dim, heads, default_attr):
    """rows -1 and num_rows read default_attr in both tables and pass no gradient to either; an empty segment is +0.0
    whatever default_attr is"""
    cnt = np.array([1, 7, 0, 33, 70], np.int32)
    r = Request(dim, heads, cnt, int(cnt.sum()), len(cnt), 21 + dim, with_edge=True)
    outside = [0, 3, 8, 20, 60, 110]
    r.rows[outside] = [-1, M, -1, M, -2 ** 40, 2 ** 40]
    got = check(r, default_attr=default_attr)
    assert dref.same_bits(got["out"][2], np.zeros(dim, np.float32))
    assert np.isfinite(got["out"]).all() and got["out"][0].any()
    # the restated row gradients skip those positions too
    assert dref.same_bits(got["grad_k"], dref.grad_rows(got["grad_e"], r.rows, cnt, r.q, M))
    assert dref.same_bits(got["grad_v"], dref.grad_rows(got["alpha"], r.rows, cnt, r.g, M))
    # position 0 is its segment's only one: soft is 1 and out is default_attr + edge
    assert dref.same_bits(got["out"][0], (np.float32(default_attr) + r.edge[0]).astype(np.float32))


@pytest.mark.parametrize("dim,heads", [(8, 1), (256, 4)])
def test_a_hub_row_and_rows_nobody_names(dim, heads):
    cnt = np.array([150, 30, 170, 5, 64], np.int32)
    n = int(cnt.sum())
    r = Request(dim, heads, cnt, n, len(cnt), dim, with_edge=True)
    rng = np.random.default_rng(1)
    r.rows[:] = rng.integers(40, 60, n)
    r.rows[rng.choice(n, 300, replace=False)] = 7  # the hub: 300 positions across the segments
    got = check(r)
    assert (r.rows == 7).sum() == 300 and got["grad_k"][7].all() and got["grad_v"][7].all()
    named = np.zeros(M, bool)
    named[np.unique(r.rows)] = True
    zeros = np.zeros((int((~named).sum()), dim), np.float32)
    assert dref.same_bits(got["grad_k"][~named], zeros) and dref.same_bits(got["grad_v"][~named], zeros)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
def test_key_and_value_in_one_buffer(with_edge, host):
    r = lengths_request(36, 3, with_edge, seed=7)
    one = check(r, host=host, same_kv=True)
    r.v = r.k.copy()
    two = check(r, host=host)
    for name in one:
        assert (one[name] is None and two[name] is None) or np.array_equal(_bits(one[name]), _bits(two[name])), name


@pytest.mark.parametrize("where", ["q", "k", "edge"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "minus_inf"])
def test_a_non_finite_element_takes_its_column_and_nothing_else(bad, where):
    """the element sits in head 0 of segment 1: that (segment, head) column follows the softmax rules, which check()
    restates from the engine's own logits; every other segment keeps its bits"""
    dim, heads = 8, 2
    cnt = np.array([9, 70, 9], np.int32)
    n = int(cnt.sum())
    r = Request(dim, heads, cnt, n, 3, 3, with_edge=True, num_rows=n + 1)
    r.rows[:] = np.arange(n)  # every row is named once: row 9 + 35 belongs to segment 1 alone
    clean = check(r)
    if where == "q":
        r.q[1, 1] = bad
    elif where == "k":
        r.k[9 + 35, 1] = bad
    else:
        r.edge[9 + 35, 1] = bad
    got = check(r)
    col = got["logit"][9:79, 0]
    assert not np.isfinite(col).all()
    if np.isnan(col).any() or (col == np.inf).any() or (col == -np.inf).all():
        assert np.isnan(got["soft"][9:79, 0]).all()
    else:  # -inf among finite logits: exactly +0.0 there
        assert dref.same_bits(got["soft"][9:79, 0][col == -np.inf], np.zeros(int((col == -np.inf).sum()), np.float32))
    others = np.ones(n, bool)
    others[9:79] = False
    for name in ("logit", "soft", "grad_e"):
        assert np.array_equal(_bits(got[name][others]), _bits(clean[name][others])), name
        assert np.array_equal(_bits(got[name][9:79, 1]), _bits(clean[name][9:79, 1])), name  # the other head too
    for name in ("out", "grad_q"):
        assert np.array_equal(_bits(got[name][[0, 2]]), _bits(clean[name][[0, 2]])), name


@pytest.mark.parametrize("drop_p", [0.0, 0.25])
@pytest.mark.parametrize("dim,heads", [(8, 2), (36, 3), (256, 4)])
def test_dropout_mask_is_the_restated_one(dim, heads, drop_p):
    r = lengths_request(dim, heads, True, seed=int(drop_p * 100) + dim)
    seed, call = 2 ** 40 + 12345, 2 ** 33 + 7  # both halves of both words are used
    got = check(r, drop_p=drop_p, seed=seed, call=call)  # out and grad_v are bit-exact folds of the restated alpha
    if drop_p == 0:
        assert dref.same_bits(got["alpha"], got["soft"])
        return
    keep = dref.keep_mask(r.n, heads, drop_p, seed, call)
    used = dref.segment_of(r.cnt, r.n, r.S) < r.S
    assert 0 < (~keep[used]).sum() < keep[used].size
    # grad_edge with q = 0 is alpha[p, h] * grad_out[sg]: with grad_out = 1 it is alpha itself, element by element
    r.q[:] = 0
    r.g[:] = 1
    out, soft, _ = gpu_forward(r, drop_p=drop_p, seed=seed, call=call)
    shown = gpu_backward(r, soft, drop_p=drop_p, seed=seed, call=call)[4][:, ::dim // heads]
    assert dref.same_bits(shown, dref.drop(soft, keep, drop_p))
    assert dref.same_bits(shown[~keep], np.zeros_like(shown[~keep])) and (shown[keep & used[:, None]] > 0).all()
    other = gpu_backward(r, soft, drop_p=drop_p, seed=seed, call=call + 1)[4][:, ::dim // heads]
    assert not np.array_equal(other == 0, shown == 0), "another call must draw another mask"


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_gradients_that_are_not_asked_for(host):
    cnt = np.array([3, 0, 40, 1, 120], np.int32)
    r = Request(36, 3, cnt, int(cnt.sum()), len(cnt), 4, with_edge=True)
    full = check(r, host=host, drop_p=0.25, seed=1, call=2)
    names = ["grad_q", "grad_k", "grad_v", "grad_edge"]
    for skip in range(4):
        want = tuple(i != skip for i in range(4))
        got = gpu_backward(r, full["soft"], host, want=want, drop_p=0.25, seed=1, call=2)
        assert np.array_equal(_bits(got[0]), _bits(full["grad_e"]))
        for i, name in enumerate(names):
            if i == skip:
                assert got[1 + i] is None
            else:
                assert np.array_equal(_bits(got[1 + i]), _bits(full[name])), (skip, name)
    got = gpu_backward(r, full["soft"], host, want=(False,) * 4, drop_p=0.25, seed=1, call=2)
    assert np.array_equal(_bits(got[0]), _bits(full["grad_e"])) and all(x is None for x in got[1:])
    # and no logits going forward
    out, soft, logit = gpu_forward(r, host, want_logit=False, drop_p=0.25, seed=1, call=2)
    assert logit is None and np.array_equal(_bits(out), _bits(full["out"]))
    assert np.array_equal(_bits(soft), _bits(full["soft"]))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_no_positions_and_no_segments(host):
    # no positions: every segment is empty, +0.0 whatever default_attr is, and every gradient is zeros
    cnt = np.array([0, 0, 0], np.int32)
    r = Request(8, 2, cnt, 0, 3, 5, with_edge=True, num_rows=5)
    got = check(r, host=host, default_attr=0.5)
    assert dref.same_bits(got["out"], np.zeros((3, 8), np.float32))
    assert dref.same_bits(got["grad_k"], np.zeros((5, 8), np.float32)) and got["grad_edge"].shape == (0, 8)
    # counts that consume nothing
    r = Request(8, 2, np.array([0, -1, 0], np.int32), 6, 3, 5, with_edge=True, num_rows=5)
    got = check(r, host=host, drop_p=0.25, seed=1)
    assert dref.same_bits(got["soft"], np.zeros((6, 2), np.float32))
    assert dref.same_bits(got["grad_edge"], np.zeros((6, 8), np.float32))
    # no segments: nothing is consumed
    r = Request(8, 2, None, 6, 0, 5, with_edge=True, num_rows=5)
    got = check(r, host=host)
    assert got["out"].shape == (0, 8) and dref.same_bits(got["logit"], np.zeros((6, 2), np.float32))
    assert dref.same_bits(got["grad_v"], np.zeros((5, 8), np.float32))


@pytest.mark.parametrize("dim,heads", SHAPES)
def test_without_edge_and_dropout_out_is_the_weighted_sum_of_soft(dim, heads):
    r = lengths_request(dim, heads, False, seed=200 + dim)
    out, soft, _ = gpu_forward(r)
    want = glx.aggregate_weighted(glx.SUM, _cuda(r.v), _cuda(r.rows), _cuda(soft), r.S, cnt=_cuda(r.cnt))
    got, want = out.copy(), want.cpu().numpy()
    empty = np.diff(dref.starts(r.cnt, r.n, r.S)) == 0
    assert empty.any() and not got[empty].any()
    assert np.array_equal(_bits(got[~empty]), _bits(want[~empty]))  # an empty segment there is default_attr: 0.0 too
    assert np.array_equal(_bits(got), _bits(want))
