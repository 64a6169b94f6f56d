"""glx_aggregate_weighted and its two gradients on the GPU against the numpy restatement of the contracts
(agg_weighted_ref.py).  Tolerance 0 for the forward and grad_x (bit equality, the sign of zero included; a NaN matches
a NaN); grad_w within its derived bound of the float64 value, and bit-identical between two calls."""
import numpy as np
import pytest

import agg_backward_ref as ref
import agg_weighted_ref as wref
import glx
from test_gpu_agg_backward import BASE_ROWS

pytestmark = pytest.mark.gpu

OPS = {"sum": wref.SUM, "mean": wref.MEAN}
U = 4  # row loads the kernels keep in flight per lane (kWU)
NAN = np.float32(np.nan)


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


def gpu_all(op, X, rows, w, cnt, S, grad_out, default_attr=0.0, host=False, offset=False):
    """(emb, grad_x, grad_w, grad_w of a second call) as numpy; every output buffer starts as a NaN canary"""
    num_rows, D = X.shape
    n, heads = len(rows), w.reshape(len(rows), -1).shape[1]
    if host:
        emb, gx = np.full((S, D), NAN, np.float32), np.full((num_rows, D), NAN, np.float32)
        gw = [np.full((n, heads), NAN, np.float32) for _ in range(2)]
        glx.aggregate_weighted(op, X, rows, w, S, cnt=cnt, default_attr=default_attr, out=emb)
        glx.aggregate_weighted_backward_x(op, rows, w, cnt, grad_out, num_rows, out=gx)
        for out in gw:
            glx.aggregate_weighted_backward_w(op, X, rows, heads, cnt, grad_out, default_attr, out=out)
        return emb, gx, gw[0], gw[1]
    dX, dg, dw = _cuda(X, offset), _cuda(grad_out, offset), _cuda(w, offset)
    drows, dcnt = _cuda(rows), _cuda(cnt)
    emb = _cuda(np.full((S, D), NAN, np.float32), offset)
    gx = _cuda(np.full((num_rows, D), NAN, np.float32), offset)
    gw = [_cuda(np.full((n, heads), NAN, np.float32), offset) for _ in range(2)]
    glx.aggregate_weighted(op, dX, drows, dw, S, cnt=dcnt, default_attr=default_attr, out=emb)
    glx.aggregate_weighted_backward_x(op, drows, dw, dcnt, dg, num_rows, out=gx)
    for out in gw:
        glx.aggregate_weighted_backward_w(op, dX, drows, heads, dcnt, dg, default_attr, out=out)
    return emb.cpu().numpy(), gx.cpu().numpy(), gw[0].cpu().numpy(), gw[1].cpu().numpy()


def check(op, X, rows, w, cnt, S, grad_out, default_attr=0.0, host=False, offset=False):
    """one request through the three entry points and the restatement"""
    heads = w.reshape(len(rows), -1).shape[1]
    emb, gx, gw, gw2 = gpu_all(op, X, rows, w, cnt, S, grad_out, default_attr, host, offset)
    want_emb = wref.forward(op, X, rows, w, cnt, S, default_attr)
    want_gx = wref.backward_x(op, rows, w, cnt, grad_out, X.shape[0])
    want_gw, bound = wref.backward_w(op, X, rows, heads, cnt, grad_out, default_attr)
    assert np.array_equal(np.isnan(emb), np.isnan(want_emb)), "an element of emb was not written"
    assert wref.same_bits(emb, want_emb)
    assert np.array_equal(np.isnan(gx), np.isnan(want_gx)), "an element of grad_x was not written"
    assert wref.same_bits(gx, want_gx)
    assert np.array_equal(np.isnan(gw), np.isnan(want_gw)), "an element of grad_w was not written"
    assert wref.within_bound(gw, want_gw, bound)
    assert np.array_equal(gw.view(np.uint32), gw2.view(np.uint32)), "grad_w differs between two calls"
    return emb, gx, gw


def _data(seed, num_rows, D, n, heads, S):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((num_rows, D)).astype(np.float32)
    w = rng.standard_normal((n, heads)).astype(np.float32)
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    grad_out[0, 0] = -0.0
    return X, w, grad_out


BASE_SHAPES = [(d, h) for d in (1, 4, 32, 64, 100, 128, 256, 260) for h in (1, 2, 4) if d % h == 0] + [(8, 8)]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim, heads", BASE_SHAPES)
def test_base_request_every_dimension_path(dim, heads, op, host):
    """3 x 5 positions over 7 rows.  C % 4 == 0: the float4 path (G = 8 .. 64, 260: a second column tile); 100 / 4
    (C = 25), 260 / 2, 260 / 4, 1 and 8 / 8 (C = 1): the scalar path.  grad_w: C / VEC a power of two reduces in
    sub-groups, otherwise (C = 25, 65, 100, 130, 260) head by head."""
    assert (100, 4) in BASE_SHAPES and (8, 8) in BASE_SHAPES
    X, w, grad_out = _data(dim * 8 + heads, 7, dim, len(BASE_ROWS), heads, 3)
    emb, gx, gw = check(OPS[op], X, BASE_ROWS, w, None, 3, grad_out, default_attr=0.25, host=host)
    assert not gx[5].any() and not np.signbit(gx[5]).any()  # nobody refers to row 5: +0.0


@pytest.mark.parametrize("dim, heads", [(512, 1), (1024, 2), (1024, 1)])
def test_heads_wider_than_one_column_tile(dim, heads):
    """C / 4 = 128 and 256 lanes' worth of columns per head: a head spans 2 and 4 column tiles of the 64-lane group"""
    X, w, grad_out = _data(dim + heads, 7, dim, len(BASE_ROWS), heads, 3)
    check(wref.MEAN, X, BASE_ROWS, w, None, 3, grad_out)


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim, heads", [(4, 1), (100, 4), (64, 2)])
def test_all_ones_weights_equal_the_unweighted_reduce(dim, heads, op):
    """heads == 1 is the stated contract; more heads of ones must give the same bits too"""
    rng = np.random.default_rng(dim)
    num_rows, S, k = 9, 6, 7
    X = rng.standard_normal((num_rows, dim)).astype(np.float32)
    X[1, 0], X[2, 1 % dim], X[3, 2 % dim], X[4, 3 % dim] = np.nan, np.inf, -np.inf, -0.0
    X[5] = -0.0
    rows = rng.integers(-1, num_rows + 1, S * k).astype(np.int64)
    rows[:k] = 5  # a segment of -0.0 rows
    feats = glx.Features(_cuda(X), view=True)
    want, cnt = feats.aggregate(OPS[op], _cuda(rows), None, S, -0.0)
    ones = np.ones((S * k, heads), np.float32)
    got = glx.aggregate_weighted(OPS[op], _cuda(X), _cuda(rows), _cuda(ones), S, default_attr=-0.0)
    assert ref.same_bits(got.cpu().numpy(), want.cpu().numpy())
    # ... and through the counts the unweighted forward returned
    got = glx.aggregate_weighted(OPS[op], _cuda(X), _cuda(rows), _cuda(ones), S, cnt=cnt, default_attr=-0.0)
    assert ref.same_bits(got.cpu().numpy(), want.cpu().numpy())


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim, heads", [(4, 1), (100, 4), (64, 2)])
def test_segment_lengths_at_the_launch_edges_and_an_unconsumed_tail(dim, heads, op):
    lengths = [0, 1, U, U + 1, 63, 64, 65, 200]
    cnt = np.array(lengths, np.int32)
    n, num_rows = int(cnt.sum()) + 5, 50  # the last 5 positions are not consumed
    rng = np.random.default_rng(9)
    rows = rng.integers(-1, num_rows - 1, n).astype(np.int64)  # -1 .. num_rows - 2
    rows[7] = num_rows  # a consumed position beyond the table
    rows[-5:] = num_rows - 1  # a row that only the tail refers to
    X, w, grad_out = _data(dim, num_rows, dim, n, heads, len(lengths))
    emb, gx, gw = check(OPS[op], X, rows, w, cnt, len(lengths), grad_out, default_attr=0.5)
    assert (emb[0] == 0.5).all()  # the empty segment
    assert not gw[-5:].any() and not np.signbit(gw[-5:]).any()  # +0.0
    assert not gx[num_rows - 1].any()


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim, heads", [(4, 1), (100, 4)])
def test_row_list_lengths_at_the_launch_edges(dim, heads, op):
    lengths = [0, 1, U, U + 1, 63, 64, 65, 200]
    rows = np.repeat(np.arange(len(lengths)), lengths).astype(np.int64)
    np.random.default_rng(3).shuffle(rows)
    assert len(rows) == 402
    X, w, grad_out = _data(dim + 1, len(lengths), dim, len(rows), heads, 6)
    check(OPS[op], X, rows, w, None, 6, grad_out)


@pytest.mark.parametrize("dim", [4, 64, 128, 256])  # 32 / 16 / 8 / 4 groups per workgroup
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_segment_row_and_position_counts_at_the_workgroup_edges(count, dim):
    """`count` segments (forward), `count` rows (grad_x) and 3 * count positions (grad_w: 3, 189, 192, 195, 771)"""
    rng = np.random.default_rng(count)
    rows = rng.integers(-1, count + 1, 3 * count).astype(np.int64)
    rows[-1] = count - 1  # the last row of the last workgroup has a list
    X, w, grad_out = _data(count + dim, count, dim, len(rows), 2, count)
    check(wref.MEAN, X, rows, w, None, count, grad_out)


@pytest.mark.parametrize("op", sorted(OPS))
def test_special_weights(op):
    """0.0, -0.0, a subnormal, and inf times a zero element: NaN is the contract's answer, here and in the restatement"""
    rng = np.random.default_rng(41)
    num_rows, D, S, k = 6, 8, 4, 5
    X = rng.standard_normal((num_rows, D)).astype(np.float32)
    X[2, :4] = 0.0
    X[3, 4:] = -0.0
    rows = rng.integers(0, num_rows, S * k).astype(np.int64)
    rows[0], rows[6] = 2, 3
    w = rng.standard_normal((S * k, 2)).astype(np.float32)
    w[0] = np.inf  # times row 2's zeros: NaN in columns 0..3 of segment 0
    w[6] = -np.inf  # times row 3's -0.0: NaN in columns 4..7 of segment 1
    w[1], w[2], w[3] = 0.0, -0.0, np.float32(1e-41)
    w[10:15] = -0.0  # a whole segment of -0.0 weights: the sign of each zero sum is the contract's
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    grad_out[0, :2] = 0.0  # inf * 0 in grad_x too
    emb, gx, gw = check(OPS[op], X, rows, w, None, S, grad_out)
    assert np.isnan(emb[0, :4]).all() and not np.isnan(emb[0, 4:]).any()
    assert np.isnan(emb[1, 4:]).all()
    assert np.isnan(gx[2, :2]).all()


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim, heads", [(64, 2), (256, 1)])
def test_misaligned_pointers_take_the_scalar_path_with_the_same_bits(dim, heads, op):
    rng = np.random.default_rng(dim)
    num_rows, S, k = 12, 5, 6
    rows = rng.integers(-1, num_rows + 1, S * k).astype(np.int64)
    X, w, grad_out = _data(dim + 3, num_rows, dim, S * k, heads, S)
    aligned = gpu_all(OPS[op], X, rows, w, None, S, grad_out)
    emb, gx, gw = check(OPS[op], X, rows, w, None, S, grad_out, offset=True)
    assert wref.same_bits(emb, aligned[0]) and wref.same_bits(gx, aligned[1])


@pytest.mark.parametrize("op", sorted(OPS))
def test_counts_that_promise_more_than_the_request_has(op):
    """6 positions, counts 3 + 4 + 5: the second segment is cut to 3 positions (Mean divides by 3), the third to none
    (it is empty: default_attr, no gradient)"""
    rows = np.array([0, 1, 2, 3, 1, 0], np.int64)
    X, w, grad_out = _data(13, 4, 8, 6, 2, 3)
    emb, gx, gw = check(OPS[op], X, rows, w, np.array([3, 4, 5], np.int32), 3, grad_out, default_attr=0.5)
    assert (emb[2] == 0.5).all() and gw.all()


def test_weighted_max_min_prod_are_refused():
    import torch
    x = torch.ones((3, 4), device="cuda")
    rows = torch.zeros(4, dtype=torch.int64, device="cuda")
    w = torch.ones((4, 1), device="cuda")
    for op, name in ((glx.MAX, "Max"), (glx.MIN, "Min"), (glx.PROD, "Prod")):
        with pytest.raises(glx.GlxError) as e:
            glx.aggregate_weighted(op, x, rows, w, 2)
        assert e.value.code == 3 and name in str(e.value)


def test_empty_requests():
    import torch
    x = torch.ones((3, 4), device="cuda")
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    w0 = torch.zeros((0, 2), device="cuda")
    emb = glx.aggregate_weighted(glx.SUM, x, none, w0, 2, default_attr=1.5)
    assert (emb.cpu().numpy() == 1.5).all()
    g = torch.ones((2, 4), device="cuda")
    gx = torch.full((3, 4), float("nan"), device="cuda")
    glx.aggregate_weighted_backward_x(glx.SUM, none, w0, None, g, 3, out=gx)
    assert ref.same_bits(gx.cpu().numpy(), np.zeros((3, 4), np.float32))
    # fewer positions than segments: the implied fan-out is 0, nothing was consumed
    X, w, grad_out = _data(1, 5, 4, 2, 2, 3)
    emb, gx, gw = check(wref.SUM, X, np.array([1, 2], np.int64), w, None, 3, grad_out, default_attr=2.0)
    assert (emb == 2.0).all() and not gx.any() and not gw.any()
