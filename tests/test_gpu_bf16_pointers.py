"""The bfloat16 training path at every pointer offset.  A 4-element access of a bfloat16 matrix needs 8
bytes (glx_aligned_vec4), so a bfloat16 matrix 8 bytes off 16-byte alignment takes the vector path -- a class float32
never had -- and one 2, 4 or 6 bytes off takes the scalar path with 2-byte loads and stores.

Fold kernels (the weighted forward, the three row gradients, all four ops of aggregate_backward): the bits do not depend
on the path, so at every offset the output equals the aligned bfloat16 call, the float32 entry point on the upcast table
(rounded once where the output is bfloat16) and the numpy restatement, and the guard codes around every output stay.
Tree kernels (grad_w, the pair scores): the bits depend on VEC, so a bfloat16 table 0 or 8 bytes off must equal the
float32 call with everything aligned, and one 2, 4 or 6 bytes off the float32 call whose table is 4 bytes off -- which
differ from each other on the data used here (asserted).  Every comparison is to the bit."""
import numpy as np
import pytest

import agg_backward_ref as ref
import agg_weighted_ref as wref
import bf16_training_ref as b16
import glx
import pair_dot_ref as pref

pytestmark = pytest.mark.gpu

OPS = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}
SHAPES = [(12, 1), (16, 4), (48, 4), (64, 2), (256, 1), (6, 2)]  # (6, 2): C % 4 != 0, the scalar path at every offset
GUARD16, GUARD32 = 0x1234, 0x12345678
NUM_ROWS, N, S = 20, 60, 12
CNT = np.array([0, 9, 0, 7, 4, 0, 11, 1, 0, 5, 6, 30], np.int32)  # zeros; the last count is cut at N


class Placed:
    """`a` copied k ELEMENTS past a 16-byte boundary of a larger CUDA buffer that is filled with a guard code: uint16
    codes become a bfloat16 view (2 k bytes off), float32 and int32 keep their type (4 k bytes off)"""

    def __init__(self, a, k):
        import torch
        a = np.ascontiguousarray(a)
        wide = a.dtype.itemsize == 4
        assert a.dtype in (np.uint16, np.float32, np.int32)
        self.pad = (4 if wide else 8) + k  # one 16-byte line, then k elements
        self.size = a.size
        self.guard = GUARD32 if wide else GUARD16
        self.buf = torch.full((self.pad + a.size + (4 if wide else 8),), self.guard,
                              dtype=torch.int32 if wide else torch.int16, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        own = self.buf[self.pad:self.pad + a.size]
        own.copy_(torch.from_numpy(a.reshape(-1).view(np.int32 if wide else np.int16)))
        view = {"uint16": torch.bfloat16, "float32": torch.float32, "int32": torch.int32}[a.dtype.name]
        self.t = own.view(view).view(a.shape)
        assert self.t.data_ptr() % 16 == a.dtype.itemsize * k and self.t.is_contiguous()

    def guards_intact(self):
        raw = self.buf.cpu().numpy()
        return bool((raw[:self.pad] == self.guard).all() and (raw[self.pad + self.size:] == self.guard).all())

    def bits(self):
        raw = self.buf.cpu().numpy()[self.pad:self.pad + self.size]
        return raw.view(np.uint32 if raw.dtype == np.int32 else np.uint16).reshape(tuple(self.t.shape))


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(rng, shape, spread=0):
    """(uint16 codes, the float32 matrix of exactly those values); spread: every element scaled by a random power of two
    up to 2^+-spread -- products of two bfloat16 values have 16 bits, and without a spread of exponents a short sum of
    them is exact in float32 in any order"""
    x = rng.standard_normal(shape).astype(np.float32)
    if spread:
        x = x * (2.0 ** rng.integers(-spread, spread + 1, shape)).astype(np.float32)
    codes = b16.to_bf16(x)
    return codes, b16.upcast(codes)


def _out16(shape, k):
    return Placed(np.full(shape, 0x7FC0, np.uint16), k)  # a NaN canary


def _out32(shape, k):
    return Placed(np.full(shape, np.nan, np.float32), k)


def _weighted_request(dim, heads):
    rng = np.random.default_rng(dim * 8 + heads)
    codes, xf = _table(rng, (NUM_ROWS, dim))
    rows = rng.integers(-1, NUM_ROWS + 1, N).astype(np.int64)
    rows[:2] = (-1, NUM_ROWS)
    rows[-1] = NUM_ROWS - 1  # the last row, next to the guard, has a list
    w = rng.standard_normal((N, heads)).astype(np.float32)
    grad_out = rng.standard_normal((S, dim)).astype(np.float32)
    return codes, xf, rows, w, grad_out


# ---- fold kernels: the same bits at every offset, nothing written outside --------------------------------------------
@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_weighted_forward_at_every_offset(dim, heads, op):
    op = OPS[op]
    codes, xf, rows, w, _ = _weighted_request(dim, heads)
    d_rows, d_w, d_cnt = _cuda(rows), _cuda(w), _cuda(CNT)
    kw = dict(cnt=d_cnt, default_attr=0.25)
    want = glx.aggregate_weighted(op, Placed(codes, 0).t, d_rows, d_w, S, **kw).cpu().numpy()
    assert np.array_equal(want.view(np.uint32), glx.aggregate_weighted(op, _cuda(xf), d_rows, d_w, S,
                                                                       **kw).cpu().numpy().view(np.uint32))
    assert wref.same_bits(want, wref.forward(op, xf, rows, w, CNT, S, 0.25))
    # x alone, emb alone, both
    for kx, ke in [(1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (1, 1), (4, 1)]:
        x, emb = Placed(codes, kx), _out32((S, dim), ke)
        assert glx.aggregate_weighted(op, x.t, d_rows, d_w, S, out=emb.t, **kw) is emb.t
        assert np.array_equal(emb.bits(), want.view(np.uint32)), (kx, ke)
        assert emb.guards_intact() and x.guards_intact(), (kx, ke)


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_weighted_backward_x_at_every_offset(dim, heads, op):
    op = OPS[op]
    _, _, rows, w, grad_out = _weighted_request(dim, heads)
    d_rows, d_w, d_cnt = _cuda(rows), _cuda(w), _cuda(CNT)
    aligned = _out16((NUM_ROWS, dim), 0)
    glx.aggregate_weighted_backward_x(op, d_rows, d_w, d_cnt, _cuda(grad_out), NUM_ROWS, out=aligned.t)
    want = aligned.bits()
    gx32 = glx.aggregate_weighted_backward_x(op, d_rows, d_w, d_cnt, _cuda(grad_out), NUM_ROWS).cpu().numpy()
    assert np.array_equal(want, b16.to_bf16(gx32))
    assert np.array_equal(want, b16.to_bf16(wref.backward_x(op, rows, w, CNT, grad_out, NUM_ROWS)))
    assert aligned.guards_intact()
    # grad_x alone, grad_out alone, both
    for kg, kx in [(0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 4)]:
        go, gx = Placed(grad_out, kg), _out16((NUM_ROWS, dim), kx)
        glx.aggregate_weighted_backward_x(op, d_rows, d_w, d_cnt, go.t, NUM_ROWS, out=gx.t)
        assert np.array_equal(gx.bits(), want), (kg, kx)
        assert gx.guards_intact() and go.guards_intact(), (kg, kx)


@pytest.mark.parametrize("side,repeat", [(0, 3), (1, 1)])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_pair_dot_backward_at_every_offset(dim, heads, side, repeat):
    rng = np.random.default_rng(dim * 8 + heads + side)
    n_self, n_other, B = 11, 13, 10
    codes, xf = _table(rng, (n_other, dim))
    own = rng.integers(-1, n_self + 1, B if side == 0 else B * repeat).astype(np.int64)
    own[-1] = n_self - 1  # the last row, next to the guard, has a list
    other = rng.integers(-1, n_other + 1, B * repeat if side == 0 else B).astype(np.int64)
    ia, ib = (own, other) if side == 0 else (other, own)
    g = rng.standard_normal((B * repeat, heads)).astype(np.float32)
    d_ia, d_ib, d_g = _cuda(ia), _cuda(ib), _cuda(g)
    kw = dict(repeat=repeat, default_attr=0.25)
    aligned = _out16((n_self, dim), 0)
    glx.pair_dot_backward(side, d_ia, d_ib, d_g, Placed(codes, 0).t, n_self, out=aligned.t, **kw)
    want = aligned.bits()
    gs32 = glx.pair_dot_backward(side, d_ia, d_ib, d_g, _cuda(xf), n_self, **kw).cpu().numpy()
    assert np.array_equal(want, b16.to_bf16(gs32))
    assert np.array_equal(want, b16.to_bf16(pref.backward(side, ia, ib, g, xf, n_self, repeat, 0.25)))
    # x_other alone, grad_self alone, both
    for ko, ks in [(1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 1), (4, 4), (4, 1), (3, 4)]:
        x, gs = Placed(codes, ko), _out16((n_self, dim), ks)
        glx.pair_dot_backward(side, d_ia, d_ib, d_g, x.t, n_self, out=gs.t, **kw)
        assert np.array_equal(gs.bits(), want), (ko, ks)
        assert gs.guards_intact() and x.guards_intact(), (ko, ks)


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim", [d for d, _ in SHAPES])
def test_aggregate_backward_at_every_offset(dim, op):
    op = OPS[op]
    rng = np.random.default_rng(dim)
    rows = rng.integers(-1, NUM_ROWS + 1, N).astype(np.int64)
    rows[-1] = NUM_ROWS - 1
    arg = None
    if op in (ref.MAX, ref.MIN):  # small integers: ties everywhere, so arg matters
        grad_out = rng.integers(-3, 4, (S, dim)).astype(np.float32) + np.float32(2.0 ** -9)
        X = rng.integers(-2, 3, (NUM_ROWS, dim)).astype(np.float32)
        arg = ref.fold_arg(op, X, rows, np.minimum(ref.segment_starts(CNT, N, S), N))[1]
    else:
        grad_out = rng.standard_normal((S, dim)).astype(np.float32)
    d_rows, d_cnt = _cuda(rows), _cuda(CNT)
    aligned = _out16((NUM_ROWS, dim), 0)
    glx.aggregate_backward(op, d_rows, d_cnt, _cuda(grad_out), NUM_ROWS, arg=_cuda(arg), out=aligned.t)
    want = aligned.bits()
    gx32 = glx.aggregate_backward(op, d_rows, d_cnt, _cuda(grad_out), NUM_ROWS, arg=_cuda(arg)).cpu().numpy()
    assert np.array_equal(want, b16.to_bf16(gx32))
    assert np.array_equal(want, b16.to_bf16(ref.backward(op, rows, CNT, grad_out, NUM_ROWS, arg)))
    assert want.any() and aligned.guards_intact()
    # grad_x alone, grad_out alone, arg alone (Max / Min), all together
    for kg, kx, ka in [(0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0), (1, 0, 0), (0, 0, 1), (0, 4, 1), (1, 1, 1),
                       (1, 4, 1)]:
        if ka and arg is None:
            continue
        go, gx = Placed(grad_out, kg), _out16((NUM_ROWS, dim), kx)
        at = None if arg is None else Placed(arg, ka)
        glx.aggregate_backward(op, d_rows, d_cnt, go.t, NUM_ROWS, arg=None if at is None else at.t, out=gx.t)
        assert np.array_equal(gx.bits(), want), (kg, kx, ka)
        assert gx.guards_intact() and go.guards_intact(), (kg, kx, ka)


# ---- tree kernels: the alignment class decides the bits --------------------------------------------------------------
def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _classes_differ(dim, heads, vec, scalar):
    """the precondition that keeps the class tests honest: on this data the float32 kernel's two paths differ in at
    least one bit; at C % 4 != 0 there is one path"""
    if (dim // heads) % 4 == 0:
        assert not np.array_equal(vec, scalar), "pick another seed: both float32 paths give the same bits"
    else:
        assert np.array_equal(vec, scalar)


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_grad_w_takes_the_float32_calls_alignment_class(dim, heads, op):
    op = OPS[op]
    codes, xf, rows, _, grad_out = _weighted_request(dim, heads)
    d_rows, d_cnt, d_go = _cuda(rows), _cuda(CNT), _cuda(grad_out)

    def call(x, go):
        return _bits(glx.aggregate_weighted_backward_w(op, x, d_rows, heads, d_cnt, go, default_attr=0.25))

    vec = call(_cuda(xf), d_go)  # float32, everything 16-byte aligned
    scalar = call(Placed(xf, 1).t, d_go)  # float32, the table 4 bytes off
    _classes_differ(dim, heads, vec, scalar)
    want, bound = wref.backward_w(op, xf, rows, heads, CNT, grad_out, 0.25)
    for k in range(5):
        got = call(Placed(codes, k).t, d_go)
        assert np.array_equal(got, vec if k in (0, 4) else scalar), k
        assert wref.within_bound(got.view(np.float32), want, bound), k
    # grad_out 4 bytes off: the scalar class wherever the table is
    for k in (0, 1, 4):
        assert np.array_equal(call(Placed(codes, k).t, Placed(grad_out, 1).t), scalar), k


@pytest.mark.parametrize("repeat", [1, 3])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_pair_dot_takes_the_float32_calls_alignment_class(dim, heads, repeat):
    rng = np.random.default_rng(dim * 8 + heads + repeat)
    na, nb, B = 11, 13, 10
    ca, xa = _table(rng, (na, dim), spread=6)
    cb, xb = _table(rng, (nb, dim), spread=6)
    ia = rng.integers(-1, na + 1, B).astype(np.int64)
    ib = rng.integers(-1, nb + 1, B * repeat).astype(np.int64)
    d_ia, d_ib = _cuda(ia), _cuda(ib)

    def call(ta, tb):
        return _bits(glx.pair_dot(ta, d_ia, tb, d_ib, heads=heads, repeat=repeat, default_attr=0.25))

    vec = call(_cuda(xa), _cuda(xb))
    scalar = call(Placed(xa, 1).t, Placed(xb, 1).t)
    _classes_differ(dim, heads, vec, scalar)
    assert np.array_equal(call(Placed(xa, 1).t, _cuda(xb)), scalar)  # one float32 table off is the scalar class too
    want, bound = pref.forward(xa, ia, xb, ib, heads, repeat, 0.25)
    for ka, kb in [(0, 0), (4, 4), (0, 4), (4, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 2), (4, 1), (1, 4), (3, 4)]:
        got = call(Placed(ca, ka).t, Placed(cb, kb).t)
        assert np.array_equal(got, vec if ka % 4 == 0 and kb % 4 == 0 else scalar), (ka, kb)
        assert pref.within_bound(got.view(np.float32), want, bound), (ka, kb)


# ---- host pointers: staging re-aligns them ---------------------------------------------------------------------------
def _host_at(a, k, output=False):
    """(a numpy view 8 + k elements into a larger buffer of guard codes, the buffer); the view holds `a`'s values, or
    the guard code too for an output"""
    a = np.ascontiguousarray(a)
    base = np.full(a.size + 16, GUARD16, a.dtype)
    view = base[8 + k:8 + k + a.size].reshape(a.shape)
    if not output:
        view[...] = a
    return view, base


@pytest.mark.parametrize("k", [1, 4])
def test_host_codes_at_an_offset_give_the_aligned_device_calls_bits(k):
    dim, heads = 48, 4
    codes, xf, rows, w, grad_out = _weighted_request(dim, heads)
    rng = np.random.default_rng(1)
    ia = rng.integers(-1, NUM_ROWS + 1, 10).astype(np.int64)
    ib = rng.integers(-1, NUM_ROWS + 1, 30).astype(np.int64)
    g = rng.standard_normal((30, heads)).astype(np.float32)
    tab, dev = _host_at(codes, k)[0], Placed(codes, 0).t
    assert tab.flags["C_CONTIGUOUS"] and tab.ctypes.data % 4 == (2 * k) % 4
    d = _cuda
    pairs = [
        (glx.aggregate_weighted(wref.MEAN, tab, rows, w, S, cnt=CNT, default_attr=0.25),
         glx.aggregate_weighted(wref.MEAN, dev, d(rows), d(w), S, cnt=d(CNT), default_attr=0.25)),
        (glx.aggregate_weighted_backward_w(wref.MEAN, tab, rows, heads, CNT, grad_out, default_attr=0.25),
         glx.aggregate_weighted_backward_w(wref.MEAN, dev, d(rows), heads, d(CNT), d(grad_out), default_attr=0.25)),
        (glx.pair_dot(tab, ia, tab, ib, heads=heads, repeat=3, default_attr=0.25),
         glx.pair_dot(dev, d(ia), dev, d(ib), heads=heads, repeat=3, default_attr=0.25)),
    ]
    for j, (host, device) in enumerate(pairs):
        assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), _bits(device)), j
    # the three row gradients into host buffers at the same offset, guard codes around them
    outs = []
    for _ in range(3):
        outs.append(_host_at(np.zeros((NUM_ROWS, dim), np.uint16), k, output=True))
    glx.aggregate_backward(ref.MEAN, rows, CNT, grad_out, NUM_ROWS, out=outs[0][0])
    glx.aggregate_weighted_backward_x(wref.MEAN, rows, w, CNT, grad_out, NUM_ROWS, out=outs[1][0])
    glx.pair_dot_backward(1, ia, ib, g, tab, NUM_ROWS, repeat=3, default_attr=0.25, out=outs[2][0])
    want = [
        glx.aggregate_backward(ref.MEAN, d(rows), d(CNT), d(grad_out), NUM_ROWS, out_dtype="bfloat16"),
        glx.aggregate_weighted_backward_x(wref.MEAN, d(rows), d(w), d(CNT), d(grad_out), NUM_ROWS,
                                          out_dtype="bfloat16"),
        glx.pair_dot_backward(1, d(ia), d(ib), d(g), dev, NUM_ROWS, repeat=3, default_attr=0.25),
    ]
    import torch
    for j, ((view, base), device) in enumerate(zip(outs, want)):
        assert np.array_equal(view, device.view(torch.int16).cpu().numpy().view(np.uint16)), j
        assert view.any() and (base[:8 + k] == GUARD16).all() and (base[8 + k + view.size:] == GUARD16).all(), j
