"""glx_pair_dot and glx_pair_dot_backward on the GPU against the numpy restatement of the contracts (pair_dot_ref.py).
The forward within its derived bound of the float64 value, bit-identical between two calls and between host and device
pointers; the backward at tolerance 0 (bit equality, the sign of zero included; a NaN matches a NaN)."""
import numpy as np
import pytest

import glx
import pair_dot_ref as pref

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)


def _cuda(a, offset=False):
    """a CUDA copy of `a`; offset: 4 bytes into its buffer, so that it is not 16-byte aligned"""
    import torch
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a).cuda()
    assert a.dtype == np.float32
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def gpu_all(xa, ia, xb, ib, g, heads, repeat, default_attr=0.0, host=False, offset=False, same=False):
    """(out, out of a second call, grad_a, grad_b) as numpy; every output buffer starts as a NaN canary.  same: xa and
    xb are one buffer (xb is ignored)"""
    n, (na, D), nb = ib.size, xa.shape, (xa if same else xb).shape[0]
    kw = dict(repeat=repeat, default_attr=default_attr)
    if host:
        xb = xa if same else xb
        out = [np.full((n, heads), NAN, np.float32) for _ in range(2)]
        ga, gb = np.full((na, D), NAN, np.float32), np.full((nb, D), NAN, np.float32)
        for o in out:
            glx.pair_dot(xa, ia, xb, ib, heads=heads, out=o, **kw)
        glx.pair_dot_backward(0, ia, ib, g, xb, na, out=ga, **kw)
        glx.pair_dot_backward(1, ia, ib, g, xa, nb, out=gb, **kw)
        return out[0], out[1], ga, gb
    dxa = _cuda(xa, offset)
    dxb = dxa if same else _cuda(xb, offset)
    dia, dib, dg = _cuda(ia), _cuda(ib), _cuda(g)
    out = [_cuda(np.full((n, heads), NAN, np.float32)) for _ in range(2)]
    ga, gb = _cuda(np.full((na, D), NAN, np.float32), offset), _cuda(np.full((nb, D), NAN, np.float32), offset)
    for o in out:
        glx.pair_dot(dxa, dia, dxb, dib, heads=heads, out=o, **kw)
    glx.pair_dot_backward(0, dia, dib, dg, dxb, na, out=ga, **kw)
    glx.pair_dot_backward(1, dia, dib, dg, dxa, nb, out=gb, **kw)
    return tuple(t.cpu().numpy() for t in (out[0], out[1], ga, gb))


def check(xa, ia, xb, ib, g, heads, repeat, default_attr=0.0, host=False, offset=False, same=False):
    """one request through both entry points (both sides of the backward) and the restatement"""
    out, out2, ga, gb = gpu_all(xa, ia, xb, ib, g, heads, repeat, default_attr, host, offset, same)
    xb = xa if same else xb
    want, bound = pref.forward(xa, ia, xb, ib, heads, repeat, default_attr)
    want_ga = pref.backward(0, ia, ib, g, xb, xa.shape[0], repeat, default_attr)
    want_gb = pref.backward(1, ia, ib, g, xa, xb.shape[0], repeat, default_attr)
    assert np.array_equal(np.isnan(out), np.isnan(want)), "an element of out was not written"
    assert pref.within_bound(out, want, bound)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "out differs between two calls"
    assert np.array_equal(np.isnan(ga), np.isnan(want_ga)), "an element of grad_a was not written"
    assert pref.same_bits(ga, want_ga)
    assert np.array_equal(np.isnan(gb), np.isnan(want_gb)), "an element of grad_b was not written"
    assert pref.same_bits(gb, want_gb)
    return out, ga, gb


def _data(seed, na, nb, D, n, heads):
    rng = np.random.default_rng(seed)
    xa = rng.standard_normal((na, D)).astype(np.float32)
    xb = rng.standard_normal((nb, D)).astype(np.float32)
    g = rng.standard_normal((n, heads)).astype(np.float32)
    if n:
        g[0, 0] = -0.0
    return xa, xb, g


def _indices(seed, na, nb, n, repeat):
    """ia[n / repeat], ib[n] with -1 and the table's size among them"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1, na + 1, n // repeat).astype(np.int64), rng.integers(-1, nb + 1, n).astype(np.int64))


DIMS = (1, 3, 4, 20, 64, 100, 256, 260)
# + (512, 1): a head that spans two column tiles of the 64-lane group (the sub-group mapping's `steps` loop)
SHAPES = sorted({(d, h) for d in DIMS for h in (1, 2, 4, d) if d % h == 0} | {(512, 1)})


@pytest.mark.parametrize("dim, heads", SHAPES)
def test_every_dimension_path_from_host_and_device_pointers(dim, heads):
    """VEC 4 (C % 4 == 0) and 1; the sub-group mapping (C / VEC a power of two) and the loop over heads; every group
    size 8 .. 64; 260 and 100 / 100: more columns than one tile.  The same bits from numpy and from CUDA buffers."""
    assert (260, 1) in SHAPES and (20, 20) in SHAPES and (3, 1) in SHAPES and (100, 4) in SHAPES
    na, nb, repeat, n = 6, 9, 5, 20
    xa, xb, g = _data(dim * 8 + heads, na, nb, dim, n, heads)
    ia, ib = _indices(dim + heads, na, nb, n, repeat)
    out, ga, gb = check(xa, ia, xb, ib, g, heads, repeat, default_attr=0.25)
    host = gpu_all(xa, ia, xb, ib, g, heads, repeat, default_attr=0.25, host=True)
    assert np.array_equal(out.view(np.uint32), host[0].view(np.uint32)), "host and device pointers differ"
    assert pref.same_bits(ga, host[2]) and pref.same_bits(gb, host[3])


@pytest.mark.parametrize("dim, heads", [(64, 2), (256, 1), (20, 1)])
def test_misaligned_tables_take_the_scalar_path(dim, heads):
    """x one float into its buffer: VEC = 1 at dim % 4 == 0; the backward's bits do not depend on the path"""
    na, nb, repeat, n = 7, 5, 1, 33
    xa, xb, g = _data(dim + 3, na, nb, dim, n, heads)
    ia, ib = _indices(dim, na, nb, n, repeat)
    aligned = gpu_all(xa, ia, xb, ib, g, heads, repeat)
    out, ga, gb = check(xa, ia, xb, ib, g, heads, repeat, offset=True)
    assert pref.same_bits(ga, aligned[2]) and pref.same_bits(gb, aligned[3])


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("repeat", [1, 5])
@pytest.mark.parametrize("num_pairs", [0, 1, 65, 130])
def test_pair_counts_at_the_workgroup_edges(num_pairs, repeat, host):
    """dim 4: G = 8, 32 groups per workgroup -- one pair, one past two workgroups, two past four (repeat 5: the counts
    become the next multiples 0, 5, 65, 130)"""
    n = -(-num_pairs // repeat) * repeat
    na, nb = 9, 70  # grad_b: three workgroups of rows
    xa, xb, g = _data(n + repeat, na, nb, 4, n, 1)
    ia, ib = _indices(n, na, nb, n, repeat)
    out, ga, gb = check(xa, ia, xb, ib, g, 1, repeat, default_attr=0.5, host=host)
    if n == 0:
        assert not ga.any() and not gb.any() and not np.signbit(ga).any()  # +0.0 everywhere


@pytest.mark.parametrize("same", [False, True], ids=["two_tables", "one_table"])
@pytest.mark.parametrize("dim, heads", [(4, 1), (100, 4), (64, 2)])
def test_own_side_list_lengths_at_the_launch_edges(dim, heads, same):
    """rows referenced 0, 1, 63, 64, 65 and 130 times on either side (repeat = 1): the group width and the loads in
    flight; xa and xb distinct, and one buffer"""
    lengths = [0, 1, 63, 64, 65, 130]
    rng = np.random.default_rng(3)
    ia = np.repeat(np.arange(len(lengths)), lengths).astype(np.int64)
    ib = ia.copy()
    rng.shuffle(ia)
    rng.shuffle(ib)
    xa, xb, g = _data(dim + 1, len(lengths), len(lengths), dim, len(ia), heads)
    out, ga, gb = check(xa, ia, xb, ib, g, heads, 1, same=same)
    assert not ga[0].any() and not np.signbit(ga[0]).any() and not gb[0].any()  # nobody refers to row 0: +0.0


@pytest.mark.parametrize("side_repeat", [1, 5])
def test_a_hub_row_referenced_5000_times(side_repeat):
    """one lane group walks the hub's whole list: 5,000 pairs on each side (repeat 5: 1,000 entries of ia)"""
    n, na, nb, D, heads = 5000, 4, 6, 8, 2
    rng = np.random.default_rng(11)
    ia = np.full(n // side_repeat, 2, np.int64)
    ib = np.full(n, 3, np.int64)
    ib[::7] = rng.integers(0, nb, len(ib[::7]))  # the hub's factors are not all one row
    ia[::9] = rng.integers(0, na, len(ia[::9]))
    xa, xb, g = _data(5, na, nb, D, n, heads)
    check(xa, ia, xb, ib, g, heads, side_repeat)


def test_repeated_source_entries_interleave_with_another_rows():
    """side 0, repeat 5: ia = [1, 2, 1, 2, 1] -- row 1's pairs are 0..4, 10..14, 20..24, row 2's lie between them; the
    order of the adds is ascending p for each"""
    ia = np.array([1, 2, 1, 2, 1, 0, 2], np.int64)
    rng = np.random.default_rng(2)
    ib = rng.integers(0, 6, 35).astype(np.int64)
    xa, xb, g = _data(8, 3, 6, 20, 35, 2)
    # mixed magnitudes: another order of the adds would change bits
    g *= (10.0 ** rng.integers(-3, 4, g.shape)).astype(np.float32)
    out, ga, gb = check(xa, ia, xb, ib, g, 2, 5)
    shuffled = pref.backward(0, ia[::-1].copy(), ib.reshape(7, 5)[::-1].reshape(-1).copy(),
                             g.reshape(7, 5, 2)[::-1].reshape(35, 2).copy(), xb, 3, 5)
    assert not pref.same_bits(ga, shuffled), "the case cannot tell one order of the adds from another"


@pytest.mark.parametrize("case", ["own", "other", "both"])
@pytest.mark.parametrize("repeat", [1, 5])
def test_indices_outside_their_tables(repeat, case):
    """-1 and num_rows on each side, alone and together: the own side gets no gradient, the other side reads
    default_attr = 0.5"""
    na, nb, D, heads, B = 5, 6, 8, 2, 6
    n = B * repeat
    rng = np.random.default_rng(31 + repeat)
    ia = rng.integers(0, na, B).astype(np.int64)
    ib = rng.integers(0, nb, n).astype(np.int64)
    if case in ("own", "both"):   # seen from side 0; side 1 sees the same entries as the other side's
        ia[0], ia[3] = -1, na
    if case in ("other", "both"):
        ib[0], ib[n - 1], ib[3 * repeat] = -1, nb, nb  # pair 0 and pair 3 * repeat: both sides outside when "both"
    xa, xb, g = _data(41, na, nb, D, n, heads)
    out, ga, gb = check(xa, ia, xb, ib, g, heads, repeat, default_attr=0.5)
    if case == "both":
        assert np.all(out[0] == np.float32(0.25 * D / heads))  # default row times default row
    # with default_attr = 0 the outside entries contribute exactly nothing to the other side either
    check(xa, ia, xb, ib, g, heads, repeat, default_attr=0.0)


def test_non_finite_and_signed_zero_rows():
    """NaN, +-inf and -0.0 rows: the IEEE result going forward (inf * 0 = NaN), bit for bit going back"""
    na, nb, D, heads, repeat = 5, 5, 8, 2, 2
    rng = np.random.default_rng(43)
    xa, xb, g = _data(43, na, nb, D, 12, heads)
    xa[0, :4], xa[1, 4:], xa[2], xa[3, 0] = np.nan, np.inf, -0.0, -np.inf
    xb[0], xb[1, :4], xb[2, 2], xb[3, 5] = -0.0, 0.0, np.inf, np.nan
    ia = np.array([0, 1, 2, 3, 4, 2], np.int64)
    ib = rng.integers(0, nb, 12).astype(np.int64)
    ib[:8] = [0, 1, 0, 2, 0, 4, 2, 3]
    g[5] = -0.0
    g[6, 0] = np.inf
    out, ga, gb = check(xa, ia, xb, ib, g, heads, repeat)
    assert np.isnan(out[0, 0]) and np.isnan(out[2, 1])  # a NaN row; inf * -0.0
    assert np.isnan(ga).any() and np.isnan(gb).any()


def test_every_row_of_grad_self_is_written_over_a_sentinel():
    """out= pre-filled with a finite sentinel: rows nobody refers to, and rows only an outside index would reach, are
    +0.0 afterwards; num_pairs == 0 writes zeros"""
    import torch
    na, nb, D = 300, 200, 12
    xa, xb, g = _data(7, na, nb, D, 10, 1)
    ia = np.array([3, -1, 299, 3, na], np.int64)
    ib = np.array([0, 199, 5, nb, -1, 5, 5, 0, 7, 7], np.int64)
    for side, own_n, x_other in ((0, na, xb), (1, nb, xa)):
        out = torch.full((own_n, D), 12345.0, device="cuda")
        glx.pair_dot_backward(side, _cuda(ia), _cuda(ib), _cuda(g), _cuda(x_other), own_n, repeat=2, out=out)
        got = out.cpu().numpy()
        assert not (got == 12345.0).any()
        assert pref.same_bits(got, pref.backward(side, ia, ib, g, x_other, own_n, 2))
        none = torch.zeros(0, dtype=torch.int64, device="cuda")
        out.fill_(12345.0)
        glx.pair_dot_backward(side, none, none, torch.zeros((0, 1), device="cuda"), _cuda(x_other), own_n, out=out)
        assert pref.same_bits(out.cpu().numpy(), np.zeros((own_n, D), np.float32))


def test_bad_arguments_are_refused_on_the_device_too():
    import torch
    x = torch.ones((3, 4), device="cuda")
    ia = torch.zeros(2, dtype=torch.int64, device="cuda")
    ib = torch.zeros(6, dtype=torch.int64, device="cuda")
    with pytest.raises(glx.GlxError) as e:
        glx.pair_dot(x, ia, x, ib, heads=3, repeat=3)
    assert e.value.code == 3 and "heads" in str(e.value)
    with pytest.raises(glx.GlxError) as e:
        glx.pair_dot_backward(2, ia, ib, torch.ones((6, 1), device="cuda"), x, 3, repeat=3)
    assert e.value.code == 3 and "side" in str(e.value)
