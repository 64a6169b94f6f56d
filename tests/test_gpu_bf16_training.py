"""The bfloat16 training path at engine level: the six _ex entry points through glx.py's wrappers.

Every comparison is to the bit.  A bfloat16 row gradient has two oracles and must equal both: the float32 entry point's
answer on the same arguments pushed through glx_features_convert_host, and the numpy restatement converted the same
way.  A float32 output of a bfloat16 table must equal the float32 entry point on the upcast table, and the restatement
(bit for bit for the folds; within the restatement's own bound for the two tree kernels)."""
import numpy as np
import pytest

import agg_backward_ref as ref
import agg_weighted_ref as wref
import bf16_training_ref as b16
import glx
import pair_dot_ref as pref

pytestmark = pytest.mark.gpu

OPS = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}
GUARD = 0x1234
# C % 4 != 0 (VEC 1); C / VEC = 3 (not a power of two: the loop over heads); sub-groups; a head spanning several tiles
HEAD_SHAPES = [(6, 2), (12, 1), (16, 4), (48, 4), (256, 4)]


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cuda_bf16(codes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(codes).view(np.int16)).cuda().view(torch.bfloat16)


def _codes(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _table(rng, shape):
    """(uint16 codes, the float32 matrix of exactly those values)"""
    codes = b16.to_bf16(rng.standard_normal(shape).astype(np.float32))
    return codes, b16.upcast(codes)


# ---- glx_aggregate_backward_ex: every launch path ---------------------------------------------------------------------
NUM_ROWS, HUB, ABSENT = 40, 7, (3, 17, 39)


def _positions():
    """200 positions over rows [-1, 40]: row 7 referenced 150 times (its list spans several coalesced fetch rounds of
    every group width), rows 3, 17 and 39 by nobody, -1 and 40 outside the table"""
    rng = np.random.default_rng(5)
    pool = np.array([r for r in range(-1, NUM_ROWS + 1) if r not in ABSENT and r != HUB], np.int64)
    rows = np.concatenate([np.full(150, HUB, np.int64), rng.choice(pool, 50)])
    rows[150:152] = (-1, NUM_ROWS)
    rng.shuffle(rows)
    return rows


ROWS = _positions()
_TAIL = np.array([0, 9, 0, 31, 4, 0, 70, 1, 0, 25, 40, 0], np.int32)  # sums to 180: a tail of 20 is never consumed
_OVER = np.array([0, 9, 0, 31, 4, 0, 70, 1, 0, 25, 40, 90], np.int32)  # the last count promises 90, 20 remain
LAYOUTS = {"implied": (None, 40), "ragged_tail": (_TAIL, 12), "ragged_over": (_OVER, 12)}


def _agg_request(op, layout, dim):
    cnt, S = LAYOUTS[layout]
    rng = np.random.default_rng(dim)
    arg = None
    if op in (ref.MAX, ref.MIN):  # small integers: ties everywhere, so arg matters
        grad_out = rng.integers(-3, 4, (S, dim)).astype(np.float32)
        X = rng.integers(-2, 3, (NUM_ROWS, dim)).astype(np.float32)
        start = np.minimum(ref.segment_starts(cnt, len(ROWS), S), len(ROWS))
        arg = ref.fold_arg(op, X, ROWS, start)[1]
    else:
        grad_out = rng.standard_normal((S, dim)).astype(np.float32)
        grad_out[0, 0] = -0.0
    return cnt, grad_out, arg


def _agg_bwd(op, rows, cnt, grad_out, num_rows, arg, dtype):
    import torch
    out = torch.full((num_rows, grad_out.shape[1]), float("nan"), dtype=getattr(torch, dtype), device="cuda")
    got = glx.aggregate_backward(op, _cuda(rows), _cuda(cnt), _cuda(grad_out), num_rows, arg=_cuda(arg), out=out)
    assert got is out
    return out


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim", [1, 5, 12, 32, 36, 256, 260])
def test_aggregate_backward_every_launch_path(dim, op, layout):
    """dims: VEC 1 (1, 5) and 4; groups of 8 (12, 32), 16 (36) and 64 (256); a second column tile (260); 12 and 36
    leave lanes past the last column in the group"""
    cnt, grad_out, arg = _agg_request(OPS[op], layout, dim)
    got = _codes(_agg_bwd(OPS[op], ROWS, cnt, grad_out, NUM_ROWS, arg, "bfloat16"))
    f32 = _agg_bwd(OPS[op], ROWS, cnt, grad_out, NUM_ROWS, arg, "float32").cpu().numpy()
    want = ref.backward(OPS[op], ROWS, cnt, grad_out, NUM_ROWS, arg)
    assert ref.same_bits(f32, want)
    assert np.array_equal(got, b16.to_bf16(f32))
    assert np.array_equal(got, b16.to_bf16(want))
    assert not got[list(ABSENT)].any()  # rows nobody references: all bits clear
    assert got[HUB].any()


def test_one_rounding_of_the_float32_sum():
    """every row receives the terms of one ROUNDING_CASES entry: ties to even both ways, a sum a bfloat16 accumulator
    would lose, the overflow threshold, inf, NaN -> 0xFFFF, a bfloat16 subnormal, and +0.0 + -0.0"""
    rows, vals = [], []
    for r, (terms, _) in enumerate(b16.ROUNDING_CASES):
        rows += [r] * len(terms)
        vals += terms
    rows = np.array(rows, np.int64)
    grad_out = np.repeat(np.array(vals, np.float32)[:, None], 4, axis=1)  # one position per segment
    num_rows = len(b16.ROUNDING_CASES) + 1
    got = _codes(_agg_bwd(ref.SUM, rows, None, grad_out, num_rows, None, "bfloat16"))
    want = np.repeat(np.array([c for _, c in b16.ROUNDING_CASES] + [0], np.uint16)[:, None], 4, axis=1)
    assert np.array_equal(got, want), [hex(v) for v in got[:, 0]]
    f32 = _agg_bwd(ref.SUM, rows, None, grad_out, num_rows, None, "float32").cpu().numpy()
    assert np.array_equal(got, b16.to_bf16(f32))
    assert wref.same_bits(f32[:-1, 0], b16.rounding_sums())


# ---- nothing is written outside the buffer's own elements ---------------------------------------------------------------
def _guarded(num_rows, dim, pad=3):
    import torch
    big = torch.full((num_rows + pad, dim), GUARD, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return big, big[:num_rows]


def _guard_ok(big, num_rows):
    return bool((_codes(big)[num_rows:] == GUARD).all())


BOUND_CASES = ["empty", "more_segments_than_ids", "ordinary"]


def _bound_request(case, dim, heads=1):
    rng = np.random.default_rng(dim)
    if case == "empty":
        n, S = 0, 4
    elif case == "more_segments_than_ids":
        n, S = 3, 4  # the implied layout's fan-out is 0: nothing is consumed
    else:
        n, S = 12, 4
    rows = rng.integers(0, 9, n).astype(np.int64)
    if n == 12:
        rows[-1] = 8  # the last row, next to the guard, has a list
    return rows, rng.standard_normal((S, dim)).astype(np.float32), rng.standard_normal((n, heads)).astype(np.float32)


@pytest.mark.parametrize("case", BOUND_CASES)
@pytest.mark.parametrize("dim", [5, 12, 36])
def test_aggregate_backward_stays_inside_a_bf16_buffer(dim, case):
    rows, grad_out, _ = _bound_request(case, dim)
    big, out = _guarded(9, dim)
    glx.aggregate_backward(ref.SUM, _cuda(rows), None, _cuda(grad_out), 9, out=out)
    assert _guard_ok(big, 9)
    got = _codes(big)[:9]
    if case == "ordinary":
        assert np.array_equal(got, b16.to_bf16(ref.backward(ref.SUM, rows, None, grad_out, 9)))
    else:
        assert not got.any()


@pytest.mark.parametrize("case", BOUND_CASES)
@pytest.mark.parametrize("dim,heads", [(6, 2), (12, 1), (36, 1)])
def test_weighted_backward_x_stays_inside_a_bf16_buffer(dim, heads, case):
    rows, grad_out, w = _bound_request(case, dim, heads)
    big, out = _guarded(9, dim)
    glx.aggregate_weighted_backward_x(wref.SUM, _cuda(rows), _cuda(w), None, _cuda(grad_out), 9, out=out)
    assert _guard_ok(big, 9)
    got = _codes(big)[:9]
    if case == "ordinary":
        assert np.array_equal(got, b16.to_bf16(wref.backward_x(wref.SUM, rows, w, None, grad_out, 9)))
    else:
        assert not got.any()


@pytest.mark.parametrize("case", ["empty", "every_own_index_outside", "ordinary"])
@pytest.mark.parametrize("dim,heads", [(6, 2), (12, 1), (36, 1)])
def test_pair_dot_backward_stays_inside_a_bf16_buffer(dim, heads, case):
    rng = np.random.default_rng(dim)
    n = 0 if case == "empty" else 12
    ia = rng.integers(0, 9, n).astype(np.int64)
    ib = rng.integers(0, 7, n).astype(np.int64)
    if case == "every_own_index_outside":
        ia[:] = np.where(np.arange(n) % 2 == 0, -1, 9)
    elif n:
        ia[-1] = 8
    g = rng.standard_normal((n, heads)).astype(np.float32)
    codes, xf = _table(rng, (7, dim))
    big, out = _guarded(9, dim)
    glx.pair_dot_backward(0, _cuda(ia), _cuda(ib), _cuda(g), _cuda_bf16(codes), 9, out=out)
    assert _guard_ok(big, 9)
    got = _codes(big)[:9]
    if case == "ordinary":
        assert np.array_equal(got, b16.to_bf16(pref.backward(0, ia, ib, g, xf, 9)))
    else:
        assert not got.any()


def test_element_offsets_past_2_to_the_31():
    """a bfloat16 grad_x of 2^23 + 1 rows at dim 256 is just over 2^31 elements (4 GiB): the last row's offset needs 64
    bits"""
    import torch
    num_rows, dim = 2 ** 23 + 1, 256
    rows = np.array([0, num_rows - 1, 2 ** 22 + 5], np.int64)
    grad_out = np.random.default_rng(0).standard_normal((3, dim)).astype(np.float32)
    grad_out[grad_out == 0] = 1.0
    out = glx.aggregate_backward(ref.SUM, _cuda(rows), None, _cuda(grad_out), num_rows, out_dtype="bfloat16")
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (num_rows, dim)
    want = b16.to_bf16(grad_out)
    assert want.all()
    for k, r in enumerate(rows):
        assert np.array_equal(_codes(out[int(r)]), want[k]), r
    assert int(torch.count_nonzero(out.view(torch.int16))) == 3 * dim


# ---- the weighted ops with a bfloat16 x ---------------------------------------------------------------------------------
W_ROWS, W_N, W_S = 20, 60, 12
W_CNT = np.array([0, 9, 0, 7, 4, 0, 11, 1, 0, 5, 6, 30], np.int32)  # zeros; the last count is cut at num_ids


def _weighted_request(dim, heads, ragged):
    rng = np.random.default_rng(dim * 8 + heads)
    codes, xf = _table(rng, (W_ROWS, dim))
    rows = rng.integers(-1, W_ROWS + 1, W_N).astype(np.int64)
    rows[:2] = (-1, W_ROWS)  # both read a row of default_attr
    w = rng.standard_normal((W_N, heads)).astype(np.float32)
    grad_out = rng.standard_normal((W_S, dim)).astype(np.float32)
    return codes, xf, rows, w, grad_out, (W_CNT if ragged else None)


@pytest.mark.parametrize("ragged", [False, True], ids=["implied", "ragged"])
@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("dim,heads", HEAD_SHAPES)
def test_weighted_ops_with_a_bf16_table(dim, heads, op, ragged):
    op = OPS[op]
    codes, xf, rows, w, grad_out, cnt = _weighted_request(dim, heads, ragged)
    xb, x32 = _cuda_bf16(codes), _cuda(xf)
    d_rows, d_w, d_cnt, d_go = _cuda(rows), _cuda(w), _cuda(cnt), _cuda(grad_out)
    # forward: float32 out, the float32 call's bits
    emb = glx.aggregate_weighted(op, xb, d_rows, d_w, W_S, cnt=d_cnt, default_attr=0.25)
    emb32 = glx.aggregate_weighted(op, x32, d_rows, d_w, W_S, cnt=d_cnt, default_attr=0.25)
    assert str(emb.dtype) == "torch.float32" and np.array_equal(_bits(emb), _bits(emb32))
    assert wref.same_bits(emb.cpu().numpy(), wref.forward(op, xf, rows, w, cnt, W_S, 0.25))
    # grad_w: float32 out, the float32 call's bits (the same plan and tree), inside the restatement's bound
    gw = glx.aggregate_weighted_backward_w(op, xb, d_rows, heads, d_cnt, d_go, default_attr=0.25)
    gw32 = glx.aggregate_weighted_backward_w(op, x32, d_rows, heads, d_cnt, d_go, default_attr=0.25)
    assert str(gw.dtype) == "torch.float32" and np.array_equal(_bits(gw), _bits(gw32))
    want, bound = wref.backward_w(op, xf, rows, heads, cnt, grad_out, 0.25)
    assert wref.within_bound(gw.cpu().numpy(), want, bound)
    # grad_x: bfloat16 out, the float32 gradient rounded once
    gx = glx.aggregate_weighted_backward_x(op, d_rows, d_w, d_cnt, d_go, W_ROWS, out_dtype="bfloat16")
    gx32 = glx.aggregate_weighted_backward_x(op, d_rows, d_w, d_cnt, d_go, W_ROWS).cpu().numpy()
    assert str(gx.dtype) == "torch.bfloat16"
    assert np.array_equal(_codes(gx), b16.to_bf16(gx32))
    assert np.array_equal(_codes(gx), b16.to_bf16(wref.backward_x(op, rows, w, cnt, grad_out, W_ROWS)))


# ---- pair dot -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeat", [1, 3])
@pytest.mark.parametrize("dim,heads", HEAD_SHAPES)
def test_pair_dot_with_bf16_tables(dim, heads, repeat):
    rng = np.random.default_rng(dim * 8 + heads + repeat)
    na, nb, B = 11, 13, 10
    ca, xa = _table(rng, (na, dim))
    cb, xb = _table(rng, (nb, dim))
    ia = rng.integers(0, na, B).astype(np.int64)
    ib = rng.integers(0, nb, B * repeat).astype(np.int64)
    ia[0], ib[1], ia[2], ib[-1] = -1, nb, na, -5  # an index outside each table
    g = rng.standard_normal((B * repeat, heads)).astype(np.float32)
    d_ia, d_ib, d_g = _cuda(ia), _cuda(ib), _cuda(g)
    ta, tb, fa, fb = _cuda_bf16(ca), _cuda_bf16(cb), _cuda(xa), _cuda(xb)
    out = glx.pair_dot(ta, d_ia, tb, d_ib, heads=heads, repeat=repeat, default_attr=0.25)
    out32 = glx.pair_dot(fa, d_ia, fb, d_ib, heads=heads, repeat=repeat, default_attr=0.25)
    assert str(out.dtype) == "torch.float32" and np.array_equal(_bits(out), _bits(out32))
    want, bound = pref.forward(xa, ia, xb, ib, heads, repeat, 0.25)
    assert pref.within_bound(out.cpu().numpy(), want, bound)
    for side, (other_b, other_f, other_np, n_self) in enumerate([(tb, fb, xb, na), (ta, fa, xa, nb)]):
        gs = glx.pair_dot_backward(side, d_ia, d_ib, d_g, other_b, n_self, repeat=repeat, default_attr=0.25)
        gs32 = glx.pair_dot_backward(side, d_ia, d_ib, d_g, other_f, n_self, repeat=repeat, default_attr=0.25)
        assert str(gs.dtype) == "torch.bfloat16" and str(gs32.dtype) == "torch.float32"
        assert np.array_equal(_codes(gs), b16.to_bf16(gs32.cpu().numpy())), side
        assert np.array_equal(_codes(gs), b16.to_bf16(pref.backward(side, ia, ib, g, other_np, n_self, repeat, 0.25)))


@pytest.mark.parametrize("dim,heads", [(12, 1), (48, 4)])
def test_pair_dot_one_bf16_table_on_both_sides(dim, heads):
    rng = np.random.default_rng(dim)
    codes, xf = _table(rng, (9, dim))
    ia = rng.integers(-1, 10, 8).astype(np.int64)
    ib = rng.integers(-1, 10, 24).astype(np.int64)
    g = rng.standard_normal((24, heads)).astype(np.float32)
    t, f = _cuda_bf16(codes), _cuda(xf)
    out = glx.pair_dot(t, _cuda(ia), t, _cuda(ib), heads=heads, repeat=3)
    assert np.array_equal(_bits(out), _bits(glx.pair_dot(f, _cuda(ia), f, _cuda(ib), heads=heads, repeat=3)))
    for side in (0, 1):
        gs = glx.pair_dot_backward(side, _cuda(ia), _cuda(ib), _cuda(g), t, 9, repeat=3)
        assert np.array_equal(_codes(gs), b16.to_bf16(pref.backward(side, ia, ib, g, xf, 9, 3)))


def test_pair_dot_tables_of_two_dtypes_raise():
    codes, xf = _table(np.random.default_rng(0), (4, 8))
    idx = _cuda(np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        glx.pair_dot(_cuda_bf16(codes), idx, _cuda(xf), idx)
    with pytest.raises(ValueError):
        glx.pair_dot(_cuda(xf), idx, _cuda_bf16(codes), idx)
    with pytest.raises(ValueError):
        glx.pair_dot(_cuda(xf).half(), idx, _cuda(xf).half(), idx)


# ---- host pointers and repeatability ------------------------------------------------------------------------------------
def _six_calls(host):
    """every _ex entry point once on bfloat16 data, host (numpy, uint16 codes) or device pointers -> the outputs as
    numpy arrays of bits"""
    dim, heads = 48, 4
    codes, xf, rows, w, grad_out, cnt = _weighted_request(dim, heads, True)
    rng = np.random.default_rng(1)
    ia = rng.integers(-1, W_ROWS + 1, 10).astype(np.int64)
    ib = rng.integers(-1, W_ROWS + 1, 30).astype(np.int64)
    g = rng.standard_normal((30, heads)).astype(np.float32)
    up = (lambda a: a) if host else _cuda
    tab = codes if host else _cuda_bf16(codes)
    res = [
        glx.aggregate_backward(ref.MEAN, up(rows), up(cnt), up(grad_out), W_ROWS, out_dtype="bfloat16"),
        glx.aggregate_weighted(wref.MEAN, tab, up(rows), up(w), W_S, cnt=up(cnt), default_attr=0.25),
        glx.aggregate_weighted_backward_x(wref.MEAN, up(rows), up(w), up(cnt), up(grad_out), W_ROWS,
                                          out_dtype="bfloat16"),
        glx.aggregate_weighted_backward_w(wref.MEAN, tab, up(rows), heads, up(cnt), up(grad_out), default_attr=0.25),
        glx.pair_dot(tab, up(ia), tab, up(ib), heads=heads, repeat=3, default_attr=0.25),
        glx.pair_dot_backward(1, up(ia), up(ib), up(g), tab, W_ROWS, repeat=3, default_attr=0.25),
    ]
    bits = []
    for k, r in enumerate(res):
        narrow = k in (0, 2, 5)
        if host:
            assert r.dtype == (np.uint16 if narrow else np.float32)
            bits.append(r if narrow else r.view(np.uint32))
        else:
            assert str(r.dtype) == ("torch.bfloat16" if narrow else "torch.float32")
            bits.append(_codes(r) if narrow else _bits(r))
    return bits


def test_host_pointers_equal_device_pointers_and_calls_repeat():
    dev, dev2, host = _six_calls(False), _six_calls(False), _six_calls(True)
    for k in range(6):
        assert dev[k].any()
        assert np.array_equal(dev[k], dev2[k]), k
        assert np.array_equal(dev[k], host[k]), k


def test_host_torch_bf16_buffers_are_taken_as_they_are():
    import torch
    dim = 12
    codes, xf, rows, w, grad_out, cnt = _weighted_request(dim, 1, False)
    x = torch.from_numpy(codes.view(np.int16)).view(torch.bfloat16)
    emb = glx.aggregate_weighted(wref.SUM, x, rows, w, W_S)
    assert wref.same_bits(emb, wref.forward(wref.SUM, xf, rows, w, None, W_S))
    out = torch.full((W_ROWS, dim), float("nan"), dtype=torch.bfloat16)
    glx.aggregate_backward(ref.SUM, rows, None, grad_out, W_ROWS, out=out)
    assert np.array_equal(_codes(out), b16.to_bf16(ref.backward(ref.SUM, rows, None, grad_out, W_ROWS)))
