"""CPU tests of the pair scores (glx_pair_dot and glx_pair_dot_backward): argument errors are found before any device
use, a well-formed call without a device fails loudly, and the numpy restatement of the contracts (pair_dot_ref.py) is
the gathered dot product and its gradients."""
import ctypes

import numpy as np
import pytest

import glx
import pair_dot_ref as pref

INVALID, UNAVAILABLE = 3, 14
ENTRY_POINTS = ["forward", "backward"]


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(entry, side=0, num_pairs=6, repeat=3, num_rows_a=3, num_rows_b=4, dim=4, heads=2, ptr_kind=glx.PTR_HOST,
          **null):
    """one well-formed call (2 sources x 3 candidates, tables of 3 and 4 rows, dim 4, 2 heads) with the named arguments
    replaced; xa=None etc. pass NULL for that buffer.  backward: side 0 (xa is the own table) unless side says else."""
    keep = {
        "xa": np.ones((3, 4), np.float32), "xb": np.ones((4, 4), np.float32), "ia": np.array([0, 2], np.int64),
        "ib": np.array([0, 1, 2, 3, 1, 0], np.int64), "out": np.zeros((6, 2), np.float32),
        "g": np.ones((6, 2), np.float32), "grad_self": np.zeros((4, 4), np.float32),
    }
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    if entry == "forward":
        rc = L.glx_pair_dot(0, ptr["xa"], num_rows_a, ptr["xb"], num_rows_b, dim, heads, ptr["ia"], ptr["ib"], num_pairs,
                            repeat, 0.0, ptr["out"], ptr_kind, None)
    else:
        own, other = (num_rows_a, num_rows_b) if side == 0 else (num_rows_b, num_rows_a)
        rc = L.glx_pair_dot_backward(0, side, ptr["ia"], ptr["ib"], num_pairs, repeat, ptr["g"], heads,
                                     ptr["xb" if side == 0 else "xa"], other, dim, own, 0.0, ptr["grad_self"], ptr_kind,
                                     None)
    return rc, L.glx_last_error().decode()


COMMON_ERRORS = [
    (dict(ia=None), "ia is NULL"),
    (dict(ib=None), "ib is NULL"),
    (dict(num_pairs=-3), "negative"),
    (dict(num_rows_a=-1), "negative"),
    (dict(num_rows_b=-1), "negative"),
    (dict(dim=0), "dim"),
    (dict(dim=-4), "dim"),
    (dict(heads=0), "heads"),
    (dict(heads=-2), "heads"),
    (dict(heads=3), "not a multiple of heads"),
    (dict(repeat=0), "repeat"),
    (dict(repeat=-3), "repeat"),
    (dict(repeat=4), "not a multiple of repeat"),
    (dict(ptr_kind=5), "ptr_kind"),
    (dict(num_rows_a=2 ** 31 - 1), "num_rows"),
    (dict(num_rows_b=2 ** 31 - 1), "num_rows"),
    (dict(num_pairs=2 ** 30 + 2, heads=2), "num_pairs * heads"),
]
OWN_ERRORS = {
    "forward": [(dict(xa=None), "xa is NULL"), (dict(xb=None), "xb is NULL"), (dict(out=None), "out is NULL")],
    "backward": [(dict(g=None), "g is NULL"), (dict(xb=None), "x_other is NULL"),
                 (dict(side=1, xa=None), "x_other is NULL"), (dict(grad_self=None), "grad_self is NULL"),
                 (dict(side=2), "side"), (dict(side=-1), "side")],
}


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_argument_errors_name_the_fault(entry):
    for kwargs, word in COMMON_ERRORS + OWN_ERRORS[entry]:
        rc, msg = _call(entry, **kwargs)
        assert rc == INVALID, (entry, kwargs, rc, msg)
        assert msg and word in msg, (entry, kwargs, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_well_formed_call_fails_loudly_without_a_device(entry):
    for kwargs in ({}, {"side": 1}, {"repeat": 1, "num_pairs": 2}, {"num_pairs": 0}):
        rc, msg = _call(entry, **kwargs)
        assert rc == UNAVAILABLE, (kwargs, rc, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_python_wrappers_raise_without_a_device():
    x = np.ones((3, 4), np.float32)
    ia, ib, g = np.array([0, 1], np.int64), np.array([[0, 1], [2, 0]], np.int64), np.ones((4, 2), np.float32)
    for call in (lambda: glx.pair_dot(x, ia, x, ib, heads=2, repeat=2),
                 lambda: glx.pair_dot_backward(0, ia, ib, g, x, 3, repeat=2),
                 lambda: glx.pair_dot_backward(1, ia, ib, g, x, 3, repeat=2)):
        with pytest.raises(glx.GlxError) as e:
            call()
        assert e.value.code == UNAVAILABLE


# ---- the restatement ------------------------------------------------------------------------------------------
def _composite(xa, ia, xb, ib, heads, repeat, default_attr):
    """(xa[ia].repeat_interleave(repeat, 0) * xb[ib]).view(n, H, C).sum(-1) in torch, with the rule for an index
    outside its table: a row of default_attr that passes no gradient on"""
    import torch

    def rows(x, idx):
        ok = (idx >= 0) & (idx < x.shape[0])
        picked = x[idx.clamp(0, x.shape[0] - 1)]
        return torch.where(ok[:, None], picked, torch.full_like(picked, default_attr))

    n = ib.numel()
    return (rows(xa, ia).repeat_interleave(repeat, 0) * rows(xb, ib)).view(n, heads, -1).sum(-1)


@pytest.mark.parametrize("repeat", [1, 3])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("out_of_range", [False, True])
def test_restatement_is_the_gradient_of_the_composite(out_of_range, heads, repeat):
    """backward in float64 against torch's CPU autograd of the composite: 1e-12 relative (a float64 sum of a dozen
    terms in another order differs by a few 1e-16 of the terms' magnitude)"""
    import torch
    rng = np.random.default_rng(5 + heads + 10 * repeat + 100 * out_of_range)
    na, nb, D, B, default_attr = 5, 7, 6, 8, 0.5
    lo, extra = (-1, 1) if out_of_range else (0, 0)
    ia = rng.integers(lo, na + extra, B).astype(np.int64)
    ib = rng.integers(lo, nb + extra, B * repeat).astype(np.int64)
    if out_of_range:
        ia[0], ia[1], ib[0], ib[-1], ib[repeat] = -1, na, 2, nb, -1  # alone on either side, and together (pair `repeat`)
    ia[2] = ia[3] = 1  # one source row behind two entries: their pairs interleave with nobody's, but both add to row 1
    xa, xb = rng.standard_normal((na, D)), rng.standard_normal((nb, D))
    g = rng.standard_normal((B * repeat, heads))
    ta, tb = torch.tensor(xa, requires_grad=True), torch.tensor(xb, requires_grad=True)
    out = _composite(ta, torch.tensor(ia), tb, torch.tensor(ib), heads, repeat, default_attr)
    out.backward(torch.tensor(g))
    want_out, _ = pref.forward(xa, ia, xb, ib, heads, repeat, default_attr)
    assert np.all(np.abs(out.detach().numpy() - want_out) <= 1e-12 * np.abs(want_out))
    ga = pref.backward(0, ia, ib, g, xb, na, repeat, default_attr, dtype=np.float64)
    gb = pref.backward(1, ia, ib, g, xa, nb, repeat, default_attr, dtype=np.float64)
    assert np.all(np.abs(ga - ta.grad.numpy()) <= 1e-12 * np.abs(ta.grad.numpy()))
    assert np.all(np.abs(gb - tb.grad.numpy()) <= 1e-12 * np.abs(tb.grad.numpy()))
    assert np.any(ga != 0) and np.any(gb != 0)


def test_restatement_rounds_the_product_before_the_add():
    """one element where a fused multiply-add differs from multiply-then-add"""
    a = np.float32(1 + 2.0 ** -12)
    xb = np.array([[a], [-1.0]], np.float32)
    g = np.array([a, a * a], np.float32)  # a * a rounds; g0 xb0 + g1 xb1 is exactly 0 only if the product rounds
    grad = pref.backward(0, np.array([0, 0], np.int64), np.array([0, 1], np.int64), g, xb, 1)
    assert grad[0, 0] == 0.0
    assert np.float64(a) * np.float64(a) - np.float64(g[1]) != 0.0  # fused, it would not be


def test_restatement_out_of_range_rule_and_bound():
    xa = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    xb = np.array([[1.0, 1.0, 10.0, 10.0], [2.0, 2.0, 2.0, 2.0]], np.float32)
    ia, ib = np.array([0, 7], np.int64), np.array([0, 1, -1, 1], np.int64)  # 2 sources x 2 candidates
    out, bound = pref.forward(xa, ia, xb, ib, heads=2, repeat=2, default_attr=0.5)
    assert out.tolist() == [[3.0, 70.0], [6.0, 14.0], [0.5, 0.5], [2.0, 2.0]]
    assert bound[0, 0] == 2 * 2.0 ** -23 * 3.0 + 2.0 ** -126
    g = np.ones((4, 2), np.float32)
    ga = pref.backward(0, ia, ib, g, xb, 1, repeat=2, default_attr=0.5)
    assert ga.tolist() == [[3.0, 3.0, 12.0, 12.0]]  # pairs 0 and 1; source 7 is outside xa: nothing
    gb = pref.backward(1, ia, ib, g, xa, 2, repeat=2, default_attr=0.5)
    assert gb.tolist() == [[1.0, 2.0, 3.0, 4.0], [1.5, 2.5, 3.5, 4.5]]  # row 1: pair 1's xa[0] plus pair 3's default row


def test_a_float32_dot_in_any_column_order_stays_inside_the_bound():
    """200 dot products of mixed magnitudes, summed in float32 left to right, right to left and as a pairwise tree over
    strided partial sums (what a lane group does): each within C * 2^-23 * sum|a b| + 2^-126 of the exact value"""
    rng = np.random.default_rng(23)
    f32 = np.float32
    for case in range(200):
        C = int(rng.integers(1, 300))
        scale = 10.0 ** rng.integers(-6, 7, C)
        a = (rng.standard_normal(C) * scale).astype(f32)
        b = (rng.standard_normal(C) * 10.0 ** rng.integers(-3, 4, C)).astype(f32)
        want, bound = pref.forward(a[None], [0], b[None], [0])
        prod = a * b  # float32, rounded
        orders = []
        acc = f32(0)
        for t in prod:
            acc = f32(acc + t)
        orders.append(acc)
        acc = f32(0)
        for t in prod[::-1]:
            acc = f32(acc + t)
        orders.append(acc)
        lanes = np.zeros(64, f32)
        for i, t in enumerate(prod):  # lane i % 64 owns term i
            lanes[i % 64] = f32(lanes[i % 64] + t)
        width = 64
        while width > 1:  # the xor tree
            width //= 2
            lanes[:width] = lanes[:width] + lanes[width:2 * width]
        orders.append(lanes[0])
        for got in orders:
            assert abs(np.float64(got) - want[0, 0]) <= bound[0, 0], (case, C, got, want[0, 0], bound[0, 0])
