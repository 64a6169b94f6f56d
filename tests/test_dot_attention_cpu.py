"""CPU tests of the fused dot-product attention (glx_dot_attention and glx_dot_attention_backward): the library carries
the entry points and finds argument errors before any device use, and the numpy restatement of the contract
(dot_attention_ref.py) has the gradients of its own float64 forward."""
import ctypes

import numpy as np
import pytest

import dot_attention_ref as dref
import glx

INVALID = 3


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_the_library_exports_both_entry_points():
    assert "glx_dot_attention" in glx.EXPORTS and "glx_dot_attention_backward" in glx.EXPORTS
    L = ctypes.CDLL(glx.LIB_PATH)
    assert hasattr(L, "glx_dot_attention") and hasattr(L, "glx_dot_attention_backward")
    assert L.glx_abi_version() == 5


def _call(entry, num_ids=4, num_segments=2, dim=4, heads=2, num_rows=3, scale=0.5, drop_p=0.0, ptr_kind=glx.PTR_HOST,
          **null):
    """one well-formed call (4 positions, 2 segments, 4 columns in 2 heads, 3 rows) with the named arguments replaced;
    q=None etc. pass NULL for that buffer"""
    keep = {
        "q": np.ones((2, 4), np.float32), "k": np.ones((3, 4), np.float32), "v": np.ones((3, 4), np.float32),
        "rows": np.zeros(4, np.int64), "edge": np.ones((4, 4), np.float32), "cnt": np.array([2, 2], np.int32),
        "logit_out": np.zeros((4, 2), np.float32), "soft_out": np.zeros((4, 2), np.float32),
        "out": np.zeros((2, 4), np.float32), "soft": np.full((4, 2), 0.5, np.float32),
        "grad_out": np.ones((2, 4), np.float32), "grad_e": np.zeros((4, 2), np.float32),
        "grad_q": np.zeros((2, 4), np.float32), "grad_k": np.zeros((3, 4), np.float32),
        "grad_v": np.zeros((3, 4), np.float32), "grad_edge": np.zeros((4, 4), np.float32),
    }
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    if entry == "forward":
        rc = L.glx_dot_attention(0, ptr["q"], ptr["k"], ptr["v"], num_rows, dim, heads, ptr["rows"], ptr["edge"],
                                 ptr["cnt"], num_ids, num_segments, scale, 0.0, drop_p, 1, 2, ptr["logit_out"],
                                 ptr["soft_out"], ptr["out"], ptr_kind, None)
    else:
        rc = L.glx_dot_attention_backward(0, ptr["q"], ptr["k"], ptr["v"], num_rows, dim, heads, ptr["rows"],
                                          ptr["edge"], ptr["cnt"], num_ids, num_segments, scale, 0.0, drop_p, 1, 2,
                                          ptr["soft"], ptr["grad_out"], ptr["grad_e"], ptr["grad_q"], ptr["grad_k"],
                                          ptr["grad_v"], ptr["grad_edge"], ptr_kind, None)
    return rc, L.glx_last_error().decode()


COMMON_ERRORS = [
    (dict(heads=3), "multiple of heads"),
    (dict(dim=6, heads=4), "multiple of heads"),
    (dict(heads=0), "heads"),
    (dict(heads=-2), "heads"),
    (dict(dim=0), "dim"),
    (dict(dim=-4), "dim"),
    (dict(num_ids=-1), "negative"),
    (dict(num_segments=-1), "negative"),
    (dict(num_rows=-1), "negative"),
    (dict(drop_p=-0.1), "drop_p"),
    (dict(drop_p=1.0), "drop_p"),
    (dict(drop_p=float("nan")), "drop_p"),
    (dict(scale=float("inf")), "scale"),
    (dict(scale=float("-inf")), "scale"),
    (dict(scale=float("nan")), "scale"),
    (dict(num_ids=2 ** 30, heads=4), "num_ids * heads"),
    (dict(num_segments=2 ** 30), "num_segments * dim"),
    (dict(num_rows=2 ** 31), "num_rows"),
    (dict(ptr_kind=5), "ptr_kind"),
    (dict(cnt=None, num_ids=3), "multiple"),
    (dict(rows=None), "rows is NULL"),
    (dict(q=None), "q is NULL"),
    (dict(k=None), "k or v is NULL"),
    (dict(v=None), "k or v is NULL"),
]
OWN_ERRORS = {
    "forward": [(dict(soft_out=None), "soft_out is NULL"), (dict(out=None), "out is NULL")],
    "backward": [(dict(soft=None), "soft is NULL"), (dict(grad_out=None), "grad_out is NULL"),
                 (dict(grad_e=None), "grad_e_out is NULL"), (dict(edge=None), "grad_edge_out needs edge")],
}


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_argument_errors_need_no_gpu(entry):
    for kwargs, word in COMMON_ERRORS + OWN_ERRORS[entry]:
        rc, msg = _call(entry, **kwargs)
        assert rc == INVALID and word in msg, (entry, kwargs, rc, msg)


def _request(heads, with_edge, seed):
    """5 segments (one empty), a tail nobody consumes, rows outside the table"""
    rng = np.random.default_rng(seed)
    cnt = np.array([3, 0, 1, 6, 4], np.int32)
    S, n, M, D = len(cnt), int(cnt.sum()) + 2, 7, 6
    q = rng.standard_normal((S, D))
    k = rng.standard_normal((M, D))
    v = rng.standard_normal((M, D))
    rows = rng.integers(0, M, n).astype(np.int64)
    rows[4], rows[9] = -1, M
    edge = rng.standard_normal((n, D)) if with_edge else None
    g = rng.standard_normal((S, D))
    return q, k, v, rows, edge, cnt, S, g


@pytest.mark.parametrize("drop_p", [0.0, 0.25])
@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("heads", [1, 3])
def test_analytic_gradients_are_the_central_differences_of_the_float64_forward(heads, with_edge, drop_p):
    """every element of q, k, v and edge: (f(x + h) - f(x - h)) / 2h of f = sum(out * g) at h = 1e-6 against the
    contract's formulas; the truncation error is O(h^2) and the cancellation error about 1e-16 / h = 1e-10 of the
    magnitudes, so 1e-7 absolute on values of order 1 has three decimal digits of room"""
    q, k, v, rows, edge, cnt, S, g = _request(heads, with_edge, heads)
    scale, da = 0.7, 0.5
    n = len(rows)
    ks = None
    if drop_p:
        keep = dref.keep_mask(n, heads, drop_p, 7, 2 ** 33 + 1)
        ks = np.where(keep, float(dref.gref.scale(drop_p)), 0.0)
        assert 0 < keep.sum() < keep.size

    def f(q_, k_, v_, e_):
        return float((dref.forward64(q_, k_, v_, rows, e_, cnt, S, heads, scale, da, ks)[0] * g).sum())

    got = dref.backward64(q, k, v, rows, edge, cnt, S, heads, scale, g, da, ks)
    args = [q, k, v, edge]
    h = 1e-6
    for which, grad in enumerate(got):
        if args[which] is None:
            assert grad is None
            continue
        num = np.zeros_like(args[which])
        for idx in np.ndindex(*args[which].shape):
            hi = [a if a is None else a.copy() for a in args]
            lo = [a if a is None else a.copy() for a in args]
            hi[which][idx] += h
            lo[which][idx] -= h
            num[idx] = (f(*hi) - f(*lo)) / (2 * h)
        assert np.abs(num - grad).max() <= 1e-7, (which, np.abs(num - grad).max())
        assert np.any(grad != 0)
    # the empty segment's query, the rows nobody names and the tail's edge rows get nothing
    assert not got[0][1].any()
    named = np.zeros(len(k), bool)
    named[rows[:int(cnt.sum())][(rows[:int(cnt.sum())] >= 0) & (rows[:int(cnt.sum())] < len(k))]] = True
    assert not got[1][~named].any() and not got[2][~named].any()
    if with_edge:
        assert not got[3][int(cnt.sum()):].any()


def test_float32_stages_agree_with_the_float64_forward():
    """the stage-by-stage float32 restatement is the float64 function inside its own bounds"""
    heads = 2
    q, k, v, rows, edge, cnt, S, g = _request(heads, True, 11)
    q, k, v, edge, g = (a.astype(np.float32) for a in (q, k, v, edge, g))
    scale = dref.default_scale(q.shape[1], heads)
    assert scale == np.float32(1.0) / np.sqrt(np.float32(3.0))
    kk, vv = dref.gathered(k, rows, edge, 0.5), dref.gathered(v, rows, edge, 0.5)
    assert kk.dtype == np.float32 and dref.same_bits(kk[4], (np.float32(0.5) + edge[4]).astype(np.float32))
    e, eb = dref.logits(q, kk, cnt, S, heads, scale)
    soft, sb = dref.softmax(e.astype(np.float32), cnt, S)
    want_out, want_soft, _ = dref.forward64(q, k, v, rows, edge, cnt, S, heads, float(scale), 0.5)
    assert np.all(np.abs(soft - want_soft) <= sb + 1e-6 * want_soft)  # float32 logits against float64 ones
    assert soft[3, 0] == 1.0 and not soft[int(cnt.sum()):].any()  # k == 1; the tail
    got = dref.out(soft.astype(np.float32), vv, cnt, S)
    assert got.dtype == np.float32 and np.allclose(got, want_out, rtol=1e-5, atol=1e-6)
    assert dref.same_bits(got[1], np.zeros(q.shape[1], np.float32))  # the empty segment: +0.0, not default_attr
    ge, gb = dref.grad_e(soft.astype(np.float32), g, vv, cnt, S, heads, scale)
    want = dref.backward64(q, k, v, rows, edge, cnt, S, heads, float(scale), g, 0.5)
    ge32 = ge.astype(np.float32)
    assert np.allclose(dref.grad_q(ge32, kk, cnt, S), want[0], rtol=1e-4, atol=1e-5)
    assert np.allclose(dref.grad_rows(ge32, rows, cnt, q, len(k)), want[1], rtol=1e-4, atol=1e-5)
    assert np.allclose(dref.grad_rows(soft.astype(np.float32), rows, cnt, g, len(v)), want[2], rtol=1e-4, atol=1e-5)
    assert np.allclose(dref.grad_edge(ge32, soft.astype(np.float32), q, g, cnt, S), want[3], rtol=1e-4, atol=1e-5)
    assert np.all(gb[:int(cnt.sum())] > 0) and not gb[int(cnt.sum()):].any()
