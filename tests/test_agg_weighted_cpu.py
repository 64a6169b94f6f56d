"""CPU tests of the weighted aggregation (glx_aggregate_weighted and its two gradients): argument errors are found
before any device use, a well-formed call without a device fails loudly, and the numpy restatement of the contracts
(agg_weighted_ref.py) is a weighted gather + reduce and its gradients."""
import ctypes

import numpy as np
import pytest

import agg_backward_ref as ref
import agg_weighted_ref as wref
import glx

INVALID, UNAVAILABLE = 3, 14
ENTRY_POINTS = ["forward", "backward_x", "backward_w"]


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(entry, op=glx.SUM, num_ids=4, num_segments=2, num_rows=3, dim=4, heads=2, ptr_kind=glx.PTR_HOST, **null):
    """one well-formed call (4 positions, 2 segments, 3 rows, dim 4, 2 heads) with the named arguments replaced;
    x=None etc. pass NULL for that buffer"""
    keep = {
        "x": np.ones((3, 4), np.float32), "rows": np.array([0, 1, 2, 1], np.int64), "w": np.ones((4, 2), np.float32),
        "cnt": np.array([2, 2], np.int32), "emb": np.zeros((2, 4), np.float32), "grad_out": np.ones((2, 4), np.float32),
        "grad_x": np.zeros((3, 4), np.float32), "grad_w": np.zeros((4, 2), np.float32),
    }
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    if entry == "forward":
        rc = L.glx_aggregate_weighted(0, op, ptr["x"], num_rows, dim, ptr["rows"], ptr["w"], heads, ptr["cnt"], num_ids,
                                      num_segments, 0.0, ptr["emb"], ptr_kind, None)
    elif entry == "backward_x":
        rc = L.glx_aggregate_weighted_backward_x(0, op, ptr["rows"], ptr["w"], heads, ptr["cnt"], num_ids, num_segments,
                                                 num_rows, dim, ptr["grad_out"], ptr["grad_x"], ptr_kind, None)
    else:
        rc = L.glx_aggregate_weighted_backward_w(0, op, ptr["x"], num_rows, dim, ptr["rows"], heads, ptr["cnt"], num_ids,
                                                 num_segments, 0.0, ptr["grad_out"], ptr["grad_w"], ptr_kind, None)
    return rc, L.glx_last_error().decode()


COMMON_ERRORS = [
    (dict(rows=None), "rows is NULL"),
    (dict(num_ids=-1), "negative"),
    (dict(num_segments=-1), "negative"),
    (dict(num_rows=-1), "negative"),
    (dict(dim=0), "dim"),
    (dict(dim=-4), "dim"),
    (dict(heads=0), "heads"),
    (dict(heads=-2), "heads"),
    (dict(heads=3), "not a multiple of heads"),
    (dict(op=glx.MAX), "Max"),
    (dict(op=glx.MIN), "Min"),
    (dict(op=glx.PROD), "Prod"),
    (dict(op=7), "unknown aggregator"),
    (dict(ptr_kind=5), "ptr_kind"),
]
OWN_ERRORS = {
    "forward": [(dict(x=None), "x is NULL"), (dict(w=None), "w is NULL"), (dict(emb=None), "emb_out is NULL")],
    "backward_x": [(dict(w=None), "w is NULL"), (dict(grad_out=None), "grad_out is NULL"),
                   (dict(grad_x=None), "grad_x is NULL")],
    "backward_w": [(dict(x=None), "x is NULL"), (dict(grad_out=None), "grad_out is NULL"),
                   (dict(grad_w=None), "grad_w is NULL")],
}


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_argument_errors_name_the_fault(entry):
    for kwargs, word in COMMON_ERRORS + OWN_ERRORS[entry]:
        rc, msg = _call(entry, **kwargs)
        assert rc == INVALID, (entry, kwargs, rc, msg)
        assert word in msg, (entry, kwargs, msg)


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_int32_limits(entry):
    # checked before any buffer is touched: the sizes alone decide
    rc, msg = _call(entry, num_ids=2 ** 30, heads=4, dim=4)
    assert rc == INVALID and "num_ids * heads" in msg, (rc, msg)
    rc, msg = _call(entry, num_segments=2 ** 30, dim=4)
    assert rc == INVALID and "num_segments * dim" in msg, (rc, msg)
    rc, msg = _call(entry, num_rows=2 ** 31 - 1)
    assert rc == INVALID and "num_rows" in msg, (rc, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_well_formed_call_fails_loudly_without_a_device(entry):
    for op in (glx.SUM, glx.MEAN):
        for null in ({}, {"cnt": None}):
            rc, msg = _call(entry, op=op, **null)
            assert rc == UNAVAILABLE, (rc, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_python_wrappers_raise_without_a_device():
    x, rows = np.ones((3, 4), np.float32), np.array([0, 1], np.int64)
    w, g = np.ones((2, 2), np.float32), np.ones((2, 4), np.float32)
    for call in (lambda: glx.aggregate_weighted("SumAggregator", x, rows, w, 2),
                 lambda: glx.aggregate_weighted_backward_x(glx.SUM, rows, w, None, g, 3),
                 lambda: glx.aggregate_weighted_backward_w(glx.MEAN, x, rows, 2, None, g)):
        with pytest.raises(glx.GlxError) as e:
            call()
        assert e.value.code == UNAVAILABLE


# ---- the restatement ------------------------------------------------------------------------------------------
def _request(rng, ragged):
    """(rows, cnt, S, num_rows): 36 positions over 7 rows, -1 and num_rows among them; ragged: counts with empty
    segments whose sum leaves a tail that is not consumed"""
    n, num_rows = 36, 7
    rows = rng.integers(-1, num_rows + 1, n).astype(np.int64)
    rows[:8] = rng.integers(0, 2, 8)  # two long lists
    if not ragged:
        return rows, None, 6, num_rows
    cnt = np.array([5, 0, 1, 12, 0, 8, 4, 0], np.int32)  # 30 of 36 consumed
    return rows, cnt, len(cnt), num_rows


@pytest.mark.parametrize("op", [wref.SUM, wref.MEAN])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("ragged", [False, True])
def test_restatement_gradients_agree_with_central_differences(ragged, heads, op):
    """f(x, w) = sum(forward(x, w) * G) in float64 is linear in x and in w, so a central difference with a power-of-two
    step is its derivative up to rounding: relative 1e-6"""
    rng = np.random.default_rng(3 + op + 10 * heads + 100 * ragged)
    rows, cnt, S, num_rows = _request(rng, ragged)
    n, D, default_attr, h = len(rows), 4, 0.5, 0.25
    X = rng.standard_normal((num_rows, D))
    W = rng.standard_normal((n, heads))
    G = rng.standard_normal((S, D))
    f = lambda x, w: float((wref.forward(op, x, rows, w, cnt, S, default_attr, dtype=np.float64) * G).sum())  # noqa: E731
    gx = wref.backward_x(op, rows, W, cnt, G, num_rows, dtype=np.float64)
    gw, _ = wref.backward_w(op, X, rows, heads, cnt, G, default_attr)
    fd_x = np.zeros_like(X)
    for i in np.ndindex(*X.shape):
        d = np.zeros_like(X)
        d[i] = h
        fd_x[i] = (f(X + d, W) - f(X - d, W)) / (2 * h)
    fd_w = np.zeros_like(W)
    for i in np.ndindex(*W.shape):
        d = np.zeros_like(W)
        d[i] = h
        fd_w[i] = (f(X, W + d) - f(X, W - d)) / (2 * h)
    assert np.all(np.abs(gx - fd_x) <= 1e-6 * np.abs(fd_x))
    assert np.all(np.abs(gw - fd_w) <= 1e-6 * np.abs(fd_w))
    assert np.any(gx != 0) and np.any(gw != 0)
    if ragged:
        assert not gw[30:].any() and not fd_w[30:].any()  # the tail was not consumed


@pytest.mark.parametrize("op", [wref.SUM, wref.MEAN])
@pytest.mark.parametrize("ragged", [False, True])
def test_all_ones_weights_are_the_unweighted_fold_bit_for_bit(ragged, op):
    rng = np.random.default_rng(17 + ragged)
    rows, cnt, S, num_rows = _request(rng, ragged)
    X = rng.standard_normal((num_rows, 5)).astype(np.float32)
    X[1, 0], X[1, 1], X[0, 2], X[0, 3] = np.nan, np.inf, -0.0, -np.inf
    X[:, 4] = -0.0  # a column whose sums stay at signed zeros
    got = wref.forward(op, X, rows, np.ones(len(rows), np.float32), cnt, S, default_attr=-0.0)
    want = ref.fold(op, X, rows, wref.starts(cnt, len(rows), S), default_attr=-0.0)
    assert ref.same_bits(got, want)


def test_restatement_rounds_the_product_before_the_add():
    """one term where a fused multiply-add differs from multiply-then-add"""
    a = np.float32(1 + 2.0 ** -12)
    X = np.array([[a], [-1.0]], np.float32)
    w = np.array([a, a * a], np.float32)  # a * a rounds; the sum (w0 x0 + w1 x1) is exactly 0 only if the product rounds
    emb = wref.forward(wref.SUM, X, np.array([0, 1], np.int64), w, None, 1)
    assert emb[0, 0] == 0.0
    assert np.float64(a) * np.float64(a) - np.float64(w[1]) != 0.0  # fused, it would not be


def test_restatement_bound_and_tail():
    X = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    rows = np.array([0, 5, 0], np.int64)
    g = np.array([[1.0, 1.0, 10.0, 10.0]], np.float32)
    gw, bound = wref.backward_w(wref.MEAN, X, rows, 2, np.array([2], np.int32), g, default_attr=0.5)
    assert gw.tolist() == [[1.5, 35.0], [0.5, 5.0], [0.0, 0.0]]
    assert bound[0, 0] == 2 * 2.0 ** -23 * 1.5 + 2.0 ** -126 and not bound[2].any()
