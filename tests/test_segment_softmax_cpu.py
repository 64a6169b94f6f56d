"""CPU tests of the ragged segment softmax (glx_segment_softmax and glx_segment_softmax_backward): argument errors are
found before any device use, a well-formed call without a device fails loudly, and the numpy restatement of the
contracts (segment_softmax_ref.py) is a softmax with its gradient and obeys the exact rules."""
import ctypes

import numpy as np
import pytest

import glx
import segment_softmax_ref as sref

INVALID, UNAVAILABLE = 3, 14
ENTRY_POINTS = ["forward", "backward"]


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(entry, num_ids=4, num_segments=2, heads=2, ptr_kind=glx.PTR_HOST, **null):
    """one well-formed call (4 positions, 2 segments, 2 heads) with the named arguments replaced; e=None etc. pass
    NULL for that buffer"""
    keep = {
        "e": np.ones((4, 2), np.float32), "alpha": np.full((4, 2), 0.5, np.float32),
        "grad_alpha": np.ones((4, 2), np.float32), "cnt": np.array([2, 2], np.int32),
        "alpha_out": np.zeros((4, 2), np.float32), "grad_e": np.zeros((4, 2), np.float32),
    }
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    if entry == "forward":
        rc = L.glx_segment_softmax(0, ptr["e"], heads, ptr["cnt"], num_ids, num_segments, ptr["alpha_out"], ptr_kind,
                                   None)
    else:
        rc = L.glx_segment_softmax_backward(0, ptr["alpha"], ptr["grad_alpha"], heads, ptr["cnt"], num_ids,
                                            num_segments, ptr["grad_e"], ptr_kind, None)
    return rc, L.glx_last_error().decode()


COMMON_ERRORS = [
    (dict(num_ids=-1), "negative"),
    (dict(num_segments=-1), "negative"),
    (dict(heads=0), "heads"),
    (dict(heads=-2), "heads"),
    (dict(ptr_kind=5), "ptr_kind"),
]
OWN_ERRORS = {
    "forward": [(dict(e=None), "e is NULL"), (dict(alpha_out=None), "alpha_out is NULL")],
    "backward": [(dict(alpha=None), "alpha is NULL"), (dict(grad_alpha=None), "grad_alpha is NULL"),
                 (dict(grad_e=None), "grad_e is NULL")],
}


def test_the_library_exports_both_entry_points():
    assert "glx_segment_softmax" in glx.EXPORTS and "glx_segment_softmax_backward" in glx.EXPORTS
    L = glx.lib()
    assert L.glx_abi_version() == 5
    assert L.glx_segment_softmax.argtypes is not None and L.glx_segment_softmax_backward.argtypes is not None


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_argument_errors_name_the_fault(entry):
    for kwargs, word in COMMON_ERRORS + OWN_ERRORS[entry]:
        rc, msg = _call(entry, **kwargs)
        assert rc == INVALID, (entry, kwargs, rc, msg)
        assert word in msg, (entry, kwargs, msg)


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_int32_limit(entry):
    # checked before any buffer is touched: the sizes alone decide
    rc, msg = _call(entry, num_ids=2 ** 30, heads=4)
    assert rc == INVALID and "num_ids * heads" in msg, (rc, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_well_formed_call_fails_loudly_without_a_device(entry):
    for null in ({}, {"cnt": None}):
        rc, msg = _call(entry, **null)
        assert rc == UNAVAILABLE, (rc, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_python_wrappers_raise_without_a_device():
    e, g = np.ones((4, 2), np.float32), np.ones((4, 2), np.float32)
    cnt = np.array([1, 3], np.int32)
    for call in (lambda: glx.segment_softmax(e, 2), lambda: glx.segment_softmax(e[:, 0].copy(), 2, cnt=cnt),
                 lambda: glx.segment_softmax_backward(e, g, None, 2),
                 lambda: glx.segment_softmax_backward(e, g, cnt, 2)):
        with pytest.raises(glx.GlxError) as err:
            call()
        assert err.value.code == UNAVAILABLE


# ---- the restatement ------------------------------------------------------------------------------------------
RAGGED = np.array([5, 0, 1, 12, -3, 8, 4, 0], np.int32)  # 30 of 36 consumed, a negative count is an empty segment


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("ragged", [False, True])
def test_restatement_backward_agrees_with_central_differences(ragged, heads):
    """f(e) = sum(forward(e) * G) in float64; a central difference with step 2^-10 is its derivative up to h^2 f''' / 6:
    relative 1e-5 of the scale of the terms"""
    rng = np.random.default_rng(5 + heads + 10 * ragged)
    n, cnt, S = 36, (RAGGED if ragged else None), (len(RAGGED) if ragged else 6)
    e = rng.standard_normal((n, heads)).astype(np.float32)  # float32 values: forward() reads float32
    G = rng.standard_normal((n, heads)).astype(np.float32)
    h = 2.0 ** -10  # e +- h is exact in float32 for |e| < 8
    alpha, _ = sref.forward(e, cnt, S)
    # the gradient from the float64 alpha itself, not from its float32 rounding
    start = sref.starts(cnt, n, S)
    grad = np.zeros((n, heads))
    for s in range(S):
        a, b = int(start[s]), int(start[s + 1])
        grad[a:b] = alpha[a:b] * (G[a:b] - (alpha[a:b] * G[a:b]).sum(0))
    # ... which the restatement's backward reproduces from the float32 rounding of alpha, inside its own bound
    got, bound = sref.backward(alpha.astype(np.float32), G, cnt, S)
    assert np.all(np.abs(got - grad) <= 2.0 ** -22 * (np.abs(G) + 1)) and np.all(bound >= 0)
    fd = np.zeros_like(grad)
    for i in np.ndindex(n, heads):
        d = np.zeros((n, heads), np.float32)
        d[i] = h
        fd[i] = ((sref.forward(e + d, cnt, S)[0] * G).sum() - (sref.forward(e - d, cnt, S)[0] * G).sum()) / (2 * h)
    assert np.all(np.abs(got - fd) <= 1e-5 * np.abs(G).max()), np.abs(got - fd).max()
    assert np.any(got != 0)
    if ragged:
        assert not got[30:].any() and not fd[30:].any() and not alpha[30:].any()  # the tail was not consumed
    for s in range(S):  # every non-empty (segment, head) sums to one
        if start[s + 1] > start[s]:
            assert np.all(np.abs(alpha[int(start[s]):int(start[s + 1])].sum(0) - 1.0) < 1e-14)


def test_restatement_exact_rules():
    inf, nan = np.inf, np.nan
    #            k = 1 | equal logits, k = 3 | a mask       | NaN  | +inf     | all -inf   | not consumed
    e = np.array([7.5, 2.0, 2.0, 2.0, 0.0, -inf, 1.0, nan, 0.0, inf, 0.0, -inf, -inf, 3.0], np.float32)
    cnt = np.array([1, 3, 3, 0, 2, 2, 2], np.int32)
    alpha, bound = sref.forward(e, cnt, len(cnt))
    assert alpha[0] == 1.0 and np.all(alpha[1:4] == 1.0 / 3.0)
    assert alpha[5] == 0.0 and bound[5] == 0.0 and not np.signbit(alpha[5])
    assert abs(alpha[4] + alpha[6] - 1.0) < 1e-15 and alpha[6] > alpha[4]
    assert np.isnan(alpha[7:13]).all()
    assert alpha[13] == 0.0 and bound[13] == 0.0
    assert np.all(bound[:5] > 0) and np.all(bound[:5] < 1e-5)
    # heads are independent: a NaN in head 0 leaves head 1 alone
    e2 = np.array([[nan, 1.0], [0.0, 1.0]], np.float32)
    a2, _ = sref.forward(e2, None, 1)
    assert np.isnan(a2[:, 0]).all() and np.all(a2[:, 1] == 0.5)
    # a shift that is exact in float32 changes nothing
    base = (np.arange(6) / 1024.0).astype(np.float32)
    assert np.array_equal(sref.forward(base, None, 2)[0], sref.forward(base + np.float32(8.0), None, 2)[0])
    # counts that promise more than the request has are cut; the implied layout leaves its remainder
    a3, _ = sref.forward(np.zeros(5, np.float32), np.array([2, 9], np.int32), 2)
    assert a3.tolist() == [0.5, 0.5, 1 / 3, 1 / 3, 1 / 3]
    a4, b4 = sref.forward(np.zeros(5, np.float32), None, 2)
    assert a4.tolist() == [0.5, 0.5, 0.5, 0.5, 0.0] and b4[4] == 0.0


def test_restatement_backward_bound_and_tail():
    alpha = np.array([0.25, 0.75, 1.0, 0.5], np.float32)
    g = np.array([4.0, 8.0, 3.0, 9.0], np.float32)
    got, bound = sref.backward(alpha, g, np.array([2, 1], np.int32), 2)
    assert got.tolist() == [0.25 * (4 - 7), 0.75 * (8 - 7), 0.0, 0.0]
    assert bound[0] == 0.25 * 4 * 2.0 ** -23 * (4 + 7) + 2.0 ** -126 and bound[3] == 0.0
    # a gradient that is constant over a segment passes nothing on
    a, _ = sref.forward(np.arange(5, dtype=np.float32), None, 1)
    got, _ = sref.backward(a, np.full(5, 3.0, np.float32), None, 1)
    assert np.all(np.abs(got) < 1e-7)
