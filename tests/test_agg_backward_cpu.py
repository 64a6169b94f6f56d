"""CPU tests of the differentiable aggregation (glx_aggregate_arg / glx_aggregate_backward): argument errors are
found before any device use, a well-formed call without a device fails loudly, and the numpy restatement of the
contract (agg_backward_ref.py) is the gradient of a gather + reduce."""
import ctypes

import numpy as np
import pytest

import agg_backward_ref as ref
import glx

INVALID, UNAVAILABLE = 3, 14


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(op=glx.SUM, rows="ok", cnt="ok", arg=None, num_ids=4, num_segments=2, num_rows=3, dim=2, grad_out="ok",
          grad_x="ok", ptr_kind=glx.PTR_HOST):
    keep = {
        "rows": np.array([0, 1, 2, 1], np.int64), "cnt": np.array([2, 2], np.int32),
        "grad_out": np.ones((2, 2), np.float32), "grad_x": np.zeros((3, 2), np.float32),
    }
    pick = lambda name, v: _p(keep[name]) if isinstance(v, str) else (None if v is None else _p(v))  # noqa: E731
    rc = glx.lib().glx_aggregate_backward(0, op, pick("rows", rows), pick("cnt", cnt), None if arg is None else _p(arg),
                                          num_ids, num_segments, num_rows, dim, pick("grad_out", grad_out),
                                          pick("grad_x", grad_x), ptr_kind, None)
    return rc, glx.lib().glx_last_error().decode()


@pytest.mark.parametrize("kwargs, word", [
    (dict(rows=None), "rows is NULL"),
    (dict(grad_out=None), "grad_out is NULL"),
    (dict(grad_x=None), "grad_x is NULL"),
    (dict(num_ids=-1), "negative"),
    (dict(num_segments=-1), "negative"),
    (dict(num_rows=-1), "negative"),
    (dict(dim=0), "dim"),
    (dict(dim=-4), "dim"),
    (dict(op=glx.PROD), "Prod"),
    (dict(op=7), "unknown aggregator"),
    (dict(op=glx.MAX), "arg is NULL"),
    (dict(op=glx.MIN), "arg is NULL"),
    (dict(ptr_kind=5), "ptr_kind"),
])
def test_backward_argument_errors_name_the_fault(kwargs, word):
    rc, msg = _call(**kwargs)
    assert rc == INVALID, (rc, msg)
    assert word in msg, msg


def test_max_names_the_op_that_needs_arg():
    assert "Max" in _call(op=glx.MAX)[1] and "Min" in _call(op=glx.MIN)[1]


def test_aggregate_arg_argument_errors():
    L = glx.lib()
    emb, cnt, arg = np.zeros(4, np.float32), np.zeros(2, np.int32), np.zeros(4, np.int32)
    ids = np.zeros(4, np.int64)
    assert L.glx_aggregate_arg(None, glx.MAX, _p(ids), None, 4, 2, 0.0, _p(emb), _p(cnt), _p(arg), 0, None) == INVALID
    assert b"features is NULL" in L.glx_last_error()


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_well_formed_backward_fails_loudly_without_a_device():
    for op, arg in ((glx.SUM, None), (glx.MEAN, None), (glx.MAX, np.zeros((2, 2), np.int32))):
        rc, msg = _call(op=op, arg=arg)
        assert rc == UNAVAILABLE, (rc, msg)
    with pytest.raises(glx.GlxError) as e:
        glx.aggregate_backward("SumAggregator", np.array([0, 1], np.int64), None, np.ones((2, 4), np.float32), 3)
    assert e.value.code == UNAVAILABLE


# ---- the restatement is the gradient of gather + reduce ------------------------------------------------------
def _request(rng, n, num_rows, ragged):
    rows = rng.integers(-1, num_rows + 1, n).astype(np.int64)  # -1 and num_rows: default rows
    rows[: n // 3] = rng.integers(0, 3, n // 3)  # a few long lists
    if not ragged:
        return rows, None, 8
    seg = np.sort(rng.integers(0, 9, n)).astype(np.int32)
    return rows, ref.cursor_counts(seg, 9), 9


@pytest.mark.parametrize("op", [ref.SUM, ref.MEAN, ref.MAX, ref.MIN])
@pytest.mark.parametrize("ragged", [False, True])
def test_restatement_agrees_with_float64_autograd(op, ragged):
    """Per element within L * 2^-23 * sum|terms| (L = the row's list length): the worst case of a left-to-right
    float32 sum of L terms (each partial sum rounds once, relative error 2^-24 of a value bounded by sum|terms|; Mean's
    divide adds one more rounding per term -- hence 2^-23, not 2^-24)."""
    import torch
    rng = np.random.default_rng(5 + op + 10 * ragged)
    n, num_rows, D = 240, 17, 6
    rows, cnt, S = _request(rng, n, num_rows, ragged)
    X = rng.standard_normal((num_rows, D)).astype(np.float32)
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    start = ref.segment_starts(cnt, n, S)
    arg = ref.fold_arg(op, X, rows, start)[1] if op in (ref.MAX, ref.MIN) else None
    got = ref.backward(op, rows, cnt, grad_out, num_rows, arg)

    x = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    xd = torch.cat([x, torch.zeros(1, D, dtype=torch.float64)])  # row num_rows: the default row, no gradient
    idx = torch.tensor(np.where((rows >= 0) & (rows < num_rows), rows, num_rows))
    gathered = xd[idx]
    outs = []
    for s in range(S):
        piece = gathered[int(start[s]):int(start[s + 1])]
        if piece.shape[0] == 0:
            outs.append(torch.zeros(D, dtype=torch.float64))
        elif op == ref.SUM:
            outs.append(piece.sum(0))
        elif op == ref.MEAN:
            outs.append(piece.mean(0))
        elif op == ref.MAX:
            # the fold starts at -37: a segment below it passes no gradient (ties do not occur in random data)
            outs.append(torch.where(piece.amax(0) > -37.0, piece.amax(0), torch.full((D,), -37.0, dtype=torch.float64)))
        else:
            outs.append(piece.amin(0))
    (torch.stack(outs) * torch.tensor(grad_out, dtype=torch.float64)).sum().backward()
    want = x.grad.numpy()

    _, r, g, sel = ref.terms(op, rows, cnt, grad_out, num_rows, arg)
    bound = np.zeros((num_rows, D))
    np.add.at(bound, r, np.abs(g.astype(np.float64)) * sel)
    length = np.bincount(r, minlength=num_rows)[:, None]
    assert np.all(np.abs(got.astype(np.float64) - want) <= length * 2.0 ** -23 * bound)
    assert np.any(got != 0)


def test_restatement_drops_the_tail_and_the_out_of_range_rows():
    rows = np.array([0, 5, -1, 0, 1, 1, 0], np.int64)
    cnt = np.array([2, 0, 3], np.int32)  # positions 5 and 6 were never consumed
    g = np.array([[1.0], [10.0], [100.0]], np.float32)
    gx = ref.backward(ref.SUM, rows, cnt, g, 5)
    assert gx[:, 0].tolist() == [101.0, 100.0, 0.0, 0.0, 0.0]
    assert ref.cursor_counts(np.array([0, 0, 2, 1, 2], np.int32), 3).tolist() == [2, 0, 1]
    assert ref.cursor_counts(np.array([0, 3, 1], np.int32), 3).tolist() == [1, 0, 0]
