"""CPU tests of the trainable embedding tables (glx_rows_coalesce and glx_embedding_update): argument errors are found
before any device use, a well-formed call without a device fails loudly, the numpy restatement of the contracts
(embedding_ref.py) is torch's SGD / Adagrad / SparseAdam on sparse gradients and glx_aggregate_backward's Sum for short
lists, the chunk rule shows in the bits, and the optimizers' bookkeeping orders pending gradients by forward."""
import ctypes
import os
import sys

import numpy as np
import pytest

import agg_backward_ref as aref
import embedding_ref as eref
import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

INVALID, UNAVAILABLE = 3, 14


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _coalesce(n=5, num_rows=7, dim=4, ptr_kind=glx.PTR_HOST, **null):
    """one well-formed call (5 positions, a table of 7 rows, dim 4) with the named arguments replaced; rows=None etc.
    pass NULL for that buffer"""
    keep = {"rows": np.array([0, 6, 0, -1, 7], np.int64), "g": np.ones((5, 4), np.float32),
            "urows": np.zeros(5, np.int64), "ug": np.zeros((5, 4), np.float32), "count": np.zeros(1, np.int64)}
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    rc = L.glx_rows_coalesce(0, ptr["rows"], n, num_rows, dim, ptr["g"], ptr["urows"], ptr["ug"], ptr["count"], ptr_kind,
                             None)
    return rc, L.glx_last_error().decode()


def _update(algo=glx.EMB_ADAM, n=2, num_rows=7, dim=4, states=None, **null):
    """one well-formed call; the buffers are host memory, which no call here gets far enough to touch.  states: which
    of (state1, state2) are passed (default: what the algo uses)"""
    keep = {"W": np.ones((7, 4), np.float32), "urows": np.array([0, 6], np.int64), "ug": np.ones((2, 4), np.float32)}
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    s = [np.zeros((7, 4), np.float32), np.zeros((7, 4), np.float32)]
    if states is None:
        states = {glx.EMB_SGD: (False, False), glx.EMB_ADAGRAD: (True, False)}.get(algo, (True, True))
    s1, s2 = (_p(s[i]) if states[i] else None for i in range(2))
    L = glx.lib()
    rc = L.glx_embedding_update(0, algo, ptr["W"], s1, s2, num_rows, dim, ptr["urows"], ptr["ug"], n, 0.1, 1e-8, 0.9, 0.1,
                                0.999, 0.001, None)
    return rc, L.glx_last_error().decode()


COALESCE_ERRORS = [
    (dict(rows=None), "rows is NULL"),
    (dict(g=None), "g is NULL"),
    (dict(urows=None), "urows_out is NULL"),
    (dict(ug=None), "ug_out is NULL"),
    (dict(count=None), "num_unique_out is NULL"),
    (dict(n=0, count=None), "num_unique_out is NULL"),
    (dict(n=-1), "negative"),
    (dict(num_rows=-1), "negative"),
    (dict(dim=0), "dim"),
    (dict(dim=-4), "dim"),
    (dict(num_rows=2 ** 31 - 1), "num_rows"),
    (dict(num_rows=2 ** 40), "num_rows"),
    (dict(n=2 ** 29, dim=4), "n * dim"),
    (dict(ptr_kind=5), "ptr_kind"),
]
UPDATE_ERRORS = [
    (dict(W=None), "W is NULL"),
    (dict(urows=None), "urows is NULL"),
    (dict(ug=None), "ug is NULL"),
    (dict(n=-1), "negative"),
    (dict(num_rows=-1), "negative"),
    (dict(dim=0), "dim"),
    (dict(num_rows=2 ** 31 - 1), "num_rows"),
    (dict(n=2 ** 29, dim=4), "n * dim"),
    (dict(algo=3), "algo"),
    (dict(algo=-1), "algo"),
    (dict(algo=glx.EMB_SGD, states=(True, False)), "state"),
    (dict(algo=glx.EMB_SGD, states=(False, True)), "state"),
    (dict(algo=glx.EMB_ADAGRAD, states=(False, False)), "state1 is NULL"),
    (dict(algo=glx.EMB_ADAGRAD, states=(True, True)), "state2"),
    (dict(algo=glx.EMB_ADAM, states=(False, True)), "state1 is NULL"),
    (dict(algo=glx.EMB_ADAM, states=(True, False)), "state2 is NULL"),
]


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "glx.h")).read()
    for name, value in (("GLX_EMB_SGD", glx.EMB_SGD), ("GLX_EMB_ADAGRAD", glx.EMB_ADAGRAD), ("GLX_EMB_ADAM", glx.EMB_ADAM),
                        ("GLX_COALESCE_CHUNK", glx.COALESCE_CHUNK)):
        assert "#define %s %d\n" % (name, value) in text, name
    assert (eref.SGD, eref.ADAGRAD, eref.ADAM, eref.CHUNK) == (0, 1, 2, 256) and glx.COALESCE_CHUNK == 256
    assert "#define GLX_ABI_VERSION 5\n" in text


def test_argument_errors_name_the_fault():
    for call, errors in ((_coalesce, COALESCE_ERRORS), (_update, UPDATE_ERRORS)):
        for kwargs, word in errors:
            rc, msg = call(**kwargs)
            assert rc == INVALID, (call.__name__, kwargs, rc, msg)
            assert msg and word in msg, (call.__name__, kwargs, msg)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_well_formed_calls_fail_loudly_without_a_device():
    for kwargs in ({}, {"n": 0}, {"num_rows": 2 ** 31 - 2}):
        rc, msg = _coalesce(**kwargs)
        assert rc == UNAVAILABLE, (kwargs, rc, msg)
    for kwargs in ({}, {"algo": glx.EMB_SGD}, {"algo": glx.EMB_ADAGRAD}, {"n": 0}):
        rc, msg = _update(**kwargs)
        assert rc == UNAVAILABLE, (kwargs, rc, msg)
    with pytest.raises(glx.GlxError) as e:
        glx.rows_coalesce(np.array([0, 1], np.int64), np.ones((2, 4), np.float32), 3)
    assert e.value.code == UNAVAILABLE


# ---- the restatement ------------------------------------------------------------------------------------------
def _sparse_grad(ids, g, num_rows):
    """the COO gradient torch's embedding backward would produce: out-of-range positions dropped, not coalesced"""
    import torch
    keep = (ids >= 0) & (ids < num_rows)
    return torch.sparse_coo_tensor(torch.tensor(ids[keep][None]), torch.tensor(g[keep]), (num_rows, g.shape[1]))


@pytest.mark.parametrize("algo", [eref.SGD, eref.ADAGRAD, eref.ADAM])
def test_restatement_is_torch_s_optimizer_on_sparse_gradients(algo):
    """float64, three steps, ids with repeats and out-of-range values, against torch.optim on CPU: 1e-12 relative"""
    import torch
    rng = np.random.default_rng(11 + algo)
    V, D, n, lr = 9, 5, 14, 0.05
    W = rng.standard_normal((V, D))
    W0 = W.copy()
    p = torch.nn.Parameter(torch.tensor(W.copy()))
    if algo == eref.SGD:
        opt = torch.optim.SGD([p], lr=lr)
    elif algo == eref.ADAGRAD:
        opt = torch.optim.Adagrad([p], lr=lr, eps=1e-10)
    else:
        opt = torch.optim.SparseAdam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    s1 = np.zeros((V, D)) if algo != eref.SGD else None
    s2 = np.zeros((V, D)) if algo == eref.ADAM else None
    for t in range(1, 4):
        ids = rng.integers(-1, V + 1, n).astype(np.int64)
        ids[0], ids[1], ids[2], ids[3] = -1, V, 4, 4
        g = rng.standard_normal((n, D))
        p.grad = _sparse_grad(ids, g, V)
        opt.step()
        urows, ug, U = eref.coalesce(ids, g, V, dtype=np.float64)
        assert U == len(set(ids[(ids >= 0) & (ids < V)].tolist())) and np.all(urows[U:] == -1)
        if algo == eref.ADAM:
            sc = eref.adam_scalars(lr, (0.9, 0.999), 1e-8, t)
        else:
            sc = (lr, 1e-10 if algo == eref.ADAGRAD else 0.0, 0.0, 0.0, 0.0, 0.0)
        eref.update(algo, W, urows, ug, s1, s2, *sc, dtype=np.float64)
        want = p.detach().numpy()
        assert np.all(np.abs(W - want) <= 1e-12 * np.abs(want)), (algo, t, np.abs(W - want).max())
    assert np.any(W != W0)


def test_restatement_coalesce_is_the_sum_backward_for_short_lists():
    """lists of at most 256 positions: the rows of agg_backward_ref's Sum (one position per segment), bit for bit"""
    rng = np.random.default_rng(4)
    V, D, n = 12, 6, 700
    rows = rng.integers(-1, V + 1, n).astype(np.int64)
    rows[rows == 3] = 5  # row 3 referenced by nobody
    rows[:256] = 7  # exactly 256 positions ...
    rows[256:][rows[256:] == 7] = 8  # ... and no more
    g = (rng.standard_normal((n, D)) * 10.0 ** rng.integers(-3, 4, (n, D))).astype(np.float32)
    urows, ug, U = eref.coalesce(rows, g, V)
    assert np.bincount(rows[(rows >= 0) & (rows < V)]).max() == 256
    want = aref.backward(aref.SUM, rows, None, g, V)
    assert urows[:U].tolist() == sorted(set(rows[(rows >= 0) & (rows < V)].tolist())) and 3 not in urows
    assert eref.same_bits(ug, want[urows[:U]])
    assert eref.same_bits(eref.plain_sum(rows, g, V)[1], ug)


def test_the_chunk_rule_shows_in_the_bits():
    """256 terms of 1.0 then 3 terms of 2^-17: plain ascending order loses every small term against 256 (half an ulp of
    256 is 2^-16); under the contract the second chunk sums them first: 256 + 3 * 2^-17 rounds to 256 + 2^-15"""
    rows = np.zeros(259, np.int64)
    g = np.concatenate([np.ones(256, np.float32), np.full(3, 2.0 ** -17, np.float32)])[:, None]
    _, ug, U = eref.coalesce(rows, g, 1)
    assert U == 1 and ug[0, 0] == np.float32(256 + 2.0 ** -15) and ug[0, 0] != np.float32(256)
    assert eref.plain_sum(rows, g, 1)[1][0, 0] == np.float32(256)


def test_restatement_update_rounds_every_operation():
    """SGD on one element where a fused multiply-subtract differs from multiply-then-subtract"""
    a = np.float32(1 + 2.0 ** -12)
    W = np.array([[a * a]], np.float32)  # rounded
    eref.update(eref.SGD, W, np.array([0, -1, 1], np.int64), np.array([[a]], np.float32), alpha=float(a))
    assert W[0, 0] == 0.0 and np.float64(a) * np.float64(a) != np.float64(np.float32(a * a))


def test_same_bits_matches_nan_with_nan_and_tells_the_zeros_apart():
    nan, other = np.float32(np.nan), np.array([0x7fc00001], np.uint32).view(np.float32)[0]
    assert eref.same_bits(np.array([nan, 1.0]), np.array([other, 1.0]))
    assert not eref.same_bits(np.array([0.0]), np.array([-0.0]))
    assert not eref.same_bits(np.array([nan]), np.array([1.0]))


# ---- the optimizers' bookkeeping, on CPU tensors ------------------------------------------------------------------
def test_pending_entries_are_ordered_by_forward_and_dropped_by_zero_grad():
    import torch
    from graphlearn.nn.pytorch import SparseAdam, SparseEmbedding, SparseSGD
    a, b = SparseEmbedding(5, 3, device="cpu", seed=1), SparseEmbedding(5, 3, device="cpu", seed=1)
    assert torch.equal(a.weight, b.weight) and not list(a.parameters()) and "weight" in a.state_dict()
    assert abs(float(SparseEmbedding(2000, 16, device="cpu").weight.std()) - 0.25) < 0.02  # dim ** -0.5
    opt = SparseSGD([a, b], lr=0.5)
    ids = [torch.tensor([0, 1]), torch.tensor([1, 2, 3]), torch.tensor([4])]
    grads = [torch.full((len(i), 3), float(k)) for k, i in enumerate(ids)]
    # backward ran in the order 3, 1, 2 of the forwards
    a._pending = [(3, ids[2], grads[2], False), (1, ids[0], grads[0], True), (2, ids[1], grads[1], False)]
    got_ids, got_g, direct = opt._collect(a)
    assert got_ids.tolist() == [0, 1, 1, 2, 3, 4] and got_g[:, 0].tolist() == [0, 0, 1, 1, 1, 2] and not direct
    b._pending = [(1, ids[0], grads[0], True)]
    assert opt._collect(b)[2] is True  # one entry, marked distinct: no coalesce
    b._pending = [(1, ids[0], grads[0], False)]
    assert opt._collect(b)[2] is False
    opt.zero_grad()
    assert a._pending == [] and b._pending == []
    opt.lr = 0.25
    assert opt.lr == 0.25 and SparseAdam(a, lr=0.01).state_dict()["state"][0]["step"] == 0
    with pytest.raises(ValueError, match="CUDA"):
        a(torch.tensor([0]))
    with pytest.raises(ValueError, match="int64"):
        a(torch.tensor([0], dtype=torch.int32))
