"""CPU tests of the fused GAT attention (glx_gat_attention and glx_gat_attention_backward): the library carries the
entry points and finds argument errors before any device use, and the numpy restatement of the contract
(gat_attention_ref.py) is the composite leaky_relu / softmax / dropout with its gradients, draws its mask from the
published Philox4x32-10 and keeps the promised share of elements."""
import ctypes
import os

import numpy as np
import pytest

import gat_attention_ref as gref
import glx

INVALID = 3


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- Philox ---------------------------------------------------------------------------------------------------

# Random123's known-answer vectors for philox4x32-10 (kat_vectors): counter, key, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = gref.philox4x32_10(np.array(ctr, np.uint32), key)
        assert [int(x) for x in got] == list(want)
    many = gref.philox4x32_10(np.array([k[0] for k in KAT[:1]] * 3, np.uint32), (0, 0))  # vectorised over counters
    assert many.shape == (3, 4) and [int(x) for x in many[2]] == list(KAT[0][2])


def test_philox_agrees_with_the_oracle():
    import oracle_bindings
    if not os.path.exists(oracle_bindings.ORACLE_SO):
        pytest.skip("the oracle library is not built")
    orc = oracle_bindings.Oracle()
    rng = np.random.default_rng(0)
    for _ in range(20):
        ctr = rng.integers(0, 2 ** 32, 4, dtype=np.uint64).astype(np.uint32)
        key = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(gref.philox4x32_10(ctr, key), orc.philox(ctr, key))


def test_dropout_keep_rate():
    """2^20 elements at p = 0.25: the kept share within 4 standard deviations (0.0017) of 0.75"""
    n, p = 1 << 20, 0.25
    for heads, seed, call in ((1, 1, 0), (4, 2 ** 40 + 7, 2 ** 33 + 1)):
        keep = gref.keep_mask(n // heads, heads, p, seed, call)
        assert keep.shape == (n // heads, heads)
        assert abs(keep.mean() - 0.75) <= 4 * np.sqrt(p * (1 - p) / n)
    a, b = gref.keep_mask(1000, 2, p, 5, 0), gref.keep_mask(1000, 2, p, 5, 1)
    assert np.array_equal(a, gref.keep_mask(1000, 2, p, 5, 0)) and not np.array_equal(a, b)
    # a prefix of a longer request draws the same words: the mask is a function of the element alone
    assert np.array_equal(a[:10], gref.keep_mask(10, 2, p, 5, 0))
    assert gref.threshold(0.25) == 2 ** 30 and gref.threshold(0.0) == 0 and float(gref.scale(0.5)) == 2.0


# ---- the restatement is the composite -------------------------------------------------------------------------

def _request(heads, ragged, seed=0):
    rng = np.random.default_rng(seed)
    M = 23
    if ragged:
        cnt = np.array([0, 5, 1, 17, -3, 40, 9, 0], np.int32)
        S, n = len(cnt), int(np.maximum(cnt, 0).sum()) + 3
    else:
        cnt, S, n = None, 9, 9 * 7
    s = rng.standard_normal((S, heads)).astype(np.float32)
    t = rng.standard_normal((M, heads)).astype(np.float32)
    rows = rng.integers(0, M, n).astype(np.int64)
    rows[::11] = -1  # padded neighbours
    g = rng.standard_normal((n, heads)).astype(np.float32)
    return s, t, rows, cnt, S, g


def torch_composite(s, t, rows, cnt, S, g, slope, default_attr, keep_scale):
    """(soft, alpha, s.grad, t.grad) of float64 CPU autograd of the composite; keep_scale[n, H] multiplies soft"""
    import torch
    n = len(rows)
    H = s.reshape(S, -1).shape[1]
    ts = torch.tensor(s.reshape(S, H), dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t.reshape(len(t), H), dtype=torch.float64, requires_grad=True)
    start = gref.starts(cnt, n, S)
    seg = gref.segment_of(cnt, n, S)
    inside = torch.tensor((rows >= 0) & (rows < len(t)))
    tv = torch.where(inside[:, None], tt[torch.tensor(np.clip(rows, 0, len(t) - 1))],
                     torch.tensor(float(default_attr), dtype=torch.float64))
    parts = [torch.zeros(0, H, dtype=torch.float64)]
    for sg in range(S):
        a, b = int(start[sg]), int(start[sg + 1])
        if a < b:
            e = torch.nn.functional.leaky_relu(ts[sg] + tv[a:b], slope)
            parts.append(torch.softmax(e, 0))
    soft = torch.cat(parts)
    used = int(start[-1])
    alpha = soft * torch.tensor(keep_scale[:used], dtype=torch.float64)
    (alpha * torch.tensor(g[:used].reshape(used, H), dtype=torch.float64)).sum().backward()
    pad = np.zeros((n - used, H))
    assert (seg[:used] < S).all()
    return (np.concatenate([soft.detach().numpy(), pad]), np.concatenate([alpha.detach().numpy(), pad]),
            ts.grad.numpy(), tt.grad.numpy())


def magnitudes(soft, ga, pre, rows, cnt, S, num_rows, slope):
    """sum |terms| behind each element of grad_s and grad_t: a position contributes |soft| (|ga| + sum |soft ga|)"""
    soft, ga = np.asarray(soft, np.float64), np.asarray(ga, np.float64)
    n = len(rows)
    start = gref.starts(cnt, n, S)
    m = np.zeros_like(soft)
    for sg in range(S):
        a, b = int(start[sg]), int(start[sg + 1])
        m[a:b] = np.abs(soft[a:b]) * (np.abs(ga[a:b]) + np.abs(soft[a:b] * ga[a:b]).sum(0))
    m *= np.where(pre > 0, 1.0, slope)
    ms = np.stack([m[int(start[sg]):int(start[sg + 1])].sum(0) for sg in range(S)])
    mt = np.zeros((num_rows, soft.shape[1]))
    ok = (rows >= 0) & (rows < num_rows)
    np.add.at(mt, rows[ok], m[ok])
    return m, ms, mt


@pytest.mark.parametrize("drop_p", [0.0, 0.4])
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("heads", [1, 3])
def test_restatement_against_float64_autograd(heads, ragged, drop_p):
    """forward inside the softmax bound of the float64 composite; the gradients relative 1e-5 of the same autograd
    over the magnitudes of their terms (the project's criterion: segments of at most 40 terms, 42 * 2^-23 < 1e-5)"""
    s, t, rows, cnt, S, g = _request(heads, ragged, seed=heads)
    slope, n = 0.2, len(rows)
    keep = gref.keep_mask(n, heads, drop_p, 11, 3)
    ks = np.where(keep, float(gref.scale(drop_p)), 0.0) if drop_p else np.ones((n, heads))
    want_soft, want_alpha, want_gs, want_gt = torch_composite(s, t, rows, cnt, S, g, slope, 0.0, ks)
    soft, bound, pre = gref.forward(s, t, rows, cnt, S, slope, 0.0)
    assert np.all(np.abs(soft - want_soft) <= bound + 1e-7 * want_soft)  # float32 logits against float64 ones
    soft32 = soft.astype(np.float32)
    alpha = gref.drop(soft32, keep, drop_p)
    assert np.allclose(alpha, want_alpha, rtol=1e-6, atol=1e-12)
    assert np.array_equal(alpha == 0, ~keep | (soft32 == 0)) if drop_p else gref.same_bits(alpha, soft32)
    grad_e, _ = gref.backward(soft32, g, pre, cnt, S, slope, keep, drop_p)
    m, ms, mt = magnitudes(soft32, gref.drop(g, keep, drop_p), pre, rows, cnt, S, len(t), slope)
    gs, _ = gref.grad_s(grad_e.astype(np.float32), cnt, S)
    gt = gref.grad_t(grad_e.astype(np.float32), rows, cnt, S, len(t))
    assert np.all(np.abs(gs - want_gs) <= 1e-5 * ms)
    assert np.all(np.abs(gt - want_gt) <= 1e-5 * mt)
    assert np.any(gs != 0) and np.any(gt != 0)


def test_restatement_obeys_the_exact_rules():
    s = np.array([[0.5], [1.0], [-2.0]], np.float32)
    t = np.array([[1.0], [1.0], [3.0]], np.float32)
    rows = np.array([2, 0, 1, 0, -1, 0, 1], np.int64)
    cnt = np.array([1, 3, 3], np.int32)
    soft, bound, pre = gref.forward(s, t, rows, cnt, 3, 0.2, -np.inf)
    assert soft[0, 0] == 1.0                                  # one position
    assert np.array_equal(soft[1:4, 0], [1 / 3] * 3)          # k equal logits
    assert soft[4, 0] == 0.0 and bound[4, 0] == 0.0           # a padded neighbour under default_attr = -inf
    assert np.allclose(soft[5:, 0], 0.5) and pre[4, 0] == -np.inf
    pre, e = gref.logits(s, t, rows, cnt, 3, 0.2, 0.0)
    assert e[5, 0] == np.float32(-1.0) * np.float32(0.2) and e[0, 0] == np.float32(3.5)
    _, e1 = gref.logits(s, t, rows, cnt, 3, 1.0)
    assert gref.same_bits(e1, pre)                            # slope 1: the identity
    _, e0 = gref.logits(s, t, rows, cnt, 3, 0.0)
    assert not e0[pre <= 0].any()                             # slope 0: relu


# ---- the library ----------------------------------------------------------------------------------------------

def test_the_library_exports_both_entry_points():
    assert "glx_gat_attention" in glx.EXPORTS and "glx_gat_attention_backward" in glx.EXPORTS
    L = ctypes.CDLL(glx.LIB_PATH)
    assert hasattr(L, "glx_gat_attention") and hasattr(L, "glx_gat_attention_backward")
    assert L.glx_abi_version() == 5


def _call(entry, num_ids=4, num_segments=2, heads=2, num_rows=3, slope=0.2, drop_p=0.0, ptr_kind=glx.PTR_HOST, **null):
    """one well-formed call (4 positions, 2 segments, 2 heads, 3 rows) with the named arguments replaced; soft=None
    etc. pass NULL for that buffer"""
    keep = {
        "s": np.ones((2, 2), np.float32), "t": np.ones((3, 2), np.float32), "rows": np.zeros(4, np.int64),
        "cnt": np.array([2, 2], np.int32), "soft": np.full((4, 2), 0.5, np.float32),
        "grad_alpha": np.ones((4, 2), np.float32), "soft_out": np.zeros((4, 2), np.float32),
        "alpha_out": np.zeros((4, 2), np.float32), "grad_e": np.zeros((4, 2), np.float32),
        "grad_s": np.zeros((2, 2), np.float32), "grad_t": np.zeros((3, 2), np.float32),
    }
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    if entry == "forward":
        rc = L.glx_gat_attention(0, ptr["s"], ptr["t"], num_rows, ptr["rows"], heads, ptr["cnt"], num_ids, num_segments,
                                 slope, 0.0, drop_p, 1, 2, ptr["soft_out"], ptr["alpha_out"], ptr_kind, None)
    else:
        rc = L.glx_gat_attention_backward(0, ptr["soft"], ptr["grad_alpha"], ptr["s"], ptr["t"], num_rows, ptr["rows"],
                                          heads, ptr["cnt"], num_ids, num_segments, slope, 0.0, drop_p, 1, 2,
                                          ptr["grad_e"], ptr["grad_s"], ptr["grad_t"], ptr_kind, None)
    return rc, L.glx_last_error().decode()


COMMON_ERRORS = [
    (dict(num_ids=-1), "negative"),
    (dict(num_segments=-1), "negative"),
    (dict(num_rows=-1), "negative"),
    (dict(heads=0), "heads"),
    (dict(heads=-2), "heads"),
    (dict(num_ids=2 ** 30, heads=4), "num_ids * heads"),
    (dict(num_segments=2 ** 30, heads=4), "num_segments * heads"),
    (dict(num_rows=2 ** 31), "num_rows"),
    (dict(slope=-0.1), "negative_slope"),
    (dict(slope=float("inf")), "negative_slope"),
    (dict(slope=float("nan")), "negative_slope"),
    (dict(drop_p=-0.1), "drop_p"),
    (dict(drop_p=1.0), "drop_p"),
    (dict(drop_p=float("nan")), "drop_p"),
    (dict(ptr_kind=5), "ptr_kind"),
    (dict(cnt=None, num_ids=3), "multiple"),
    (dict(rows=None), "rows is NULL"),
    (dict(s=None), "s is NULL"),
    (dict(t=None), "t is NULL"),
]
OWN_ERRORS = {
    "forward": [(dict(alpha_out=None), "alpha_out is NULL"), (dict(soft_out=None, drop_p=0.5), "soft_out")],
    "backward": [(dict(soft=None), "soft is NULL"), (dict(grad_alpha=None), "grad_alpha is NULL"),
                 (dict(grad_e=None), "grad_e_out is NULL")],
}


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_argument_errors_need_no_gpu(entry):
    for kwargs, word in COMMON_ERRORS + OWN_ERRORS[entry]:
        rc, msg = _call(entry, **kwargs)
        assert rc == INVALID and word in msg, (entry, kwargs, rc, msg)
