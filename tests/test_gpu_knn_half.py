"""glx_knn_search_ex with GLX_KNN_PREC_HALF (contract K-knn-half) against float64: exactly where every partial sum is
representable, within twice the derived bound otherwise; bit-equal across schedules, calls and pointer kinds."""
import ctypes

import numpy as np
import pytest
import torch

import glx
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, Tuned, _cuda

pytestmark = pytest.mark.gpu

DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
NAN_BITS = 0x7fc00000


def run(f, Q, k, metric, host=False, **kw):
    """(ids, dist) as numpy from canary-filled buffers, through host or device pointers"""
    out = (np.full((len(Q), k), -7, np.int64), np.full((len(Q), k), np.nan, np.float32))
    if host:
        return f.search(np.ascontiguousarray(Q), k, METRIC_NAMES[metric], out=out, **kw)
    out = f.search(_cuda(Q), k, METRIC_NAMES[metric], out=(_cuda(out[0]), _cuda(out[1])), **kw)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def ref64(Q, X, metric):
    """(dist, sum of |terms|, qn + xn) in float64 of float64 operands"""
    with np.errstate(invalid="ignore"):
        ip, terms = Q @ X.T, np.abs(Q) @ np.abs(X).T
        norms = (Q * Q).sum(1)[:, None] + (X * X).sum(1)[None, :]
        return (ip if metric == knn_ref.IP else np.maximum(norms - 2 * ip, 0)), terms, norms


def integers(dim, seed=0):
    rng = np.random.default_rng(seed + dim)
    return rng.integers(-3, 4, (300, dim)).astype(np.float32), rng.integers(-3, 4, (130, dim)).astype(np.float32)


@pytest.fixture(scope="module")
def gaussian():
    rng = np.random.default_rng(2)
    return rng.standard_normal((1500, 33)).astype(np.float32), rng.standard_normal((200, 33)).astype(np.float32)


@pytest.mark.parametrize("dim", [1, 8, 17, 80])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_small_integers(dtype, metric, dim):
    """every product, sum and L2 expression is exact: the float64 answer is the contract's, ties included"""
    X, Q = integers(dim)
    f = glx.Features(X, dtype=dtype)
    dist = ref64(Q.astype(np.float64), X.astype(np.float64), metric)[0].astype(np.float32)
    perm = knn_ref.order(dist, metric)
    for k in (1, 20, 400):
        want = knn_ref.take_k(dist, k, metric, perm=perm)
        for host in (False, True):
            assert knn_ref.same(run(f, Q, k, metric, host, precision="half"), want), (k, host)
            with Tuned(knn_chunk_rows=128, knn_query_block=128):
                assert knn_ref.same(run(f, Q, k, metric, host, precision="half"), want), (k, host, "tuned")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tolerance_and_schedule_independence(gaussian, dtype, metric):
    """tol = twice the derived bound dim * 2^-23 * sum|terms| (L2: through -2 ip, plus the two norm chains and the two
    roundings of knn_l2)"""
    X, Q = gaussian
    k, dim = 20, X.shape[1]
    Xh, Qh = (torch.from_numpy(a).to(DTYPES[dtype]).double().numpy() for a in (X, Q))
    ref, terms, norms = ref64(Qh, Xh, metric)
    tol = dim * 2.0 ** -22 * terms
    if metric == knn_ref.L2:
        tol = 2 * tol + (dim + 4) * 2.0 ** -23 * norms
    f = glx.Features(X, dtype=dtype)
    ids, dist = got = run(f, Q, k, metric, precision="half")
    rows = np.arange(len(Q))[:, None]
    err = np.abs(dist - ref[rows, ids])
    print("largest |dist - ref| / tol:", (err / tol[rows, ids]).max())
    assert np.all(err <= tol[rows, ids])
    sign = 1 if metric == knn_ref.L2 else -1
    step = sign * (dist[:, 1:].astype(np.float64) - dist[:, :-1])
    assert np.all((step > 0) | ((step == 0) & (ids[:, 1:] > ids[:, :-1])))
    left_out = np.ones(ref.shape, bool)
    left_out[rows, ids] = False
    assert not np.any(left_out & (sign * ref < sign * dist[:, -1:] - tol))
    assert knn_ref.same(run(f, Q, k, metric, precision="half"), got)
    assert knn_ref.same(run(f, Q, k, metric, host=True, precision="half"), got)
    with Tuned(knn_chunk_rows=256, knn_query_block=128):
        assert knn_ref.same(run(f, Q, k, metric, precision="half"), got)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_and_row_ends(dtype, metric, offset):
    """dim 17 at a pitch of 17 elements, as it stands and at a 2-byte pointer offset: a NaN in column 0 of row 101 is
    what a vector load over the tail of row 100 would pick up"""
    X, Q = integers(17, seed=5)
    X[7], X[0, 3], Q[:, 3] = 0, -1, -1
    Q[0] = X[0]  # an L2 distance of zero; row 7 gives every query an inner product of zero
    X[50, 3], X[101, 0], Q[2, 5] = np.inf, np.nan, np.nan
    flat = torch.zeros(X.size + offset, dtype=DTYPES[dtype], device="cuda")
    flat[offset:] = _cuda(X).reshape(-1).to(DTYPES[dtype])
    f = glx.Features(flat[offset:].view(X.shape), view=True)
    dist = ref64(Q.astype(np.float64), X.astype(np.float64), metric)[0].astype(np.float32)
    for k in (20, 300):
        ids, got = run(f, Q, k, metric, precision="half")
        assert knn_ref.same((ids, got), knn_ref.take_k(dist, k, metric)), k
        bits = got.view(np.uint32)
        assert ids[2].tolist() == list(range(k)) and np.all(bits[2] == NAN_BITS)
        assert not np.any(bits == 0x80000000)
    assert np.any(bits[0] == 0)  # k = 300 returns every row
    assert ids[1, -2:].tolist() == [50, 101] and np.isinf(got[1, -2]) and bits[1, -1] == NAN_BITS


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_refine(gaussian, dtype, metric):
    k = 20
    for dim in (1, 8, 17, 80):  # the half score is exact: the re-rank returns the default search's answer
        X, Q = integers(dim)
        f = glx.Features(X, dtype=dtype)
        want = run(f, Q, k, metric)
        for r in (k, 1024):
            got = run(f, Q, k, metric, precision="half", refine=r)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (dim, r)
    X, Q = gaussian
    f = glx.Features(X, dtype=dtype)
    all_ids, all_dist = run(f, Q, 1024, metric)
    found = []
    for r in (20, 64, 1024):
        ids, dist = run(f, Q, k, metric, precision="half", refine=r)
        at = ids[:, :, None] == all_ids[:, None, :]
        assert at.any(2).all()
        exact = all_dist[np.arange(len(Q))[:, None], at.argmax(2)]
        assert np.array_equal(dist.view(np.uint32), exact.view(np.uint32)), r
        found.append((ids[:, :, None] == all_ids[:, None, :k]).any(2).sum(1))
    assert np.all(found[0] <= found[1]) and np.all(found[1] <= found[2])


def test_arguments():
    X, Q = integers(8)
    half, f32 = glx.Features(X, dtype="bfloat16"), glx.Features(X)
    L, k = glx.lib(), 20
    for f, prec, refine, name in ((f32, 1, 0, b"precision"), (half, 1, k - 1, b"refine"), (half, 1, 1025, b"refine"),
                                  (half, 0, k, b"refine"), (half, 2, 0, b"precision")):
        ids, dist = np.full((len(Q), k), -7, np.int64), np.full((len(Q), k), 7, np.float32)
        rc = L.glx_knn_search_ex(f._h, 1, Q.ctypes.data_as(ctypes.c_void_p), len(Q), k, prec, refine,
                                 ids.ctypes.data_as(ctypes.c_void_p), dist.ctypes.data_as(ctypes.c_void_p), glx.PTR_HOST, None)
        assert rc == 3 and name in L.glx_last_error(), (prec, refine, L.glx_last_error())
        assert np.all(ids == -7) and np.all(dist == 7)
    with pytest.raises(ValueError, match="precision"):
        half.search(Q, k, precision="bfloat16")
    for f in (half, f32):
        assert knn_ref.same(run(f, Q, k, knn_ref.L2, precision="float32"), run(f, Q, k, knn_ref.L2))
    own = half.search(_cuda(Q).to(torch.bfloat16), k, precision="half")  # the table's own dtype: upcast exactly
    assert knn_ref.same((own[0].cpu().numpy(), own[1].cpu().numpy()), run(half, Q, k, knn_ref.IP, precision="half"))
