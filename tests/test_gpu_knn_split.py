"""Features.search(split=True) / GLX_KNN_PREC_SPLIT (contract K-knn-split) against float64: exact and bit-equal to the
default search where every partial sum is an integer below 2^24, within the header's bound otherwise; bit-equal across
chunkings, calls and pointer kinds."""
import ctypes

import numpy as np
import pytest
import torch

import glx
import knn_ref
from test_gpu_knn import METRICS, Tuned, _cuda
from test_gpu_knn_half import NAN_BITS, ref64, run

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


def table(X, view):
    """an owned table, or a view of X at a 4-byte pointer offset with a pitch of dim elements"""
    if not view:
        return glx.Features(X)
    flat = torch.zeros(X.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = _cuda(X).reshape(-1)
    return glx.Features(flat[1:].view(X.shape), view=True)


def want32(Q, X, metric):
    with np.errstate(over="ignore", invalid="ignore"):
        return ref64(Q.astype(np.float64), X.astype(np.float64), metric)[0].astype(np.float32)


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("dim", [1, 8, 17, 80, 160])
@pytest.mark.parametrize("metric", METRICS)
def test_exact_on_integers(metric, dim, view):
    """|v| <= 300 with odd values above 256: the m pieces are not zero, every product and partial sum is an integer
    below 2^24, so float64 is the contract's answer and the default search's bits"""
    rng = np.random.default_rng(dim)
    X, Q = (rng.integers(-300, 301, (n, dim)).astype(np.float32) for n in (700, 130))
    assert np.any((np.abs(X) > 256) & (X % 2 == 1))
    ip, terms, norms = ref64(Q.astype(np.float64), X.astype(np.float64), knn_ref.IP)
    assert 1.03 * terms.max() < 2 ** 24 and (norms + 2 * np.abs(ip)).max() < 2 ** 24  # the six pairs' sums; L2's
    f = table(X, view)
    dist = want32(Q, X, metric)
    perm = knn_ref.order(dist, metric)
    for k in (20, 300):
        want = knn_ref.take_k(dist, k, metric, perm=perm)
        for host in (False, True):
            assert knn_ref.same(run(f, Q, k, metric, host), want), (k, host, "default")
            assert knn_ref.same(run(f, Q, k, metric, host, split=True), want), (k, host)
            with Tuned(knn_chunk_rows=128, knn_query_block=128):
                assert knn_ref.same(run(f, Q, k, metric, host, split=True), want), (k, host, "tuned")


@pytest.mark.parametrize("dim", [17, 80])
@pytest.mark.parametrize("metric", METRICS)
def test_bound_schedule_and_refine(metric, dim):
    """bound: the header's formula for ip.  L2 goes through -2 ip and adds the two norm chains (dim fmaf roundings each)
    and the two roundings of knn_l2: 2 * bound + (dim + 4) * 2^-23 * (qn + xn), the half scan's test's reasoning"""
    rng = np.random.default_rng(dim)
    X, Q = (rng.standard_normal((n, dim)).astype(np.float32) for n in (1500, 200))
    k, rows = 20, np.arange(200)[:, None]
    ref, terms, norms = ref64(Q.astype(np.float64), X.astype(np.float64), metric)
    bound = (6.2 * dim + 2) * 2.0 ** -23 * terms + 6 * dim * 2.0 ** -126
    bound += 2.0 ** -133 * (np.abs(Q).sum(1, dtype=np.float64)[:, None] + np.abs(X).sum(1, dtype=np.float64)[None, :])
    if metric == knn_ref.L2:
        bound = 2 * bound + (dim + 4) * 2.0 ** -23 * norms
    f = glx.Features(X)
    ids, dist = got = run(f, Q, k, metric, split=True)
    err = np.abs(dist - ref[rows, ids])
    print("largest |dist - float64| / bound:", (err / bound[rows, ids]).max())
    assert np.all(err <= bound[rows, ids])
    assert knn_ref.same(run(f, Q, k, metric, split=True), got)
    assert knn_ref.same(run(f, Q, k, metric, host=True, split=True), got)
    with Tuned(knn_chunk_rows=256, knn_query_block=128):
        assert knn_ref.same(run(f, Q, k, metric, split=True), got)
    all_ids, all_dist = run(f, Q, 1024, metric)  # the exact search
    found = []
    for r in (k, 1024):
        ids, dist = run(f, Q, k, metric, split=True, refine=r)
        at = ids[:, :, None] == all_ids[:, None, :]
        assert at.any(2).all()
        assert np.array_equal(dist.view(np.uint32), all_dist[rows, at.argmax(2)].view(np.uint32)), r
        found.append((ids[:, :, None] == all_ids[:, None, :k]).any(2).sum(1))
    assert np.all(found[0] <= found[1])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("metric", METRICS)
def test_special_values_and_row_ends(metric, offset):
    """dim 17 at a pitch of 17 elements: a NaN in column 0 of row 101 is what a vector load over the tail of row 100
    would pick up.  The row with an infinity scores NaN (0 * inf among the piece products), FLT_MAX, a float32
    subnormal and -0.0 rank where float64 puts them"""
    rng = np.random.default_rng(5)
    X, Q = (rng.integers(-3, 4, (n, 17)).astype(np.float32) for n in (300, 130))
    X[7], X[0, 3], Q[:, 3] = 0, -1, -1
    Q[0] = X[0]  # an L2 distance of zero; row 7 gives every query an inner product of zero
    X[60, 3], X[61, 4] = FLT_MAX, -0.0
    X[62], X[62, 3], X[62, 5] = 0, 1, 2.0 ** -140
    X[50, 3], X[101, 0], Q[2, 5] = np.inf, np.nan, np.nan
    flat = torch.zeros(X.size + offset, dtype=torch.float32, device="cuda")
    flat[offset:] = _cuda(X).reshape(-1)
    f = glx.Features(flat[offset:].view(X.shape), view=True)
    dist = want32(Q, X, metric)
    dist[:, 50] = np.nan
    for k in (20, 300):
        ids, got = run(f, Q, k, metric, split=True)
        assert knn_ref.same((ids, got), knn_ref.take_k(dist, k, metric)), k
        bits = got.view(np.uint32)
        assert ids[2].tolist() == list(range(k)) and np.all(bits[2] == NAN_BITS)
        assert not np.any(bits == 0x80000000)
    assert np.any(bits[0] == 0)  # k = 300 returns every row
    assert ids[1, -3:].tolist() == [60, 50, 101] and np.all(bits[1, -2:] == NAN_BITS)


def test_refusals():
    rng = np.random.default_rng(0)
    X, Q = (rng.integers(-3, 4, (n, 8)).astype(np.float32) for n in (300, 130))
    half, f32 = glx.Features(X, dtype="bfloat16"), glx.Features(X)
    L, k, vp = glx.lib(), 20, ctypes.c_void_p
    ix = f32.build_ivf(4, niter=1)
    calls = (
        (b"precision", lambda q, i, d: L.glx_knn_search_tiled(half._h, 1, q, len(Q), k, 2, 0, 0, i, d, glx.PTR_HOST, None)),
        (b"tile", lambda q, i, d: L.glx_knn_search_tiled(f32._h, 1, q, len(Q), k, 2, 0, 1, i, d, glx.PTR_HOST, None)),
        (b"refine", lambda q, i, d: L.glx_knn_search_ex(f32._h, 1, q, len(Q), k, 2, k - 1, i, d, glx.PTR_HOST, None)),
        (b"precision", lambda q, i, d: L.glx_knn_ivf_search_prec(ix._h, 1, q, len(Q), k, 4, 1, 2, 0, i, d, glx.PTR_HOST, None)),
    )
    for name, call in calls:
        ids, dist = np.full((len(Q), k), -7, np.int64), np.full((len(Q), k), 7, np.float32)
        rc = call(Q.ctypes.data_as(vp), ids.ctypes.data_as(vp), dist.ctypes.data_as(vp))
        assert rc == 3 and name in L.glx_last_error(), L.glx_last_error()
        assert np.all(ids == -7) and np.all(dist == 7)
    with pytest.raises(ValueError, match="precision"):
        half.search(Q, k, precision="half", split=True)
