"""The list-major schedule of the IVF-Flat search (KnnIvf.search(schedule="list"), glx_knn_ivf_search_ex) on the GPU:
against a float64 brute force on data whose arithmetic is exact, and bit for bit against the query-major schedule on
Gaussian data with inf / NaN / -0.0, through the candidate-overflow redo and through both pointer kinds."""
import numpy as np
import pytest

import glx
import knn_ivf_ref
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, NAN, Tuned, _cuda

pytestmark = pytest.mark.gpu

INVALID = 3


def run(ix, Q, k, metric, nprobe, schedule, host=False):
    """(ids, dist) as numpy; the output buffers start as canaries, so an unwritten element shows"""
    n = Q.shape[0]
    out = (np.full((n, k), -7, np.int64), np.full((n, k), NAN, np.float32))
    if host:
        ix.search(np.ascontiguousarray(Q), k, METRIC_NAMES[metric], nprobe=nprobe, out=out, schedule=schedule)
        return out
    out = (_cuda(out[0]), _cuda(out[1]))
    ix.search(_cuda(Q), k, METRIC_NAMES[metric], nprobe=nprobe, out=out, schedule=schedule)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


# ---- against a plain float64 reference, exactly ------------------------------------------------------------------
SIZES = [1, 128, 129, 300, 200, 50, 77, 0]  # rows of the planted lists; the last centroid repeats the one before


def brute64(Q, X, index, lists, k, metric):
    """float64 scores of the rows of every query's probed lists, ordered by (distance, storage row)"""
    ptr, rows = index["list_ptr"], index["list_rows"]
    Q, X = Q.astype(np.float64), X.astype(np.float64)
    ids = np.full((Q.shape[0], k), -1, np.int64)
    dist = np.full((Q.shape[0], k), knn_ref.pad_dist(metric), np.float64)
    for q in range(Q.shape[0]):
        cand = np.sort(np.concatenate([rows[ptr[l]:ptr[l + 1]] for l in lists[q]]))
        d = X[cand] @ Q[q] if metric == knn_ref.IP else ((X[cand] - Q[q]) ** 2).sum(1)
        best = np.lexsort((cand, -d if metric == knn_ref.IP else d))[:k]
        ids[q, :best.size], dist[q, :best.size] = cand[best], d[best]
    return ids, dist


@pytest.mark.parametrize("dim", [1, 2, 33])  # VALU only; one MFMA step; a second k-tile and the odd last column
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("metric", METRICS)
def test_exact_integer_data_equals_a_float64_brute_force(metric, dtype, dim):
    """Rows, queries and centroids are integers in [-3, 3]: every product, sum and L2 expression is exact in float32, so
    the float64 result is the contract's, ties (which are everywhere) included.  Column 0 names a row's list."""
    rng = np.random.default_rng(100 + dim)
    C = np.zeros((8, dim), np.float32)
    C[:, 0] = [-3, -2, -1, 0, 1, 2, 3, 3]
    X = rng.integers(-3, 4, (sum(SIZES), dim)).astype(np.float32)
    X[:, 0] = rng.permutation(np.repeat(C[:, 0], SIZES))
    Q = rng.integers(-3, 4, (130, dim)).astype(np.float32)
    Q[:129, 0] = 0  # 129 queries share their probe ranks: two query tiles, the second with one query
    ix = glx.Features(X, dtype=None if dtype == "float32" else dtype).build_ivf(8, niter=0, centroids=C)
    ptr, rows = ix.lists()
    index = {"centroids": C, "list_ptr": ptr, "list_rows": rows}
    assert np.diff(ptr).tolist() == SIZES
    for nprobe in (1, 2, 8):  # the seed round only; one list-major pass; every list, no coarse step
        lists = knn_ivf_ref.probes(Q, index, metric, nprobe)
        assert nprobe == 1 or np.bincount(lists[:, 1:].ravel()).max() >= 129
        for k in (1, 20, 300):  # 300: more than some queries reach, the tail is -1 with -inf / +inf
            want_ids, want_dist = brute64(Q, X, index, lists, k, metric)
            ids, dist = run(ix, Q, k, metric, nprobe, "list")
            assert np.array_equal(ids, want_ids), (nprobe, k)
            assert np.array_equal(dist, want_dist.astype(np.float32)), (nprobe, k)


# ---- bit for bit against the query-major schedule ----------------------------------------------------------------
@pytest.fixture(scope="module")
def gaussian():
    """1,500 x 33 with one +inf, one NaN and a row of -0.0, a NaN in one query: a zero-padded tile would leak 0 * inf.
    -> (index, queries, {(metric, nprobe, k): the query-major result})"""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((1500, 33)).astype(np.float32)
    X[100, 32], X[700, 5], X[900] = np.inf, np.nan, -0.0
    Q = rng.standard_normal((200, 33)).astype(np.float32)
    Q[17, 3] = np.nan
    ix = glx.Features(X).build_ivf(7, niter=2)
    cases = [(m, nprobe, k) for m in METRICS for nprobe in (3, 7) for k in (1, 50)]
    return ix, Q, {c: run(ix, Q, c[2], c[0], c[1], "query") for c in cases}


def test_list_schedule_equals_the_query_schedule(gaussian):
    ix, Q, want = gaussian
    for (metric, nprobe, k), ref in want.items():
        dev = run(ix, Q, k, metric, nprobe, "list")
        assert knn_ref.same(dev, ref), (metric, nprobe, k)
        assert knn_ref.same(run(ix, Q, k, metric, nprobe, "list", host=True), ref), (metric, nprobe, k)
        assert knn_ref.same(run(ix, Q, k, metric, nprobe, "list"), dev), (metric, nprobe, k)  # the same bits again


def test_candidate_overflow_is_redone_not_truncated(gaussian):
    """four candidate keys per query: most queries overflow and take the query-major redo; blocks of 64 queries"""
    ix, Q, want = gaussian
    with Tuned(knn_list_cand_cap=4, knn_query_block=64):
        for (metric, nprobe, k), ref in want.items():
            assert knn_ref.same(run(ix, Q, k, metric, nprobe, "list"), ref), (metric, nprobe, k)
    for (metric, nprobe, k), ref in want.items():  # the knobs are back at their defaults
        assert knn_ref.same(run(ix, Q, k, metric, nprobe, "list"), ref), (metric, nprobe, k)


def test_schedule_arguments(gaussian):
    ix, Q, _ = gaussian
    with pytest.raises(ValueError):
        ix.search(Q, 5, nprobe=2, schedule="rows")
    ids, dist = np.full((200, 5), -7, np.int64), np.full((200, 5), NAN, np.float32)
    L = glx.lib()
    rc = L.glx_knn_ivf_search_ex(ix._h, 1, Q.ctypes.data, 200, 5, 2, 7, ids.ctypes.data, dist.ctypes.data, 0, None)
    assert rc == INVALID and b"schedule" in L.glx_last_error()
    assert np.all(ids == -7) and np.all(np.isnan(dist))
