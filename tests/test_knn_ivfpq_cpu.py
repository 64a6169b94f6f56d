"""CPU checks of the IVF-PQ index: the new names on every layer, the argument validation that needs no device, and the
contract's restatement (tests/knn_ivfpq_ref.py) itself -- enough candidates re-ranked equals the IVF-Flat restatement,
every list probed on top of that the exact search, found-sets are nested in refine, and a planted codebook that holds
every residual sub-vector gives every row the code of its own codeword.  (m against dim, num_rows < 256 and the nprobe
limits need an index, hence a device: tests/test_gpu_knn_ivfpq.py.)"""
import ctypes
import os

import numpy as np
import pytest

import glx
import knn_ivf_ref
import knn_ivfpq_ref
import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glx_knn_ivfpq_build", "glx_knn_ivfpq_search", "glx_knn_ivfpq_info", "glx_knn_ivfpq_export",
         "glx_knn_ivfpq_destroy"]
METRICS = [knn_ref.L2, knn_ref.IP]
INVALID = 3


def test_names_on_every_layer():
    text = open(os.path.join(ROOT, "include", "glx.h")).read()
    L = glx.lib()
    for name in NAMES:
        assert name in glx.EXPORTS and hasattr(L, name), name
        assert ("GLX_API int %s(" % name) in text or ("GLX_API void %s(" % name) in text, name
    assert "contrib/knn/ivfpq_index.cc:25-56" in text and "index_factory.cc:35-37" in text
    assert L.glx_abi_version() == 5
    assert callable(glx.Features.build_ivfpq) and callable(glx.KnnIvf.build_pq)
    for attr in ("search", "codebooks", "codes", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(glx.KnnIvfPq, attr)), attr


def test_arguments_are_refused_without_a_device():
    L = glx.lib()
    h = ctypes.c_void_p()

    def build(m, niter=0, train_rows=0, kind=0):
        return L.glx_knn_ivfpq_build(None, m, niter, train_rows, None, kind, None, ctypes.byref(h))

    assert build(4) == INVALID and b"NULL" in L.glx_last_error() and not h.value  # a NULL IVF index
    assert build(0) == INVALID and b"m must be" in L.glx_last_error()
    assert build(65) == INVALID and b"m must be" in L.glx_last_error()
    assert build(4, niter=-1) == INVALID and b"niter" in L.glx_last_error()
    assert build(4, train_rows=-1) == INVALID and b"train_rows" in L.glx_last_error()
    assert build(4, kind=7) == INVALID
    assert L.glx_knn_ivfpq_build(None, 4, 0, 0, None, 0, None, None) == INVALID

    Q = np.ones((2, 3), np.float32)
    ids, dist = np.zeros((2, 1025), np.int64), np.zeros((2, 1025), np.float32)

    def search(k, nprobe, refine=0, metric=1, nq=2, kind=0):
        return L.glx_knn_ivfpq_search(None, metric, Q.ctypes.data, nq, k, nprobe, refine, ids.ctypes.data,
                                      dist.ctypes.data, kind, None)

    assert search(1, 1) == INVALID and b"index is NULL" in L.glx_last_error()  # a NULL index
    assert search(1, 0) == INVALID and b"nprobe" in L.glx_last_error()
    assert search(0, 1) == INVALID and b"k must be" in L.glx_last_error()
    assert search(1025, 1) == INVALID and b"k must be" in L.glx_last_error()
    assert search(5, 1, refine=4) == INVALID and b"refine" in L.glx_last_error()
    assert search(5, 1, refine=-1) == INVALID and b"refine" in L.glx_last_error()
    assert search(5, 1, refine=1025) == INVALID and b"refine" in L.glx_last_error()
    assert search(5, 1, refine=5) == INVALID and b"index is NULL" in L.glx_last_error()  # refine = k is in range
    assert search(5, 1, refine=1024) == INVALID and b"index is NULL" in L.glx_last_error()
    assert search(1, 1, refine=1024, nq=(1 << 31) // 1024) == INVALID and b"2^31" in L.glx_last_error()
    assert search(1, 1, metric=2) == INVALID and b"metric" in L.glx_last_error()
    assert search(1, 1, nq=-1) == INVALID
    assert search(1, 1, kind=7) == INVALID
    assert L.glx_knn_ivfpq_info(None, None, None, None, None) == INVALID and b"NULL" in L.glx_last_error()
    assert L.glx_knn_ivfpq_export(None, None, None, 0, None) == INVALID and b"NULL" in L.glx_last_error()
    L.glx_knn_ivfpq_destroy(None)  # a no-op


@pytest.fixture(scope="module")
def small():
    """300 tied (integer-valued) rows of 6 columns with a NaN row, 7 lists, m = 3 trained codebooks"""
    rng = np.random.default_rng(31)
    X = rng.integers(-3, 4, (300, 6)).astype(np.float32)
    Q = rng.integers(-3, 4, (9, 6)).astype(np.float32)
    X[17] = np.nan
    index = knn_ivf_ref.build(X, 7, niter=3)
    pq = knn_ivfpq_ref.build(X, index, 3, niter=2)
    return X, Q, index, pq


@pytest.mark.parametrize("metric", METRICS)
def test_enough_candidates_refined_is_the_flat_index(small, metric):
    X, Q, index, pq = small
    dist = knn_ref.scores(Q, X, metric)
    for nprobe in (1, 3):
        for k in (1, 10, 300):
            got = knn_ivfpq_ref.search(Q, X, index, pq, k, metric, nprobe, refine=300, dist=dist)
            assert knn_ref.same(got, knn_ivf_ref.search(Q, X, index, k, metric, nprobe, dist=dist)), (nprobe, k)
    for k in (1, 10, 300):
        got = knn_ivfpq_ref.search(Q, X, index, pq, k, metric, 7, refine=300, dist=dist)
        assert knn_ref.same(got, knn_ref.search(Q, X, k, metric)), k
    ids = 5 + 3 * np.arange(300, dtype=np.int64)
    got = knn_ivfpq_ref.search(Q, X, index, pq, 10, metric, 7, refine=300, ids=ids)
    assert knn_ref.same(got, knn_ref.search(Q, X, 10, metric, ids=ids))


@pytest.mark.parametrize("metric", METRICS)
def test_found_sets_are_nested_in_refine(metric):
    rng = np.random.default_rng(32)
    X = rng.standard_normal((600, 8)).astype(np.float32)
    Q = rng.standard_normal((12, 8)).astype(np.float32)
    index = knn_ivf_ref.build(X, 8, niter=3)
    pq = knn_ivfpq_ref.build(X, index, 2, niter=2)
    k, nprobe = 10, 4
    dist = knn_ref.scores(Q, X, metric)
    true_ids = knn_ref.take_k(dist, k, metric)[0]
    flat = knn_ivf_ref.found(knn_ivf_ref.search(Q, X, index, k, metric, nprobe, dist=dist)[0], true_ids)
    before = [set()] * Q.shape[0]
    for refine in (10, 11, 40, 160, 600):
        got = knn_ivfpq_ref.search(Q, X, index, pq, k, metric, nprobe, refine=refine, dist=dist)
        now = knn_ivf_ref.found(got[0], true_ids)
        assert all(b <= n for b, n in zip(before, now)), refine
        assert all(n <= f for n, f in zip(now, flat)), refine  # never more than the flat index finds in those lists
        # every returned distance is the exact one of that row
        rows = got[0]
        assert np.array_equal(knn_ref.bits(got[1][rows >= 0]),
                              knn_ref.bits(np.take_along_axis(dist, np.maximum(rows, 0), 1)[rows >= 0]))
        before = now
    assert before == flat  # every candidate re-ranked: what the flat index finds
    # refine = 0 returns the adc itself, best first, and pads beyond the candidates
    got = knn_ivfpq_ref.search(Q, X, index, pq, 599, metric, 1)
    sizes = np.diff(index["list_ptr"])
    for q, l in enumerate(knn_ivf_ref.probes(Q, index, metric, 1)[:, 0]):
        assert np.all(got[0][q, sizes[l]:] == -1) and np.all(got[0][q, :sizes[l]] >= 0)
        assert np.all(got[1][q, sizes[l]:] == knn_ref.pad_dist(metric))
        head = got[1][q, :sizes[l]]
        assert np.all(np.diff(head) >= 0) if metric == knn_ref.L2 else np.all(np.diff(head) <= 0)


def test_planted_codebooks_hold_every_residual():
    """dsub = 1 and integer data: the residuals of a column take few values; a codebook that lists them (padded with far
    codewords, the values repeated once more behind the padding) gives each row the FIRST codeword equal to its residual,
    and the L2 adc of a stored row against itself is +0"""
    rng = np.random.default_rng(33)
    X = rng.integers(-3, 4, (400, 4)).astype(np.float32)
    C = rng.integers(-2, 3, (5, 4)).astype(np.float32)
    index = knn_ivf_ref.build(X, 5, niter=0, centroids=C)
    R = knn_ivfpq_ref.residuals(X, index, index["list_rows"])
    books = np.empty((4, 256, 1), np.float32)
    for j in range(4):
        values = np.unique(R[:, j])
        far = 1000 + np.arange(256 - 2 * values.size, dtype=np.float32)
        books[j, :, 0] = np.concatenate([values, far, values])
    pq = knn_ivfpq_ref.build(X, index, 4, niter=0, codebooks=books)
    assert np.array_equal(pq["codebooks"].view(np.uint32), books.view(np.uint32))
    for j in range(4):
        values = np.unique(R[:, j])
        assert np.array_equal(pq["codes"][:, j], np.searchsorted(values, R[:, j]))
        assert np.array_equal(books[j, pq["codes"][:, j], 0], R[:, j])
    rows = index["list_rows"][:20]
    got = knn_ivfpq_ref.search(X[rows], X, index, pq, 1, knn_ref.L2, 5)
    assert np.array_equal(got[1].view(np.uint32), np.zeros((20, 1), np.uint32))  # +0.0f, bit for bit
    # ... and two builds give the same bits; the default sample is the whole table up to 65,536 rows
    again = knn_ivfpq_ref.build(X, index, 4, niter=0, codebooks=books)
    assert all(np.array_equal(pq[key].view(np.uint8), again[key].view(np.uint8)) for key in pq)
    assert knn_ivfpq_ref.train_size(400) == 400 and knn_ivfpq_ref.train_size(10 ** 7) == 65536
    assert knn_ivfpq_ref.train_size(400, 3) == 256 and knn_ivfpq_ref.train_size(400, 1000) == 400
