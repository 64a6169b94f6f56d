"""CPU checks of the IVF-Flat index: the new names on every layer, the argument validation that needs no device, and the
contract's restatement (tests/knn_ivf_ref.py) itself -- all lists probed equals the exact search, found-sets are nested
in nprobe, and the build's invariants.  (nlist > num_rows and nprobe > nlist need a table and an index, hence a device:
tests/test_gpu_knn_ivf.py.)"""
import os

import numpy as np
import pytest

import glx
import knn_ivf_ref
import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glx_knn_ivf_build", "glx_knn_ivf_search", "glx_knn_ivf_info", "glx_knn_ivf_export", "glx_knn_ivf_destroy"]
METRICS = [knn_ref.L2, knn_ref.IP]
INVALID = 3


def test_names_on_every_layer():
    text = open(os.path.join(ROOT, "include", "glx.h")).read()
    L = glx.lib()
    for name in NAMES:
        assert name in glx.EXPORTS and hasattr(L, name), name
        assert ("GLX_API int %s(" % name) in text or ("GLX_API void %s(" % name) in text, name
    assert "contrib/knn/ivfflat_index.cc:25-55" in text and "index_factory.cc:32-34" in text
    assert L.glx_abi_version() == 5
    assert callable(glx.Features.build_ivf)
    for attr in ("search", "centroids", "lists", "info", "close"):
        assert callable(getattr(glx.KnnIvf, attr)), attr


def test_arguments_are_refused_without_a_device():
    import ctypes
    L = glx.lib()
    h = ctypes.c_void_p()

    def build(f, nlist, niter=0, train_rows=0, kind=0):
        return L.glx_knn_ivf_build(f, nlist, niter, train_rows, None, kind, None, ctypes.byref(h))

    assert build(None, 4) == INVALID and b"NULL" in L.glx_last_error() and not h.value  # a NULL table
    assert build(None, 0) == INVALID and b"nlist" in L.glx_last_error()
    assert build(None, 65537) == INVALID and b"nlist" in L.glx_last_error()
    assert build(None, 4, niter=-1) == INVALID and b"niter" in L.glx_last_error()
    assert build(None, 4, train_rows=-1) == INVALID and b"train_rows" in L.glx_last_error()
    assert build(None, 4, kind=7) == INVALID
    assert L.glx_knn_ivf_build(None, 4, 0, 0, None, 0, None, None) == INVALID

    Q = np.ones((2, 3), np.float32)
    ids, dist = np.zeros((2, 1025), np.int64), np.zeros((2, 1025), np.float32)

    def search(k, nprobe, metric=1, nq=2, kind=0):
        return L.glx_knn_ivf_search(None, metric, Q.ctypes.data, nq, k, nprobe, ids.ctypes.data, dist.ctypes.data, kind, None)

    assert search(1, 1) == INVALID and b"index is NULL" in L.glx_last_error()  # a NULL index
    assert search(1, 0) == INVALID and b"nprobe" in L.glx_last_error()
    assert search(0, 1) == INVALID and b"k must be" in L.glx_last_error()
    assert search(1025, 1) == INVALID and b"k must be" in L.glx_last_error()
    assert search(1, 1, metric=2) == INVALID and b"metric" in L.glx_last_error()
    assert search(1, 1, nq=-1) == INVALID
    assert search(1, 1, kind=7) == INVALID
    assert L.glx_knn_ivf_info(None, None, None, None, None, None) == INVALID and b"NULL" in L.glx_last_error()
    assert L.glx_knn_ivf_export(None, None, None, None, 0, None) == INVALID and b"NULL" in L.glx_last_error()
    L.glx_knn_ivf_destroy(None)  # a no-op


def _tied(rng, n, nq, dim):
    """integer-valued rows and queries: ties between rows and between centroids"""
    return rng.integers(-3, 4, (n, dim)).astype(np.float32), rng.integers(-3, 4, (nq, dim)).astype(np.float32)


@pytest.mark.parametrize("metric", METRICS)
def test_all_lists_probed_is_the_exact_search(metric):
    rng = np.random.default_rng(1)
    X, Q = _tied(rng, 300, 9, 4)
    X[17] = np.nan
    index = knn_ivf_ref.build(X, 7, niter=3)
    for k in (1, 10, 400):
        assert knn_ref.same(knn_ivf_ref.search(Q, X, index, k, metric, 7), knn_ref.search(Q, X, k, metric)), k
    ids = 5 + 3 * np.arange(300, dtype=np.int64)
    assert knn_ref.same(knn_ivf_ref.search(Q, X, index, 10, metric, 7, ids=ids), knn_ref.search(Q, X, 10, metric, ids=ids))


@pytest.mark.parametrize("metric", METRICS)
def test_found_sets_are_nested_in_nprobe(metric):
    rng = np.random.default_rng(2)
    X = rng.standard_normal((500, 6)).astype(np.float32)
    Q = rng.standard_normal((12, 6)).astype(np.float32)
    index = knn_ivf_ref.build(X, 16, niter=4)
    k = 20
    true_ids = knn_ref.search(Q, X, k, metric)[0]
    before = [set()] * Q.shape[0]
    for nprobe in (1, 2, 4, 8, 16):
        got = knn_ivf_ref.search(Q, X, index, k, metric, nprobe)
        now = knn_ivf_ref.found(got[0], true_ids)
        assert all(b <= n for b, n in zip(before, now)), nprobe
        before = now
    assert all(len(n) == k for n in before)  # every list probed: all of them
    # fewer candidates than k: the tail is padded
    got = knn_ivf_ref.search(Q, X, index, 499, metric, 1)
    sizes = np.diff(index["list_ptr"])
    for q, l in enumerate(knn_ivf_ref.probes(Q, index, metric, 1)[:, 0]):
        assert np.all(got[0][q, sizes[l]:] == -1) and np.all(got[0][q, :sizes[l]] >= 0)
        assert np.all(got[1][q, sizes[l]:] == knn_ref.pad_dist(metric))


def test_build_invariants():
    rng = np.random.default_rng(3)
    X, _ = _tied(rng, 300, 1, 5)
    for train_rows in (None, 100):
        index = knn_ivf_ref.build(X, 7, niter=3, train_rows=train_rows)
        ptr, rows = index["list_ptr"], index["list_rows"]
        assert ptr[0] == 0 and ptr[-1] == 300 and np.all(np.diff(ptr) >= 0)
        assert np.array_equal(np.sort(rows), np.arange(300))  # every row in exactly one list
        for l in range(7):
            assert np.all(np.diff(rows[ptr[l]:ptr[l + 1]]) > 0)  # ascending within a list
        again = knn_ivf_ref.build(X, 7, niter=3, train_rows=train_rows)
        assert all(np.array_equal(index[key].view(np.uint8), again[key].view(np.uint8)) for key in index)
    assert knn_ivf_ref.train_size(300, 7) == 300 and knn_ivf_ref.train_size(10 ** 7, 4096) == 256 * 4096
    assert knn_ivf_ref.train_size(300, 7, 3) == 7 and knn_ivf_ref.train_size(300, 7, 1000) == 300
    assert knn_ivf_ref.sample_rows(10, 4).tolist() == [0, 2, 5, 7]
    # 16 planted centroids over 5 distinct row values: a centroid without rows keeps its value through the updates,
    # duplicates of a centroid lose every row to the first of them
    values = np.arange(5, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    Y = values[rng.integers(0, 5, 200)]
    C = np.concatenate([values, values + np.float32(0.25), values, np.full((1, 3), 100, np.float32)])
    index = knn_ivf_ref.build(Y, 16, niter=2, centroids=C)
    sizes = np.diff(index["list_ptr"])
    assert np.all(sizes[:5] > 0) and np.all(sizes[5:] == 0) and sizes.sum() == 200
    assert np.array_equal(index["centroids"][5:], C[5:]) and np.array_equal(index["centroids"][:5], values)
    # the mean is a sequential float32 sum from +0.0f: -0.0 rows give +0.0, and the order of the rows shows
    assert not np.signbit(knn_ivf_ref.mean_rows(np.full((3, 2), -0.0, np.float32))).any()
    R = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    assert knn_ivf_ref.mean_rows(R)[0] != knn_ivf_ref.mean_rows(R[::-1])[0]
