"""CPU checks of the KNN contract's restatement (tests/knn_ref.py) itself: the chain against float64 within the derived
bound, ids against a float64 brute force on well-separated data, the tie / NaN order, the padding, and the merge."""
import numpy as np
import pytest

import glx
import knn_ref

METRICS = [knn_ref.L2, knn_ref.IP]


def _separated(rng, n, nq, dim):
    """Rows on a coarse integer lattice plus small noise; each query sits next to one row: every gap between two
    scores of a query is far above float32 rounding."""
    X = (rng.integers(-8, 9, (n, dim)) + rng.uniform(-0.05, 0.05, (n, dim))).astype(np.float32)
    planted = rng.integers(0, n, nq)
    Q = (X[planted] + rng.uniform(-0.01, 0.01, (nq, dim))).astype(np.float32)
    return X, Q, planted


@pytest.mark.parametrize("metric", METRICS)
def test_ids_equal_float64_brute_force_on_separated_data(metric):
    rng = np.random.default_rng(1)
    X, Q, planted = _separated(rng, 400, 30, 16)
    ids, dist = knn_ref.search(Q, X, 10, metric)
    want = knn_ref.brute64(Q, X, 10, metric)
    assert np.array_equal(ids, want)
    if metric == knn_ref.L2:
        assert np.array_equal(ids[:, 0], planted)


@pytest.mark.parametrize("dim", [1, 3, 33, 130, 1024])
def test_chain_lies_inside_the_derived_bound(dim):
    """dim + 2 roundings of relative size 2^-24 at most, each on a partial sum no larger than sum|q_c x_c| (to first
    order; the + 2 covers the second-order terms): |ip - ip64| <= (dim + 2) * 2^-24 * sum|q_c x_c|."""
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((50, dim)).astype(np.float32)
    Q = rng.standard_normal((20, dim)).astype(np.float32)
    ip = knn_ref.scores(Q, X, knn_ref.IP).astype(np.float64)
    Q64, X64 = Q.astype(np.float64), X.astype(np.float64)
    ip64 = Q64 @ X64.T
    mag = np.abs(Q64) @ np.abs(X64).T
    assert np.all(np.abs(ip - ip64) <= (dim + 2) * 2.0 ** -24 * mag)
    l2 = knn_ref.scores(Q, X, knn_ref.L2).astype(np.float64)
    qn, xn = (Q64 * Q64).sum(1)[:, None], (X64 * X64).sum(1)[None, :]
    l264 = np.maximum(qn + xn - 2 * ip64, 0)
    assert np.all(np.abs(l2 - l264) <= (dim + 4) * 2.0 ** -24 * (qn + xn + 2 * mag))


def test_chain_is_single_rounding():
    """fmaf(a, a, -round(a * a)) is the exact rounding error of the product; a twice-rounded emulation returns 0"""
    a = np.float32(1.0 + 2.0 ** -12)
    p = np.float32(a * a)
    got = knn_ref.scores(np.array([[a, np.float32(1)]], np.float32), np.array([[a, -p]], np.float32), knn_ref.IP)
    # chain: fmaf(a, a, 0) = p, then fmaf(1, -p, p) = 0; the other order shows the residue
    got2 = knn_ref.scores(np.array([[np.float32(1), a]], np.float32), np.array([[-p, a]], np.float32), knn_ref.IP)
    assert got[0, 0] == 0.0
    assert got2[0, 0] == np.float32(float(a) * float(a) - float(p)) and got2[0, 0] != 0.0


@pytest.mark.parametrize("metric", METRICS)
def test_tie_order_is_by_row(metric):
    base = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    X = np.tile(base, (100, 1))  # row r is base[r % 3]
    Q = np.array([[1, 0], [0.5, 0.5]], np.float32)
    ids, dist = knn_ref.search(Q, X, 150, metric)
    for q in range(2):
        for a in range(149):
            da, db = dist[q, a], dist[q, a + 1]
            assert da <= db if metric == knn_ref.L2 else da >= db
            if da == db:
                assert ids[q, a] < ids[q, a + 1]
    # query 1 scores rows of kinds 0 and 1 alike: they interleave by row
    if metric == knn_ref.IP:
        assert ids[0, :3].tolist() == [0, 2, 3]
    assert +0.0 == -0.0
    # a product that underflows rounds to -0.0f (the chain's +0.0f start only absorbs an exact zero)
    z = np.array([[0.0], [-1e-30], [1e-30]], np.float32)
    zi, zd = knn_ref.search(np.array([[1e-30]], np.float32), z, 3, knn_ref.IP)
    assert zi.tolist() == [[0, 1, 2]] and np.signbit(zd[0]).tolist() == [False, True, False]


@pytest.mark.parametrize("metric", METRICS)
def test_nan_scores_come_last_by_row(metric):
    X = np.full((300, 3), np.nan, np.float32)
    good = [7, 50, 123, 200, 299]
    X[good] = np.arange(15, dtype=np.float32).reshape(5, 3)
    ids, dist = knn_ref.search(np.ones((1, 3), np.float32), X, 10, metric)
    assert sorted(ids[0, :5].tolist()) == good and not np.isnan(dist[0, :5]).any()
    assert ids[0, 5:].tolist() == [0, 1, 2, 3, 4] and np.isnan(dist[0, 5:]).all()
    # a NaN query: every score is a NaN, rows in order
    ids, dist = knn_ref.search(np.array([[np.nan, 0, 0]], np.float32), X, 4, metric)
    assert ids.tolist() == [[0, 1, 2, 3]] and np.isnan(dist).all()


@pytest.mark.parametrize("metric", METRICS)
def test_k_beyond_the_table_pads(metric):
    X = np.arange(6, dtype=np.float32).reshape(3, 2)
    ids, dist = knn_ref.search(np.ones((2, 2), np.float32), X, 5, metric, ids=[10, 20, 30])
    assert sorted(ids[0, :3].tolist()) == [10, 20, 30] and ids[:, 3:].tolist() == [[-1, -1]] * 2
    assert np.all(dist[:, 3:] == (np.inf if metric == knn_ref.L2 else -np.inf))


@pytest.mark.parametrize("metric", METRICS)
def test_merge_of_three_row_ranges_equals_the_whole_search(metric):
    rng = np.random.default_rng(5)
    X = rng.integers(-2, 3, (90, 2)).astype(np.float32)  # many ties
    X[17] = np.nan
    Q = rng.integers(-2, 3, (7, 2)).astype(np.float32)
    k = 40  # beyond one range's 25 / 30 / 35 rows: padded parts
    cuts = [0, 25, 55, 90]
    parts = [knn_ref.search(Q, X[a:b], k, metric, ids=np.arange(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    got = knn_ref.merge(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), metric)
    assert knn_ref.same(got, knn_ref.search(Q, X, k, metric))


def test_python_surface_exists():
    assert {"glx_knn_search", "glx_knn_merge"} <= set(glx.EXPORTS)
    assert glx.KNN_METRICS == {"l2": 0, "ip": 1}
    assert callable(glx.Features.search) and callable(glx.knn_merge)
    L = glx.lib()
    assert L.glx_knn_search(None, 1, None, 1, 1, None, None, 0, None) == 3  # a NULL table
    assert b"NULL" in L.glx_last_error()
    assert L.glx_knn_merge(0, 1, 1, None, None, 0, 0, None, None, 0, None) == 3  # k = 0
    assert L.glx_tune(b"knn_chunk_rows", -1) == 0 and L.glx_tune(b"knn_query_block", -1) == 0
