"""The IVF-PQ index (glx_knn_ivfpq_*) on the GPU against the restatement of its contract (tests/knn_ivfpq_ref.py), bit
for bit everywhere: codebooks and codes of the build; ids and adc of the coded search (refine = 0); ids and exact
distances of the re-ranked search (refine > 0), which with few enough candidates is KnnIvf.search and Features.search.
A NaN matches a NaN; a zero matches with its sign."""
import ctypes

import numpy as np
import pytest

import glx
import knn_ivf_ref
import knn_ivfpq_ref
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, NAN, Tuned, _cuda, gpu_search
from test_gpu_knn_ivf import exported, ivf_search, same_index, upcast

pytestmark = pytest.mark.gpu

INVALID = 3


def pq_search(px, Q, k, metric, nprobe, refine=0, host=False):
    """(ids, dist) as numpy; the output buffers start as canaries, so an unwritten element shows"""
    n = Q.shape[0]
    if host:
        out = (np.full((n, k), -7, np.int64), np.full((n, k), NAN, np.float32))
        px.search(np.ascontiguousarray(Q), k, METRIC_NAMES[metric], nprobe=nprobe, refine=refine, out=out)
        return out
    out = (_cuda(np.full((n, k), -7, np.int64)), _cuda(np.full((n, k), NAN, np.float32)))
    px.search(Q if glx._is_torch(Q) else _cuda(Q), k, METRIC_NAMES[metric], nprobe=nprobe, refine=refine, out=out)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def exported_pq(px):
    return {"codebooks": px.codebooks(), "codes": px.codes()}


def same_pq(got, want):
    return (got["codebooks"].shape == want["codebooks"].shape and got["codes"].dtype == np.uint8
            and np.array_equal(knn_ref.bits(got["codebooks"]), knn_ref.bits(want["codebooks"]))
            and np.array_equal(got["codes"], want["codes"]))


def check_searches(px, X, Q, index, pq, cases, ids=None):
    """cases: (k, nprobe, refine) triples, each under both metrics against the restatement over the index's own lists,
    codebooks and codes"""
    for metric in METRICS:
        dist = knn_ref.scores(Q, X, metric)
        for k, nprobe, refine in cases:
            want = knn_ivfpq_ref.search(Q, X, index, pq, k, metric, nprobe, refine=refine, ids=ids, dist=dist)
            assert knn_ref.same(pq_search(px, Q, k, metric, nprobe, refine), want), (metric, k, nprobe, refine)


def _data(rng, n, dim, tied):
    if tied:
        return (rng.integers(-4, 5, (n, dim)) / 4).astype(np.float32)
    return rng.standard_normal((n, dim)).astype(np.float32)


# ---- the build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_rows", [None, 256])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_build_equals_the_restatement(dtype, train_rows):
    rng = np.random.default_rng(41)
    X = rng.integers(-3, 4, (700, 8)).astype(np.float32) / np.float32(3)  # thirds: a half table rounds them
    f = glx.Features(X, dtype=None if dtype == "float32" else dtype)
    ix = f.build_ivf(5, niter=2)
    index = exported(ix)
    up = upcast(X, dtype)
    assert same_index(index, knn_ivf_ref.build(up, 5, niter=2))
    px = ix.build_pq(2, niter=2, train_rows=train_rows)
    got = exported_pq(px)
    assert same_pq(got, knn_ivfpq_ref.build(up, index, 2, niter=2, train_rows=train_rows))
    assert same_pq(exported_pq(ix.build_pq(2, niter=2, train_rows=train_rows)), got)  # two builds, the same bits
    info = px.info()
    assert (info["m"], info["dsub"], info["num_rows"]) == (2, 4, 700) and (px.m, px.dsub, px.ivf) == (2, 4, ix)
    assert info["device_bytes"] == 2 * 256 * (2 * 4 + 1) * 4 + 700 * 2
    # both layers at once, and as a context manager
    with f.build_ivfpq(5, 2, niter=2, train_rows=train_rows) as both:
        if train_rows is None:  # the same sample size on both layers: the same index
            assert same_index(exported(both.ivf), index) and same_pq(exported_pq(both), got)
        assert both.ivf.features is f
    assert both._h is None


@pytest.mark.parametrize("dim,m", [(8, 1), (8, 2), (8, 8), (24, 8), (66, 2), (64, 64)])
def test_build_shapes(dim, m):
    """dsub = dim, even, 1, odd (3 and 33) and the largest m; tied data where the sub-vectors are short"""
    rng = np.random.default_rng(100 * dim + m)
    N = 600
    X, Q = _data(rng, N, dim, dim == 8), _data(rng, 3, dim, dim == 8)
    f = glx.Features(X)
    ix = f.build_ivf(6, niter=1)
    index = exported(ix)
    px = ix.build_pq(m, niter=1)
    got = exported_pq(px)
    assert got["codebooks"].shape == (m, 256, dim // m) and got["codes"].shape == (N, m)
    assert same_pq(got, knn_ivfpq_ref.build(X, index, m, niter=1))
    check_searches(px, X, Q, index, got, [(10, 2, 0), (10, 6, 0), (10, 2, 40)])


def test_codebooks_are_ivf_centroids_on_the_device():
    """codebook j is Features(R_j).build_ivf(256, niter, train_rows=T).centroids(), with and without a start"""
    rng = np.random.default_rng(42)
    N, dim, m, T = 3000, 6, 2, 1000
    X = rng.standard_normal((N, dim)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(9, niter=1)
    index = exported(ix)
    start = rng.standard_normal((m, 256, 3)).astype(np.float32)
    R = knn_ivfpq_ref.residuals(X, index, knn_ivf_ref.sample_rows(N, T))
    for init in (None, start, _cuda(start)):
        books = ix.build_pq(m, niter=2, train_rows=T, codebooks=init).codebooks()
        for j in range(m):
            Rj = np.ascontiguousarray(R[:, 3 * j:3 * j + 3])
            cj = None if init is None else start[j]
            want = glx.Features(Rj).build_ivf(256, niter=2, train_rows=T, centroids=cj).centroids()
            assert np.array_equal(knn_ref.bits(books[j]), knn_ref.bits(want)), j
    # niter = 0 with codebooks only encodes
    px = ix.build_pq(m, niter=0, codebooks=start)
    got = exported_pq(px)
    assert np.array_equal(got["codebooks"].view(np.uint32), start.view(np.uint32))
    assert same_pq(got, knn_ivfpq_ref.build(X, index, m, niter=0, codebooks=start))


# ---- the coded search and the re-ranked search against the restatement ------------------------------------------
@pytest.fixture(scope="module")
def nine_hundred():
    """900 rows (100 of them tied copies) x 8 columns, 12 lists, m = 4; the exact distances come from Features.search"""
    rng = np.random.default_rng(43)
    X = rng.standard_normal((900, 8)).astype(np.float32)
    X[300:400] = X[:100]
    Q = X[rng.integers(0, 900, 129)] + np.float32(0.125)
    f = glx.Features(X)
    ix = f.build_ivf(12, niter=2)
    px = ix.build_pq(4, niter=2)
    return X, Q, f, ix, px, exported(ix), exported_pq(px)


@pytest.mark.parametrize("num_queries", [1, 2, 129])
def test_adc_search_equals_the_restatement(nine_hundred, num_queries):
    X, Q, f, ix, px, index, pq = nine_hundred
    Q = Q[:num_queries]
    check_searches(px, X, Q, index, pq, [(k, nprobe, 0) for nprobe in (1, 3, 12) for k in (1, 20, 1000)])
    for metric in METRICS:
        want = knn_ivfpq_ref.search(Q, X, index, pq, 20, metric, 3)
        assert knn_ref.same(pq_search(px, Q, 20, metric, 3, host=True), want)
        assert np.all(knn_ivfpq_ref.search(Q, X, index, pq, 1000, metric, 1)[0][:, -1] == -1)  # 1000: a padded tail


@pytest.mark.parametrize("num_queries", [2, 129])
def test_refined_search_equals_the_restatement(nine_hundred, num_queries):
    X, Q, f, ix, px, index, pq = nine_hundred
    Q = Q[:num_queries]
    check_searches(px, X, Q, index, pq, [(1, 1, 1), (20, 3, 20), (20, 3, 50), (20, 12, 1024), (7, 1, 1000)])
    for metric in METRICS:  # every returned dist is the exact search's dist of that id
        all_ids, all_dist = gpu_search(f, Q, 900, metric)
        by_row = np.take_along_axis(all_dist, np.argsort(all_ids, axis=1), 1)  # ids are rows here
        for k, nprobe, refine in ((20, 3, 50), (100, 12, 100), (1, 12, 1)):
            ids, dist = pq_search(px, Q, k, metric, nprobe, refine)
            assert np.all(ids >= 0)
            assert np.array_equal(knn_ref.bits(dist), knn_ref.bits(np.take_along_axis(by_row, ids, 1))), (k, nprobe)


def test_few_candidates_equal_the_flat_index_and_the_exact_search():
    rng = np.random.default_rng(44)
    # at most 1,024 rows, every list probed: the exact search
    X = rng.standard_normal((1000, 5)).astype(np.float32)
    X[500:600] = X[:100]
    Q = rng.standard_normal((9, 5)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(7, niter=1)
    px = ix.build_pq(5, niter=1)
    for metric in METRICS:
        for k in (1, 33, 1024):
            got = pq_search(px, Q, k, metric, 7, refine=1024)
            assert knn_ref.same(got, gpu_search(f, Q, k, metric)) and knn_ref.same(got, ivf_search(ix, Q, k, metric, 7))
        assert knn_ref.same(pq_search(px, Q, 10, metric, 7, refine=1024), knn_ref.search(Q, X, 10, metric))
    # 3,000 rows with planted short lists: queries whose probed lists hold at most `refine` rows get the flat index's
    # answer, here all of them
    sizes = [2400, 150, 200, 100, 150]
    centres = np.array([[0, 0], [20, 0], [0, 20], [20, 20], [-20, -20]], np.float32)
    of = np.repeat(np.arange(5), sizes)
    rng.shuffle(of)
    X = centres[of] + (rng.integers(-8, 9, (of.size, 2)) / 8).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(5, niter=0, centroids=centres)
    index = exported(ix)
    assert np.diff(index["list_ptr"]).tolist() == sizes
    px = ix.build_pq(2, niter=1)
    Q = centres[1:4] * np.float32(1.1) + np.float32(0.3)
    for metric in METRICS:
        lists = knn_ivf_ref.probes(Q, index, metric, 2)
        assert np.all(lists != 0) and max(sum(sizes[l] for l in row) for row in lists) <= 350
        for k, refine in ((5, 350), (350, 350), (400, 512)):
            got = pq_search(px, Q, k, metric, 2, refine=refine)
            assert knn_ref.same(got, ivf_search(ix, Q, k, metric, 2)), (metric, k)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("dim", [1, 2, 3, 31, 32, 33, 130])
def test_refine_of_every_row_over_the_column_tile_borders(dim, dtype):
    """The re-rank scores its rows with the function the IVF-Flat scan uses (knn_score_gathered): one column, an odd
    count, one short of / exactly / one past a 32-column tile, several tiles with a tail; every storage type.  With
    every list probed and refine >= num_rows the answer is Features.search on the same table, bit for bit."""
    rng = np.random.default_rng(4800 + dim)
    X, Q = _data(rng, 300, dim, False), _data(rng, 3, dim, False)
    f = glx.Features(X, dtype=None if dtype == "float32" else dtype)
    px = f.build_ivfpq(3, 1, niter=1)
    for metric in METRICS:
        for k in (1, 300):
            got = pq_search(px, Q, k, metric, 3, refine=1024)
            assert knn_ref.same(got, gpu_search(f, Q, k, metric)), (metric, k)
            if dtype == "float32":
                assert knn_ref.same(got, knn_ref.search(Q, X, k, metric)), (metric, k)


@pytest.fixture(scope="module")
def forty_thousand_lists():
    """40,000 rows x 2 columns, every row a list of its own, m = 1; the lists, codebook and codes as the device has them"""
    rng = np.random.default_rng(49)
    X = rng.standard_normal((40000, 2)).astype(np.float32)
    Q = rng.standard_normal((2, 2)).astype(np.float32)
    ix = glx.Features(X).build_ivf(40000, niter=0, centroids=X)
    px = ix.build_pq(1, niter=1)
    return X, Q, px, exported(ix), exported_pq(px)


@pytest.mark.parametrize("metric", METRICS)
def test_probe_slots_of_one_query_take_two_passes(forty_thousand_lists, metric):
    """The shape of test_gpu_knn_ivf.py's test of this name through the IVF-PQ search, whose slot plan is the same
    function (knn_slot_plan): 40,000 probed slots of RP = 1,024 keys exceed the workspace budget for one query alone,
    so the slots go in passes of 32,768 and 7,232."""
    X, Q, px, index, pq = forty_thousand_lists
    N, RP = 40000, 1024
    budget_keys = (256 << 20) // 8
    assert budget_keys // (N * RP) == 0  # not even one query's slots fit ...
    P = budget_keys // RP
    assert [min(P, N - p0) for p0 in range(0, N, P)] == [32768, 7232]  # ... so they go in two passes
    want = knn_ivfpq_ref.search(Q, X, index, pq, 10, metric, N, refine=RP)
    # every list is probed, so slot p is list p: the answer must hold rows of both passes for the case to pin the second
    list_of = np.empty(N, np.int64)
    list_of[index["list_rows"]] = np.repeat(np.arange(N), np.diff(index["list_ptr"]))
    assert (list_of[want[0]] >= P).any() and (list_of[want[0]] < P).any()
    assert knn_ref.same(pq_search(px, Q, 10, metric, N, refine=RP), want)


@pytest.mark.parametrize("metric", METRICS)
def test_found_sets_are_nested_in_refine(metric):
    rng = np.random.default_rng(45)
    centres = 3 * rng.standard_normal((16, 8))
    X = (centres[rng.integers(0, 16, 2000)] + rng.standard_normal((2000, 8))).astype(np.float32)
    Q = (centres[rng.integers(0, 16, 40)] + rng.standard_normal((40, 8))).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(16, niter=2)
    px = ix.build_pq(2, niter=2)
    k, nprobe = 20, 4
    true_ids = gpu_search(f, Q, k, metric)[0]
    flat = knn_ivf_ref.found(ivf_search(ix, Q, k, metric, nprobe)[0], true_ids)
    before = [set()] * Q.shape[0]
    for refine in (20, 21, 80, 320, 1024):
        now = knn_ivf_ref.found(pq_search(px, Q, k, metric, nprobe, refine)[0], true_ids)
        assert all(b <= n for b, n in zip(before, now)), refine
        assert all(n <= fl for n, fl in zip(now, flat)), refine
        before = now


# ---- list lengths at the borders of a scan batch (1,024 codes) and of a lane group (256) ----------------------
def _planted_lists(rng, sizes, centres, m=2, niter=1):
    of = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(of)
    X = centres[of] + (rng.integers(-8, 9, (of.size, 2)) / 8).astype(np.float32)  # ties inside a list
    f = glx.Features(X)
    ix = f.build_ivf(len(sizes), niter=0, centroids=centres)
    index = exported(ix)
    assert np.diff(index["list_ptr"]).tolist() == list(sizes)
    px = ix.build_pq(m, niter=niter)
    pq = exported_pq(px)
    assert same_pq(pq, knn_ivfpq_ref.build(X, index, m, niter=niter))
    return X, f, ix, px, index, pq


BORDER_CASES = [(1, 1, 0), (7, 1, 0), (1024, 1, 0), (1024, 3, 0), (1, 1, 1), (7, 2, 100), (1024, 1, 1024), (300, 3, 1024)]


def test_planted_lists_of_0_1_and_around_256_and_1023():
    rng = np.random.default_rng(46)
    sizes = [0, 1, 255, 256, 257, 1023]
    centres = np.array([[40, 40], [0, 0], [10, 0], [0, 10], [10, 10], [-10, -10]], np.float32)
    X, f, ix, px, index, pq = _planted_lists(rng, sizes, centres)
    Q = np.concatenate([centres + np.float32(0.3), rng.standard_normal((1, 2)).astype(np.float32)])
    check_searches(px, X, Q, index, pq, BORDER_CASES)  # k above the candidates of a list: the tail is padded
    ids, dist = pq_search(px, Q[:1], 5, knn_ref.L2, 1)  # the nearest list of query 0 is the empty one
    assert np.all(ids == -1) and np.all(dist == np.inf)
    ids, dist = pq_search(px, Q[:1], 5, knn_ref.L2, 1, refine=9)
    assert np.all(ids == -1) and np.all(dist == np.inf)


def test_planted_lists_of_1024_and_1025_and_one_that_holds_everything():
    rng = np.random.default_rng(47)
    sizes = [1024, 1025, 0, 3]
    centres = np.array([[0, 0], [10, 0], [0, 10], [10, 10]], np.float32)
    X, f, ix, px, index, pq = _planted_lists(rng, sizes, centres, m=1)
    Q = np.concatenate([centres + np.float32(0.3), rng.standard_normal((2, 2)).astype(np.float32)])
    check_searches(px, X, Q, index, pq, BORDER_CASES + [(1024, 4, 0), (1000, 4, 1024)])
    # one list holds every row
    sizes = [0, 2500, 0, 0]
    centres = np.array([[50, 50], [2, 2], [60, 60], [-70, 0]], np.float32)
    X, f, ix, px, index, pq = _planted_lists(rng, sizes, centres)
    Q = rng.standard_normal((4, 2)).astype(np.float32) + np.float32(2)
    check_searches(px, X, Q, index, pq, [(1, 1, 0), (1024, 4, 0), (33, 2, 1024), (1, 4, 1)])


def test_two_table_passes_over_several_batches():
    """m = 64 takes the look-up tables in two passes of 32; a list beyond 1,024 rows takes them again for every batch
    of codes, and the chain of a position stays one ascending sum"""
    rng = np.random.default_rng(53)
    X = rng.standard_normal((2600, 64)).astype(np.float32)
    X[:2300, 0] += np.float32(40)
    C = np.zeros((2, 64), np.float32)
    C[0, 0] = 40
    f = glx.Features(X)
    ix = f.build_ivf(2, niter=0, centroids=C)
    index = exported(ix)
    assert np.diff(index["list_ptr"]).tolist() == [2300, 300]
    px = ix.build_pq(64, niter=1, train_rows=300)
    pq = exported_pq(px)
    assert same_pq(pq, knn_ivfpq_ref.build(X, index, 64, niter=1, train_rows=300))
    Q = X[[0, 2400, 7]] + np.float32(0.125)
    check_searches(px, X, Q, index, pq, [(10, 1, 0), (1024, 2, 0), (10, 2, 100)])


# ---- special values --------------------------------------------------------------------------------------------
def _special(rng, dim=33):
    """inf elements, NaN rows and a row with one NaN column, subnormal rows and queries, zero rows and queries"""
    X = rng.standard_normal((300, dim)).astype(np.float32)
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    X[10, -1], X[11, -1], X[12, 0] = np.inf, -np.inf, np.inf
    Q[1, :] = 0
    X[20] = 0
    X[21] = -0.0
    Q[2] = 1e-30
    X[30:34] = np.nan
    X[45, 7] = np.nan
    Q[3, 2] = np.nan
    Q[4] = 3e38
    X[50:60] = (rng.integers(-100, 101, (10, dim)) * 1e-41).astype(np.float32)  # subnormal rows
    X[60:70] = X[50:60]  # ... tied
    Q[6] = (rng.integers(-100, 101, dim) * 1e-42).astype(np.float32)  # a subnormal query: products underflow
    return X, Q


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_special_values(dtype):
    rng = np.random.default_rng(48)
    X, Q = _special(rng)
    up = upcast(X, dtype)
    f = glx.Features(X, dtype=None if dtype == "float32" else dtype)
    C = up[[0, 1, 2, 3, 50, 100, 200]].copy()
    C[5, 1] = np.nan  # a NaN centroid: it takes no row that is a number, its residuals and tables are NaN
    ix = f.build_ivf(7, niter=0, centroids=C)
    index = exported(ix)
    assert same_index(index, knn_ivf_ref.build(up, 7, niter=0, centroids=C))
    # planted codebooks of numbers: a NaN row gets the contract's codes, which is the first codeword wherever its
    # residual is a NaN, and its NaN adc sorts last by row
    books = rng.standard_normal((3, 256, 11)).astype(np.float32)
    books[1, 7] = 0
    books[2, 9] = (rng.integers(-100, 101, 11) * 1e-41).astype(np.float32)
    px = ix.build_pq(3, niter=0, codebooks=books)
    pq = exported_pq(px)
    assert same_pq(pq, knn_ivfpq_ref.build(up, index, 3, niter=0, codebooks=books))
    at = {int(r): p for p, r in enumerate(index["list_rows"])}
    assert all(np.all(pq["codes"][at[r]] == 0) for r in range(30, 34)) and pq["codes"][at[45], 0] == 0
    cases = [(10, 1, 0), (300, 7, 0), (10, 3, 0), (10, 3, 40), (300, 7, 300), (1, 6, 1)]
    check_searches(px, up, Q, index, pq, cases)
    # trained codebooks: inf and NaN residuals flow into the codewords, still the restatement's bits
    px = ix.build_pq(3, niter=1)
    pq = exported_pq(px)
    assert same_pq(pq, knn_ivfpq_ref.build(up, index, 3, niter=1))
    assert np.isnan(pq["codebooks"][:, 0]).all()  # the NaN rows went to the first codeword of every sub-quantiser
    check_searches(px, up, Q, index, pq, cases)
    for metric in METRICS:  # all lists, refine = 0: the rows with a NaN adc close the list in ascending row
        ids, dist = pq_search(px, Q[:1], 300, metric, 7)
        nan_at = np.flatnonzero(np.isnan(dist[0]))
        assert nan_at.size >= 5 and nan_at[0] == 300 - nan_at.size and np.all(np.diff(ids[0, nan_at]) > 0)
        assert {30, 31, 32, 33, 45} <= set(ids[0, nan_at].tolist())


def test_inner_product_adc_of_minus_zero():
    """every term of an inner-product adc underflows to -0.0f: the sum is -0.0f, which the key cannot hold"""
    rng = np.random.default_rng(49)
    X = rng.standard_normal((300, 4)).astype(np.float32)
    C = np.array([[1e-30, 0, 0, 0], [5, 5, 5, 5]], np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(2, niter=0, centroids=C)
    index = exported(ix)
    books = np.full((2, 256, 2), 1e-30, np.float32)  # one codeword value: every code is 0
    px = ix.build_pq(2, niter=0, codebooks=books)
    pq = exported_pq(px)
    Q = np.array([[-1e-30, -1e-30, -1e-30, -1e-30], [1e-30, 1e-30, 1e-30, 1e-30]], np.float32)
    want = knn_ivfpq_ref.search(Q, X, index, pq, 5, knn_ref.IP, 2)
    assert np.all(np.signbit(want[1][0])) and np.all(want[1] == 0) and not np.any(np.signbit(want[1][1]))
    for nprobe in (1, 2):
        want = knn_ivfpq_ref.search(Q, X, index, pq, 5, knn_ref.IP, nprobe)
        assert knn_ref.same(pq_search(px, Q, 5, knn_ref.IP, nprobe), want)


# ---- layouts -----------------------------------------------------------------------------------------------------
def test_table_layouts():
    rng = np.random.default_rng(50)
    cases = [(10, 2, 0), (600, 5, 0), (10, 2, 30), (600, 6, 1024)]
    # id-mapped tables answer ids: a hash map (scattered ids) and an arithmetic one
    X = rng.standard_normal((500, 9)).astype(np.float32)
    Q = rng.standard_normal((20, 9)).astype(np.float32)
    for ids in (rng.permutation(10 ** 6)[:500].astype(np.int64) - 1000, 5 + 3 * np.arange(500, dtype=np.int64)):
        f = glx.Features(X, ids=ids)
        ix = f.build_ivf(6, niter=1)
        index = exported(ix)
        px = ix.build_pq(3, niter=1)
        pq = exported_pq(px)
        assert same_pq(pq, knn_ivfpq_ref.build(X, index, 3, niter=1))
        check_searches(px, X, Q, index, pq, cases, ids=ids)
    # from 4,096 rows on an owned table is stored swizzled with a padded stride: codes follow LOGICAL rows
    X = rng.standard_normal((4096 + 500, 6)).astype(np.float32)
    X[4000:4200] = X[100:300]  # ties across the swizzle's blocks
    Q = X[rng.integers(0, X.shape[0], 12)] + np.float32(0.25)
    owned = glx.Features(X)
    ix = owned.build_ivf(9, niter=1)
    index = exported(ix)
    px = ix.build_pq(2, niter=1, train_rows=700)
    pq = exported_pq(px)
    assert same_pq(pq, knn_ivfpq_ref.build(X, index, 2, niter=1, train_rows=700))
    cases = [(50, 1, 0), (50, 4, 0), (50, 4, 200)]
    check_searches(px, X, Q, index, pq, cases)
    # a view: the lists and codes of the build, and with refine > 0 the distances of the rows as they are now
    dX = _cuda(X)
    view = glx.Features(dX, view=True)
    vix = view.build_ivf(9, niter=1)
    assert same_index(exported(vix), index)
    vpx = vix.build_pq(2, niter=1, train_rows=700)
    assert same_pq(exported_pq(vpx), pq)
    check_searches(vpx, X, Q, index, pq, cases)
    coded = [pq_search(vpx, Q, 50, metric, 4) for metric in METRICS]
    Y = np.ascontiguousarray(X[::-1] * np.float32(1.5))
    dX.copy_(_cuda(Y))
    assert same_pq(exported_pq(vpx), pq)  # the codes stay
    for metric, before in zip(METRICS, coded):
        assert knn_ref.same(pq_search(vpx, Q, 50, metric, 4), before)  # ... and so does the coded search
        want = knn_ivfpq_ref.search(Q, Y, index, pq, 50, metric, 4, refine=200)  # stale candidates, current distances
        assert knn_ref.same(pq_search(vpx, Q, 50, metric, 4, refine=200), want)


def test_query_block_borders():
    """129 queries in blocks of 64 (the knob only shrinks the block) and, without the knob, the border the workspace
    budget draws: 299 probe slots of 1,024 keys leave room for 109 queries a block"""
    rng = np.random.default_rng(51)
    X = rng.standard_normal((1500, 6)).astype(np.float32)
    Q = rng.standard_normal((129, 6)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(300, niter=1)
    px = ix.build_pq(3, niter=1)
    index, pq = exported(ix), exported_pq(px)
    for metric in METRICS:
        for refine in (0, 40):
            want = knn_ivfpq_ref.search(Q, X, index, pq, 7, metric, 3, refine=refine)
            plain = pq_search(px, Q, 7, metric, 3, refine)
            with Tuned(knn_query_block=64):
                assert knn_ref.same(pq_search(px, Q, 7, metric, 3, refine), want)
                every = pq_search(px, Q, 7, metric, 300, refine)
            assert knn_ref.same(plain, want)
            assert knn_ref.same(pq_search(px, Q, 7, metric, 300, refine), every)
    assert (256 << 20) // 8 // (299 * 1024) == 109
    got = pq_search(px, Q, 5, knn_ref.IP, 299, refine=1024)
    with Tuned(knn_query_block=64):
        assert knn_ref.same(pq_search(px, Q, 5, knn_ref.IP, 299, refine=1024), got)
    sel = [0, 108, 109, 128]  # the restatement costs a table per (query, list): the queries at the block's border
    want = knn_ivfpq_ref.search(Q[sel], X, index, pq, 5, knn_ref.IP, 299, refine=1024)
    assert knn_ref.same((got[0][sel], got[1][sel]), want)


# ---- errors and call forms --------------------------------------------------------------------------------------
def test_errors_and_call_forms():
    import torch
    rng = np.random.default_rng(52)
    X = rng.standard_normal((300, 6)).astype(np.float32)
    Q = rng.standard_normal((3, 6)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(8, niter=1)
    L = glx.lib()
    h = ctypes.c_void_p()
    assert L.glx_knn_ivfpq_build(ix._h, 4, 0, 0, None, 0, None, ctypes.byref(h)) == INVALID  # 6 % 4 != 0
    assert b"divide" in L.glx_last_error() and not h.value
    for m in (0, 65, 4, -1):
        with pytest.raises(glx.GlxError) as e:
            ix.build_pq(m)
        assert e.value.code == INVALID
    small = glx.Features(X[:255]).build_ivf(4, niter=1)
    with pytest.raises(glx.GlxError) as e:
        small.build_pq(2)  # fewer rows than codewords
    assert e.value.code == INVALID and "num_rows" in str(e.value)
    for shape in ((2, 256, 2), (3, 255, 2), (3, 256, 3), (3, 512)):
        with pytest.raises(ValueError):
            ix.build_pq(3, codebooks=np.zeros(shape, np.float32))
    px = ix.build_pq(3, niter=1)
    index, pq = exported(ix), exported_pq(px)
    for k, refine in ((5, 4), (5, 1), (5, 1025), (5, -1)):
        with pytest.raises(glx.GlxError) as e:
            px.search(Q, k, refine=refine)
        assert e.value.code == INVALID and "refine" in str(e.value)
    for nprobe in (0, 9):
        with pytest.raises(glx.GlxError):
            px.search(Q, 5, nprobe=nprobe)
    for k in (0, 1025):
        with pytest.raises(glx.GlxError):
            px.search(Q, k, out=(np.zeros((3, k), np.int64), np.zeros((3, k), np.float32)))
    with pytest.raises(ValueError):
        px.search(np.ones((2, 5), np.float32), 1)
    with pytest.raises(ValueError):
        px.search(Q, 1, metric="cosine")
    good = (np.zeros((3, 5), np.int64), np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError):
        px.search(Q, 5, out=(np.zeros((3, 4), np.int64), good[1]))
    # out=, the default buffers (numpy in, numpy out; torch in, torch out on the current stream), no queries
    got = px.search(Q, 5, "l2", nprobe=2, refine=9, out=good)
    assert got[0] is good[0] and got[1] is good[1]
    assert knn_ref.same(good, knn_ivfpq_ref.search(Q, X, index, pq, 5, knn_ref.L2, 2, refine=9))
    ids, dist = px.search(Q, 5, nprobe=2)
    want = knn_ivfpq_ref.search(Q, X, index, pq, 5, knn_ref.IP, 2)
    assert isinstance(ids, np.ndarray) and knn_ref.same((ids, dist), want)
    dQ = _cuda(Q)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ids, dist = px.search(dQ, 5, nprobe=2)
    side.synchronize()
    assert ids.is_cuda and knn_ref.same((ids.cpu().numpy(), dist.cpu().numpy()), want)
    assert L.glx_knn_ivfpq_search(px._h, 1, None, 0, 5, 2, 0, None, None, 0, None) == 0
    # a closed index refuses; closing twice is fine; an index over a closed IVF index refuses as well
    px.close()
    px.close()
    assert px._h is None
    with pytest.raises(ValueError):
        px.search(Q, 5)
    with pytest.raises(ValueError):
        px.info()
    fresh = ix.build_pq(2, niter=1)
    assert fresh.info()["m"] == 2 and fresh.info()["dsub"] == 3
    ix.close()
    with pytest.raises(ValueError):
        fresh.search(Q, 5)
    with pytest.raises(ValueError):
        ix.build_pq(2)
    # the index keeps its IVF index and table alive
    keep = glx.Features(X).build_ivfpq(4, 2, niter=1)
    import gc
    gc.collect()
    assert knn_ref.same(pq_search(keep, Q, 5, knn_ref.L2, 4, refine=300), knn_ref.search(Q, X, 5, knn_ref.L2))
