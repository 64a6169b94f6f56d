"""The IVF-Flat index (glx_knn_ivf_*) on the GPU.  The build against the restatement of its contract
(tests/knn_ivf_ref.py) bit for bit; a search that probes every list against Features.search bit for bit; a search that
probes fewer against the restatement over the index's own lists bit for bit (ids exactly, dist with the sign of zero, a
NaN matches a NaN)."""
import ctypes

import numpy as np
import pytest

import glx
import knn_ivf_ref
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, NAN, Tuned, _cuda, gpu_search

pytestmark = pytest.mark.gpu

INVALID = 3


def ivf_search(ix, Q, k, metric, nprobe, host=False):
    """(ids, dist) as numpy; the output buffers start as canaries, so an unwritten element shows"""
    n = Q.shape[0]
    if host:
        out = (np.full((n, k), -7, np.int64), np.full((n, k), NAN, np.float32))
        ix.search(np.ascontiguousarray(Q), k, METRIC_NAMES[metric], nprobe=nprobe, out=out)
        return out
    out = (_cuda(np.full((n, k), -7, np.int64)), _cuda(np.full((n, k), NAN, np.float32)))
    ix.search(Q if glx._is_torch(Q) else _cuda(Q), k, METRIC_NAMES[metric], nprobe=nprobe, out=out)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def exported(ix):
    ptr, rows = ix.lists()
    return {"centroids": ix.centroids(), "list_ptr": ptr, "list_rows": rows}


def same_index(got, want):
    return (np.array_equal(knn_ref.bits(got["centroids"]), knn_ref.bits(want["centroids"]))
            and np.array_equal(got["list_ptr"], want["list_ptr"]) and np.array_equal(got["list_rows"], want["list_rows"]))


def upcast(X, dtype):
    import torch
    return X if dtype == "float32" else torch.from_numpy(X).to(getattr(torch, dtype)).to(torch.float32).numpy()


def check_lists(index, N):
    ptr, rows = index["list_ptr"], index["list_rows"]
    assert ptr[0] == 0 and ptr[-1] == N and np.all(np.diff(ptr) >= 0)
    assert np.array_equal(np.sort(rows), np.arange(N))
    for l in range(ptr.shape[0] - 1):
        assert np.all(np.diff(rows[ptr[l]:ptr[l + 1]]) > 0), l


def check_against_both(f, ix, X, Q, ks, nprobes, ids=None, index=None):
    """every list probed equals Features.search; fewer equal the restatement over the index's own lists"""
    index = exported(ix) if index is None else index
    for metric in METRICS:
        dist = knn_ref.scores(Q, X, metric)
        for k in ks:
            assert knn_ref.same(ivf_search(ix, Q, k, metric, ix.nlist), gpu_search(f, Q, k, metric)), (metric, k)
            for nprobe in nprobes:
                want = knn_ivf_ref.search(Q, X, index, k, metric, nprobe, ids=ids, dist=dist)
                assert knn_ref.same(ivf_search(ix, Q, k, metric, nprobe), want), (metric, k, nprobe)


# ---- the build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_rows", [None, 100])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_build_equals_the_restatement(dtype, train_rows):
    rng = np.random.default_rng(11)
    X = rng.integers(-3, 4, (300, 5)).astype(np.float32)  # integer-valued: ties between rows and between centroids
    f = glx.Features(X, dtype=None if dtype == "float32" else dtype)
    ix = f.build_ivf(7, niter=3, train_rows=train_rows)
    got = exported(ix)
    want = knn_ivf_ref.build(upcast(X, dtype), 7, niter=3, train_rows=train_rows)
    assert same_index(got, want)
    check_lists(got, 300)
    assert same_index(exported(f.build_ivf(7, niter=3, train_rows=train_rows)), got)  # two builds, the same bits
    info = ix.info()
    assert (info["nlist"], info["dim"], info["num_rows"]) == (7, 5, 300) and ix.nlist == 7
    assert info["longest_list"] == np.diff(got["list_ptr"]).max()
    assert info["device_bytes"] == 7 * 5 * 4 + 8 * 4 + 300 * 4


def test_build_defaults_and_centroid_forms():
    """the default sample of a table beyond 256 * nlist rows, a swizzled table, non-integer data; planted centroids from
    the host and from the device"""
    rng = np.random.default_rng(12)
    X = rng.standard_normal((4096 + 700, 6)).astype(np.float32)
    f = glx.Features(X)
    got = exported(f.build_ivf(3, niter=2))  # T = 768 of 4,796 rows
    assert knn_ivf_ref.train_size(4796, 3) == 768
    assert same_index(got, knn_ivf_ref.build(X, 3, niter=2))
    C = rng.standard_normal((5, 6)).astype(np.float32)
    want = knn_ivf_ref.build(X, 5, niter=1, train_rows=1000, centroids=C)
    assert same_index(exported(f.build_ivf(5, niter=1, train_rows=1000, centroids=C)), want)
    assert same_index(exported(f.build_ivf(5, niter=1, train_rows=1000, centroids=_cuda(C))), want)
    with pytest.raises(ValueError):
        f.build_ivf(5, centroids=C[:4])


def planted(X, C, dtype=None, ids=None):
    f = glx.Features(X, ids=ids, dtype=dtype)
    ix = f.build_ivf(C.shape[0], niter=0, centroids=C)
    got = exported(ix)
    assert same_index(got, knn_ivf_ref.build(upcast(X, dtype or "float32"), C.shape[0], niter=0, centroids=C))
    check_lists(got, X.shape[0])
    return f, ix, got


def test_planted_empty_lists_one_full_list_and_the_nlist_limits():
    rng = np.random.default_rng(13)
    values = np.arange(5, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    X = values[rng.integers(0, 5, 400)]
    Q = rng.standard_normal((5, 3)).astype(np.float32)
    # 16 centroids, 5 distinct row values: eleven lists stay empty (duplicates lose every row to the first of them)
    C = np.concatenate([values, values + np.float32(0.25), values, np.full((1, 3), 100, np.float32)])
    f, ix, got = planted(X, C)
    sizes = np.diff(got["list_ptr"])
    assert np.all(sizes[:5] > 0) and np.all(sizes[5:] == 0)
    check_against_both(f, ix, X, Q, (1, 10, 500), (1, 2, 15), index=got)
    # niter > 0 from the same start: the empty lists keep their centroids
    kept = exported(f.build_ivf(16, niter=2, centroids=C))
    assert same_index(kept, knn_ivf_ref.build(X, 16, niter=2, centroids=C))
    assert np.array_equal(kept["centroids"][5:], C[5:])
    # one list holds every row
    C = np.array([[50, 50, 50], [2, 2, 2], [60, 60, 60], [-70, 0, 0]], np.float32)
    f, ix, got = planted(X, C)
    assert np.diff(got["list_ptr"]).tolist() == [0, 400, 0, 0] and ix.info()["longest_list"] == 400
    check_against_both(f, ix, X, Q, (1, 500), (1, 3), index=got)
    # nlist = 1 and nlist = N
    f, ix, got = planted(X, np.zeros((1, 3), np.float32))
    check_against_both(f, ix, X, Q, (1, 500), (), index=got)
    Y = rng.integers(-2, 3, (129, 3)).astype(np.float32)  # duplicates: some of the 129 lists are empty
    f, ix, got = planted(Y, Y.copy())
    assert np.diff(got["list_ptr"]).min() == 0
    check_against_both(f, ix, Y, Q, (1, 10, 200), (1, 2, 128), index=got)
    ix = f.build_ivf(129, niter=2)  # the default start with T = nlist = N
    assert same_index(exported(ix), knn_ivf_ref.build(Y, 129, niter=2))


def test_planted_lists_at_the_sorted_batch_borders():
    """lists of 1,023 / 1,024 / 1,025 and 2,100 rows (a sorted batch of the fold is 1,024 keys, a scoring pass 256
    rows), one of 3 and an empty one; k up to the whole batch"""
    rng = np.random.default_rng(14)
    sizes = [1023, 1024, 1025, 2100, 3, 0]
    centres = np.array([[0, 0], [10, 0], [0, 10], [10, 10], [-10, -10], [30, 30]], np.float32)
    of = np.repeat(np.arange(6), sizes)
    rng.shuffle(of)
    X = centres[of] + (rng.integers(-8, 9, (of.size, 2)) / 8).astype(np.float32)  # ties inside a list
    f, ix, got = planted(X, centres)
    assert np.diff(got["list_ptr"]).tolist() == sizes and ix.info()["longest_list"] == 2100
    Q = np.concatenate([centres[:5] + np.float32(0.3), rng.standard_normal((2, 2)).astype(np.float32)])
    check_against_both(f, ix, X, Q, (1, 1024), (1, 2, 5), index=got)
    dist = knn_ref.scores(Q, X, knn_ref.L2)
    for k in (2, 100, 1023):
        want = knn_ivf_ref.search(Q, X, got, k, knn_ref.L2, 1, dist=dist)
        assert knn_ref.same(ivf_search(ix, Q, k, knn_ref.L2, 1, host=True), want), k


def test_planted_nan_row_and_nan_centroid():
    rng = np.random.default_rng(15)
    X = rng.integers(-3, 4, (500, 4)).astype(np.float32)
    X[77] = np.nan  # every distance a NaN: the first centroid takes it
    X[78, 2] = np.nan
    C = rng.integers(-3, 4, (6, 4)).astype(np.float32)
    C[2, 1] = np.nan  # takes no row (every other centroid is a number for the rows that are numbers); probed last
    f, ix, got = planted(X, C)
    ptr, rows = got["list_ptr"], got["list_rows"]
    assert ptr[3] == ptr[2] and {77, 78} <= set(rows[ptr[0]:ptr[1]].tolist())
    Q = rng.integers(-3, 4, (6, 4)).astype(np.float32)
    Q[5, 0] = np.nan  # every coarse score a NaN: the lists in order
    check_against_both(f, ix, X, Q, (1, 10, 600), (1, 2, 5), index=got)
    for metric in METRICS:
        assert np.all(knn_ivf_ref.probes(Q[:5], got, metric, 5) != 2)
    # a NaN centroid at the front takes exactly the rows whose distances are all NaN
    C[0] = np.nan
    f, ix, got = planted(X, C)
    assert got["list_rows"][:got["list_ptr"][1]].tolist() == [77, 78]
    # ... and the updates leave a centroid that took NaN rows a NaN
    kept = exported(f.build_ivf(6, niter=2, centroids=C))
    assert same_index(kept, knn_ivf_ref.build(X, 6, niter=2, centroids=C)) and np.isnan(kept["centroids"][0]).all()


# ---- every list probed: the flat search, bit for bit ----------------------------------------------------------
def _data(rng, n, dim):
    """small dims draw from a handful of values (ties everywhere), larger ones from a normal distribution"""
    if dim <= 3:
        return (rng.integers(-4, 5, (n, dim)) / 4).astype(np.float32)
    return rng.standard_normal((n, dim)).astype(np.float32)


@pytest.mark.parametrize("num_rows", [1, 129, 3000])
@pytest.mark.parametrize("dim", [1, 2, 3, 31, 32, 33, 130])
def test_all_lists_equal_the_flat_search(dim, num_rows):
    rng = np.random.default_rng(1000 * dim + num_rows)
    X, Q = _data(rng, num_rows, dim), _data(rng, 9, dim)
    f = glx.Features(X)
    ix = f.build_ivf(min(num_rows, 12), niter=2)
    dQ = _cuda(Q)
    for metric in METRICS:
        for k in (1, 10, 1024):  # 1024 > N pads; with N = 3,000 it fills the whole list
            assert knn_ref.same(ivf_search(ix, dQ, k, metric, ix.nlist), gpu_search(f, dQ, k, metric)), (metric, k)
    if num_rows == 3000:  # ... and against the restatement, so that both being wrong alike would show
        assert knn_ref.same(ivf_search(ix, dQ, 10, knn_ref.L2, ix.nlist), knn_ref.search(Q, X, 10, knn_ref.L2))


def _special(rng, dim=33):
    """test_gpu_knn.py::test_special_values' table: inf, 0 * inf, chains that underflow to -0.0f, NaN rows, and
    subnormal rows and queries"""
    X = rng.standard_normal((300, dim)).astype(np.float32)
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    X[10, -1], X[11, -1], X[12, 0] = np.inf, -np.inf, np.inf
    Q[1, :] = 0
    X[20] = 0
    X[20, -1] = -1e-30
    X[21] = 0
    X[21, 4] = -1e-30
    X[21, 5:] = -0.0
    Q[2] = 1e-30
    X[30:40] = np.nan
    X[45, 7] = np.nan
    Q[3, 2] = np.nan
    Q[4] = 3e38
    X[50:60] = (rng.integers(-100, 101, (10, dim)) * 1e-41).astype(np.float32)  # subnormal rows
    X[60:70] = X[50:60]  # ... tied
    Q[5] = (rng.integers(1, 100, dim) * 1e3).astype(np.float32)
    Q[6] = (rng.integers(-100, 101, dim) * 1e-42).astype(np.float32)  # a subnormal query: products underflow
    return X, Q


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_special_values_and_half_tables(dtype):
    rng = np.random.default_rng(16)
    X, Q = _special(rng)
    up = upcast(X, dtype)
    f = glx.Features(X, dtype=None if dtype == "float32" else dtype)
    C = up[[0, 1, 2, 3, 50, 100, 200]].copy()
    ix = f.build_ivf(7, niter=0, centroids=C)
    index = exported(ix)
    assert same_index(index, knn_ivf_ref.build(up, 7, niter=0, centroids=C))
    check_against_both(f, ix, up, Q, (1, 10, 300), (1, 3, 6), index=index)
    for metric in METRICS:  # the flat search is itself right here
        assert knn_ref.same(ivf_search(ix, Q, 10, metric, 7), knn_ref.search(Q, up, 10, metric))
    ix2 = f.build_ivf(7, niter=2)  # NaN and inf rows flow into the centroids: still the restatement's bits
    assert same_index(exported(ix2), knn_ivf_ref.build(up, 7, niter=2))


def test_table_layouts():
    rng = np.random.default_rng(17)
    # id-mapped tables answer ids: a hash map (scattered ids) and an arithmetic one
    X = rng.standard_normal((500, 9)).astype(np.float32)
    Q = rng.standard_normal((20, 9)).astype(np.float32)
    for ids in (rng.permutation(10 ** 6)[:500].astype(np.int64) - 1000, 5 + 3 * np.arange(500, dtype=np.int64)):
        f = glx.Features(X, ids=ids)
        ix = f.build_ivf(6, niter=2)
        assert same_index(exported(ix), knn_ivf_ref.build(X, 6, niter=2))
        check_against_both(f, ix, X, Q, (1, 600), (1, 5), ids=ids)
    # from 4,096 rows on an owned table is stored swizzled: lists hold LOGICAL rows
    X = rng.standard_normal((4096 + 500, 6)).astype(np.float32)
    X[4000:4200] = X[100:300]  # ties across the swizzle's blocks
    Q = X[rng.integers(0, X.shape[0], 12)] + np.float32(0.25)
    owned = glx.Features(X)
    ix = owned.build_ivf(9, niter=2)
    assert same_index(exported(ix), knn_ivf_ref.build(X, 9, niter=2))
    check_against_both(owned, ix, X, Q, (50,), (1, 4))
    # a view: the lists of the build, the distances of the rows as they are now
    dX = _cuda(X)
    view = glx.Features(dX, view=True)
    vix = view.build_ivf(9, niter=2)
    index = exported(vix)
    assert same_index(index, exported(ix))
    check_against_both(view, vix, X, Q, (50,), (1, 4), index=index)
    Y = np.ascontiguousarray(X[::-1] * np.float32(1.5))
    dX.copy_(_cuda(Y))
    check_against_both(view, vix, Y, Q, (50,), (1, 4), index=index)  # stale lists, current distances (and norms)


def test_more_lists_than_the_coarse_search_serves():
    """nlist = 2,000 > 1,024: probing every list needs no coarse step; the coarse step serves up to 1,024"""
    rng = np.random.default_rng(18)
    X = rng.standard_normal((3000, 7)).astype(np.float32)
    Q = rng.standard_normal((5, 7)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(2000, niter=1)
    index = exported(ix)
    assert same_index(index, knn_ivf_ref.build(X, 2000, niter=1))
    check_against_both(f, ix, X, Q, (1, 100), (3, 1024), index=index)
    L = glx.lib()
    out = np.zeros((5, 4), np.int64), np.zeros((5, 4), np.float32)
    rc = L.glx_knn_ivf_search(ix._h, 1, Q.ctypes.data, 5, 4, 1025, out[0].ctypes.data, out[1].ctypes.data, 0, None)
    assert rc == INVALID and b"nprobe" in L.glx_last_error()


# ---- fewer lists probed: the restatement over the index's lists, bit for bit ------------------------------------
@pytest.mark.parametrize("num_queries", [1, 2, 129])
def test_probed_search_equals_the_restatement(num_queries):
    rng = np.random.default_rng(19)
    X = rng.standard_normal((900, 9)).astype(np.float32)
    X[300:400] = X[:100]  # tied rows
    Q = X[rng.integers(0, 900, num_queries)] + np.float32(0.125)
    f = glx.Features(X)
    ix = f.build_ivf(12, niter=3)
    index = exported(ix)
    for metric in METRICS:
        dist = knn_ref.scores(Q, X, metric)
        for nprobe in (1, 2, 11):
            for k in (1, 20, 1000):  # 1000: beyond the probed lists' rows, the tail is padded
                want = knn_ivf_ref.search(Q, X, index, k, metric, nprobe, dist=dist)
                dev = ivf_search(ix, Q, k, metric, nprobe)
                assert knn_ref.same(dev, want), (metric, nprobe, k)
                if k == 1000:
                    assert np.all(want[0][:, -1] == -1)
            assert knn_ref.same(ivf_search(ix, Q, 20, metric, nprobe, host=True),
                                knn_ivf_ref.search(Q, X, index, 20, metric, nprobe, dist=dist))


def test_query_block_borders():
    """129 queries in blocks of 64 (the knob only shrinks the block) and, without the knob, the border the workspace
    budget draws: 299 probe slots of 1,024 keys leave room for 109 queries a block"""
    rng = np.random.default_rng(20)
    X = rng.standard_normal((1500, 5)).astype(np.float32)
    Q = rng.standard_normal((129, 5)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(300, niter=1)
    index = exported(ix)
    for metric in METRICS:
        dist = knn_ref.scores(Q, X, metric)
        want = knn_ivf_ref.search(Q, X, index, 7, metric, 3, dist=dist)
        with Tuned(knn_query_block=64):
            assert knn_ref.same(ivf_search(ix, Q, 7, metric, 3), want)
            assert knn_ref.same(ivf_search(ix, Q, 7, metric, 300), gpu_search(f, Q, 7, metric))
        assert knn_ref.same(ivf_search(ix, Q, 7, metric, 3), want)
    assert (256 << 20) // 8 // (299 * 1024) == 109
    want = knn_ivf_ref.search(Q, X, index, 1024, knn_ref.IP, 299)
    assert knn_ref.same(ivf_search(ix, Q, 1024, knn_ref.IP, 299), want)


def test_probe_slots_of_one_query_take_two_passes():
    """40,000 lists of one row each, all probed with k = 513: a query's 40,000 slot lists of KP = 1,024 keys exceed the
    workspace budget alone, so the block is one query and its slots go in passes of P = 32,768 and 7,232 that fold into
    the same running list.  (The IVF-PQ search takes its plan from the same function, knn_slot_plan:
    tests/test_gpu_knn_ivfpq.py has this shape too.)"""
    N, k, KP = 40000, 513, 1024
    budget_keys = (256 << 20) // 8
    assert budget_keys // (N * KP) == 0  # not even one query's slots fit ...
    P = budget_keys // KP
    assert P == 32768 and [min(P, N - p0) for p0 in range(0, N, P)] == [32768, 7232]  # ... so they go in two passes
    rng = np.random.default_rng(22)
    X = rng.standard_normal((N, 2)).astype(np.float32)
    Q = rng.standard_normal((2, 2)).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(N, niter=0, centroids=X)
    for metric in METRICS:
        assert knn_ref.same(ivf_search(ix, Q, k, metric, N), gpu_search(f, Q, k, metric)), metric


@pytest.mark.parametrize("metric", METRICS)
def test_found_sets_are_nested_in_nprobe(metric):
    rng = np.random.default_rng(21)
    centres = 3 * rng.standard_normal((16, 8))
    X = (centres[rng.integers(0, 16, 2000)] + rng.standard_normal((2000, 8))).astype(np.float32)
    Q = (centres[rng.integers(0, 16, 40)] + rng.standard_normal((40, 8))).astype(np.float32)
    f = glx.Features(X)
    ix = f.build_ivf(16, niter=5)
    k = 20
    true_ids = gpu_search(f, Q, k, metric)[0]
    before = [set()] * Q.shape[0]
    recall = []
    for nprobe in (1, 2, 4, 8, 16):
        now = knn_ivf_ref.found(ivf_search(ix, Q, k, metric, nprobe)[0], true_ids)
        assert all(b <= n for b, n in zip(before, now)), nprobe
        recall.append(sum(len(n) for n in now) / (k * len(now)))
        before = now
    assert recall[-1] == 1.0 and recall == sorted(recall)


# ---- errors and call forms --------------------------------------------------------------------------------------
def test_errors_and_call_forms():
    import torch
    rng = np.random.default_rng(22)
    X = rng.standard_normal((200, 4)).astype(np.float32)
    Q = rng.standard_normal((3, 4)).astype(np.float32)
    f = glx.Features(X)
    L = glx.lib()
    h = ctypes.c_void_p()
    assert L.glx_knn_ivf_build(f._h, 201, 0, 0, None, 0, None, ctypes.byref(h)) == INVALID  # nlist > N
    assert b"nlist" in L.glx_last_error() and not h.value
    with pytest.raises(glx.GlxError):
        f.build_ivf(0)
    ix = f.build_ivf(8, niter=2)
    with pytest.raises(glx.GlxError) as e:
        ix.search(Q, 5, nprobe=9)  # nprobe > nlist
    assert e.value.code == INVALID and "nprobe" in str(e.value)
    for bad in (0, -1):
        with pytest.raises(glx.GlxError):
            ix.search(Q, 5, nprobe=bad)
    for k in (0, 1025):
        with pytest.raises(glx.GlxError):
            ix.search(Q, k, out=(np.zeros((3, k), np.int64), np.zeros((3, k), np.float32)))
    with pytest.raises(ValueError):
        ix.search(np.ones((2, 5), np.float32), 1)
    with pytest.raises(ValueError):
        ix.search(Q, 1, metric="cosine")
    # out= validation: shape and type of both buffers
    good = (np.zeros((3, 5), np.int64), np.zeros((3, 5), np.float32))
    for out in ((np.zeros((3, 4), np.int64), good[1]), (good[0], np.zeros((2, 5), np.float32)),
                (np.zeros((3, 5), np.int32), good[1]), (good[0], np.zeros((3, 5), np.float64))):
        with pytest.raises(ValueError):
            ix.search(Q, 5, nprobe=2, out=out)
    got = ix.search(Q, 5, "l2", nprobe=2, out=good)
    assert got[0] is good[0] and got[1] is good[1]
    index = exported(ix)
    assert knn_ref.same(good, knn_ivf_ref.search(Q, X, index, 5, knn_ref.L2, 2))
    # the default buffers: numpy in, numpy out; torch in, torch out on the current (side) stream
    ids, dist = ix.search(Q, 5, nprobe=2)
    want = knn_ivf_ref.search(Q, X, index, 5, knn_ref.IP, 2)
    assert isinstance(ids, np.ndarray) and knn_ref.same((ids, dist), want)
    dQ = _cuda(Q)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ids, dist = ix.search(dQ, 5, nprobe=2)
    side.synchronize()
    assert ids.is_cuda and knn_ref.same((ids.cpu().numpy(), dist.cpu().numpy()), want)
    assert L.glx_knn_ivf_search(ix._h, 1, None, 0, 5, 2, None, None, 0, None) == 0  # no queries: a no-op success
    # a capture is refused before anything is queued
    out = (_cuda(np.full((3, 5), -7, np.int64)), _cuda(np.full((3, 5), NAN, np.float32)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(glx.GlxError) as e:
            ix.search(dQ, 5, nprobe=2, out=out)
    assert e.value.code == INVALID and "capture" in str(e.value)
    torch.cuda.synchronize()
    assert np.all(out[0].cpu().numpy() == -7)
    # destroy, then a fresh index answers info and searches
    ix.close()
    ix.close()
    assert ix._h is None
    fresh = f.build_ivf(5, niter=1)
    assert fresh.info()["nlist"] == 5 and fresh.info()["num_rows"] == 200
    assert knn_ref.same(ivf_search(fresh, Q, 5, knn_ref.IP, 5), gpu_search(f, Q, 5, knn_ref.IP))
    # the index keeps its table alive
    keep = glx.Features(X).build_ivf(4, niter=1)
    import gc
    gc.collect()
    assert knn_ref.same(ivf_search(keep, Q, 5, knn_ref.L2, 4), knn_ref.search(Q, X, 5, knn_ref.L2))
