"""glx_knn_search / glx_knn_merge on the paths of the host schedule (knn_search_device) that tests/test_gpu_knn.py does
not reach: the select kernel at KP = kSortN over several folds, several sorted batches per chunk, the default query
blocks, the merge beyond one batch with absent entries anywhere, subnormal elements / products / distances through
the matrix-core and the VALU columns, half x swizzle x id map, the empty table, and L2 on a view whose rows change.

Every comparison is knn_ref.same: ids exactly, dist bit for bit, a NaN matches a NaN; outputs start as canaries.
The cases live in the module-level tables below; tests/test_knn_cpu.py imports them and checks, with a restatement of
the schedule that reads its constants from glx_knn.hip, that each case lands on the path it is written for."""
import numpy as np
import pytest

import glx
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, NAN, Tuned, _cuda, _data, gpu_search

pytestmark = pytest.mark.gpu

# ---- the cases (chunk knob -1 = the default schedule) --------------------------------------------------------------
WIDE = dict(num_rows=1300, num_queries=70, dims=(3, 33), chunk_knobs=(128, 256), ks=(257, 512, 513, 1000, 1024),
            arrivals=("best_last", "best_first", "random"))
BATCHES = dict(num_rows=3000, num_queries=40, dims=(3, 33), chunk_knobs=(-1, 4096), ks=(1, 2, 3, 100, 1024),
               arrivals=("best_last", "random"))
QBLOCKS = dict(num_queries=4096 + 104, dim=3, tables=(300, 2200), ks=(1, 20))
MERGE_NQ = 33
MERGE_SHAPES = [(5, 300), (16, 100), (2, 1024), (16, 1024)]  # (parts, k)
SUBNORMAL = dict(num_rows=300, num_queries=20, dims=(2, 3, 33, 64), ks=(1, 10, 300), chunk_knobs=(-1, 128))
SUBNORMAL_CASES = [("a", knn_ref.IP), ("b", knn_ref.L2), ("b", knn_ref.IP)]
MIN_NORMAL = np.float32(2.0 ** -126)


def arranged(seed, num_rows, num_queries, dim, metric, arrival):
    """(X, Q): every query a near-copy of query 0, the rows in the order in which query 0 ranks them (best last / best
    first) or as drawn.  Best last, every row of every chunk beats the threshold of the chunks before it."""
    rng = np.random.default_rng(seed)
    X, Q = _data(rng, num_rows, dim), _data(rng, num_queries, dim)
    Q[1:] = Q[0] + np.float32(0.01) * Q[1:]
    by_q0 = knn_ref.order(knn_ref.scores(Q[:1], X, metric), metric)[0]
    if arrival == "best_last":
        X = X[by_q0[::-1]]
    elif arrival == "best_first":
        X = X[by_q0]
    return np.ascontiguousarray(X), Q


def subnormal_inputs(case, dim, num_rows=SUBNORMAL["num_rows"], num_queries=SUBNORMAL["num_queries"]):
    """Small integers in [-8, 8] times a power of two (every value exact in float32).
    a: table 2^-140 (every non-zero element subnormal), queries 2^60: every product a normal number.
    b: table 2^-75, queries 2^-70: products, partial sums, norms and distances all in the subnormal range."""
    rng = np.random.default_rng(100 + dim)
    xs, qs = {"a": (2.0 ** -140, 2.0 ** 60), "b": (2.0 ** -75, 2.0 ** -70)}[case]
    X = rng.integers(-8, 9, (num_rows, dim)).astype(np.float32) * np.float32(xs)
    Q = rng.integers(-8, 9, (num_queries, dim)).astype(np.float32) * np.float32(qs)
    return X, Q


def check_subnormal_reference(case, X, dist):
    """What the REFERENCE must show before anything is compared with it: a host that flushed subnormals would
    otherwise agree with a flushing GPU on zeros."""
    mag = np.abs(dist)
    sub = (mag > 0) & (mag < MIN_NORMAL)
    if case == "a":
        nz = np.abs(X[X != 0])
        assert nz.size > 0 and np.all(nz < MIN_NORMAL)  # every non-zero table element is subnormal
        assert not sub.any()
        assert np.unique(dist[np.isfinite(dist) & (mag >= MIN_NORMAL)]).size >= 100
    else:
        assert sub.sum() >= 0.9 * dist.size, (int(sub.sum()), dist.size)


def merge_inputs(parts, k, metric, nq=MERGE_NQ):
    """[parts, nq, k] lists that no search wrote: unsorted, distances from a seven-value grid (ties across parts and
    positions, both zeros, NaN, both infinities), ids in [-1, 50) so that absent entries stand anywhere; query 1 has
    no present entry at all, query 2 fewer than k."""
    rng = np.random.default_rng(1000 * parts + k + metric)
    grid = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, -2.25], np.float32)
    dist = grid[rng.integers(0, grid.size, (parts, nq, k))]
    ids = rng.integers(-1, 50, (parts, nq, k)).astype(np.int64)
    ids[:, 1, :] = -1
    few = rng.random((parts, k)) < (k // 2) / (parts * k)  # about k / 2 present entries
    ids[:, 2, :] = np.where(few, ids[:, 2, :], -1)
    ids[0, 2, k - 1] = 7  # ... and at least one
    return ids, dist


# ---- 1. the select kernel's steady state --------------------------------------------------------------------------
@pytest.mark.parametrize("dim", WIDE["dims"])
@pytest.mark.parametrize("arrival", WIDE["arrivals"])
@pytest.mark.parametrize("metric", METRICS)
def test_wide_lists_over_many_chunks(metric, arrival, dim):
    """k up to kSortN folded over 11 (6) chunks of 128 (256) rows: the select kernel merges sorted batches into a
    partly filled and then a full list at KP = 512 and KP = kSortN, where every thread of knn_merge_batch holds two
    list slots."""
    X, Q = arranged(21, WIDE["num_rows"], WIDE["num_queries"], dim, metric, arrival)
    f = glx.Features(X)
    dQ = _cuda(Q)
    dist = knn_ref.scores(Q, X, metric)
    perm = knn_ref.order(dist, metric)
    for knob in WIDE["chunk_knobs"]:
        with Tuned(knn_chunk_rows=knob):
            for k in WIDE["ks"]:
                want = knn_ref.take_k(dist, k, metric, perm=perm)
                assert knn_ref.same(gpu_search(f, dQ, k, metric), want), (knob, k)


@pytest.mark.parametrize("dim", BATCHES["dims"])
@pytest.mark.parametrize("arrival", BATCHES["arrivals"])
@pytest.mark.parametrize("metric", METRICS)
def test_more_candidates_than_one_sorted_batch(metric, arrival, dim):
    """Default schedule: a first chunk of two full sorted batches, then 952 rows.  One 4,096-row chunk: 3,000
    candidates = three batches, the last padded with empty keys."""
    X, Q = arranged(22, BATCHES["num_rows"], BATCHES["num_queries"], dim, metric, arrival)
    f = glx.Features(X)
    dQ = _cuda(Q)
    dist = knn_ref.scores(Q, X, metric)
    perm = knn_ref.order(dist, metric)
    for knob in BATCHES["chunk_knobs"]:
        with Tuned(knn_chunk_rows=knob):
            for k in BATCHES["ks"]:
                want = knn_ref.take_k(dist, k, metric, perm=perm)
                assert knn_ref.same(gpu_search(f, dQ, k, metric), want), (knob, k)


# ---- 2. the default query blocks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_rows", QBLOCKS["tables"])
def test_more_queries_than_one_default_block(num_rows):
    """4,200 queries under the default knobs: a block of 4,096 and one of 104, the second reading its queries, norms
    and outputs at an offset."""
    nq, dim = QBLOCKS["num_queries"], QBLOCKS["dim"]
    rng = np.random.default_rng(23 + num_rows)
    X, Q = _data(rng, num_rows, dim), _data(rng, nq, dim)
    f = glx.Features(X)
    dQ = _cuda(Q)
    for metric in METRICS:
        dist = knn_ref.scores(Q, X, metric)
        perm = knn_ref.order(dist, metric)
        for k in QBLOCKS["ks"]:
            want = knn_ref.take_k(dist, k, metric, perm=perm)
            runs = [("device", gpu_search(f, dQ, k, metric))]
            if num_rows == min(QBLOCKS["tables"]):
                runs.append(("host", gpu_search(f, Q, k, metric, host=True)))
            for name, got in runs:
                second = tuple(a[4096:] for a in got), tuple(a[4096:] for a in want)
                assert knn_ref.same(*second), ("the second query block", name, metric, k)
                assert knn_ref.same(got, want), (name, metric, k)


# ---- 3. glx_knn_merge beyond one batch, absent entries anywhere ---------------------------------------------------
@pytest.mark.parametrize("parts,k", MERGE_SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_merge_of_many_long_lists(metric, parts, k):
    ids, dist = merge_inputs(parts, k, metric)
    want = knn_ref.merge(ids, dist, metric)
    assert np.all(want[0][1] == -1) and np.all(want[1][1] == knn_ref.pad_dist(metric))
    present = int((ids[:, 2, :] != -1).sum())
    assert 0 < present < k and np.all(want[0][2, present:] == -1) and np.all(want[0][2, :present] != -1)
    out = (np.full((MERGE_NQ, k), -7, np.int64), np.full((MERGE_NQ, k), NAN, np.float32))
    glx.knn_merge(ids, dist, METRIC_NAMES[metric], out=out)
    assert knn_ref.same(out, want), "host pointers"
    dout = (_cuda(np.full((MERGE_NQ, k), -7, np.int64)), _cuda(np.full((MERGE_NQ, k), NAN, np.float32)))
    glx.knn_merge(_cuda(ids), _cuda(dist), METRIC_NAMES[metric], out=dout)
    assert knn_ref.same((dout[0].cpu().numpy(), dout[1].cpu().numpy()), want), "device pointers"


# ---- 4. subnormals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", SUBNORMAL["dims"])
@pytest.mark.parametrize("case,metric", SUBNORMAL_CASES)
def test_subnormal_elements_products_and_distances(case, metric, dim):
    """The contract's chain keeps float32 subnormals: as B operands of the f32 MFMA (case a: a flushed operand makes
    every score zero), as its products and accumulators, in the VALU last column, in the norms and the L2 formula
    (case b).  A build that flushed denormals would change answers and ranks here."""
    X, Q = subnormal_inputs(case, dim)
    dist = knn_ref.scores(Q, X, metric)
    check_subnormal_reference(case, X, dist)
    perm = knn_ref.order(dist, metric)
    f = glx.Features(X)
    dQ = _cuda(Q)
    for knob in SUBNORMAL["chunk_knobs"]:
        with Tuned(knn_chunk_rows=knob):
            for k in SUBNORMAL["ks"]:
                want = knn_ref.take_k(dist, k, metric, perm=perm)
                assert knn_ref.same(gpu_search(f, dQ, k, metric), want), (knob, k)


def half_subnormal_table(dtype, num_rows=SUBNORMAL["num_rows"], dim=33):
    """(the table in its storage type, its exact float32 upcast): bfloat16 m * 2^-130 (bfloat16 has float32's exponent
    range: the upcast is a float32 subnormal too), float16 m * 2^-24 (float16 subnormals, float32 normals)."""
    import torch
    rng = np.random.default_rng(7)
    m = rng.integers(-8, 9, (num_rows, dim)).astype(np.float32)
    up = m * np.float32(2.0 ** -130 if dtype == "bfloat16" else 2.0 ** -24)
    stored = torch.from_numpy(up).to(getattr(torch, dtype))
    assert np.array_equal(stored.to(torch.float32).numpy().view(np.uint32), up.view(np.uint32))  # nothing rounded
    return stored, up


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_half_tables_of_subnormals_give_the_bits_of_the_upcast_table(dtype):
    stored, up = half_subnormal_table(dtype)
    nz = np.abs(up[up != 0])
    assert np.all(nz < (MIN_NORMAL if dtype == "bfloat16" else np.float32(2.0 ** -14)))  # subnormal in the storage type
    rng = np.random.default_rng(8)
    scale = np.float32(2.0 ** 60 if dtype == "bfloat16" else 1.0)
    Q = rng.integers(-8, 9, (SUBNORMAL["num_queries"], up.shape[1])).astype(np.float32) * scale
    ip = knn_ref.scores(Q, up, knn_ref.IP)
    assert np.unique(ip[ip != 0]).size >= 100 and np.all(np.abs(ip[ip != 0]) >= MIN_NORMAL)
    f = glx.Features(stored if dtype == "bfloat16" else stored.numpy())
    assert f.dtype == dtype
    for knob in SUBNORMAL["chunk_knobs"]:
        with Tuned(knn_chunk_rows=knob):
            for metric in METRICS:
                for k in (1, 10, 300):
                    assert knn_ref.same(gpu_search(f, Q, k, metric), knn_ref.search(Q, up, k, metric)), (knob, metric, k)


# ---- 5. layout combinations and the empty table ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_half_swizzled_id_mapped_tables(dtype):
    """half storage, the swizzle of an owned table of 4,096 rows and more, and an id map, all at once; L2 puts the
    norms kernel through swizzle and half storage together.  Ties across the swizzle's blocks go by LOGICAL row."""
    import torch
    rng = np.random.default_rng(31)
    n = 4096 + 300
    X = rng.standard_normal((n, 6)).astype(np.float32)
    X[4000:4200] = X[100:300]
    up = torch.from_numpy(X).to(getattr(torch, dtype)).to(torch.float32).numpy()
    Q = up[rng.integers(0, n, 30)] + np.float32(0.25)
    want = {metric: knn_ref.scores(Q, up, metric) for metric in METRICS}
    for ids in (rng.permutation(10 ** 6)[:n].astype(np.int64) - 1000, 5 + 3 * np.arange(n, dtype=np.int64)):
        f = glx.Features(X, ids=ids, dtype=dtype)
        for metric in METRICS:
            assert knn_ref.same(gpu_search(f, Q, 50, metric), knn_ref.take_k(want[metric], 50, metric, ids=ids)), metric


@pytest.mark.parametrize("metric", METRICS)
def test_a_table_of_no_rows(metric):
    f = glx.Features(np.zeros((0, 5), np.float32))
    assert f.num_rows == 0
    Q = np.random.default_rng(32).standard_normal((3, 5)).astype(np.float32)
    for k in (1, 1024):
        for host in (False, True):
            ids, dist = gpu_search(f, Q, k, metric, host=host)
            assert np.all(ids == -1) and np.all(dist == knn_ref.pad_dist(metric)), (k, host)  # and no canary is left
            assert knn_ref.same((ids, dist), knn_ref.search(Q, np.zeros((0, 5), np.float32), k, metric))


# ---- 6. L2 on a view follows the caller's matrix -----------------------------------------------------------------
def test_l2_search_on_a_view_follows_the_callers_matrix():
    """A view reads the caller's rows as they are NOW: norms of the rows an earlier search saw must not be reused.
    Before the norms of a view were built per search, the second L2 search below failed on
    `assert knn_ref.same(gpu_search(view, Q, 9, L2), knn_ref.search(Q, X2, 9, L2))` (stale xn: wrong distances)."""
    import torch
    rng = np.random.default_rng(41)
    X1 = rng.standard_normal((600, 17)).astype(np.float32)
    X2 = (3 * rng.standard_normal((600, 17))).astype(np.float32)
    Q = rng.standard_normal((20, 17)).astype(np.float32)
    dX, dQ = _cuda(X1), _cuda(Q)
    view = glx.Features(dX, view=True)
    L2, IP = knn_ref.L2, knn_ref.IP
    assert knn_ref.same(gpu_search(view, dQ, 9, L2), knn_ref.search(Q, X1, 9, L2))
    dX.copy_(_cuda(X2))
    torch.cuda.synchronize()
    assert knn_ref.same(gpu_search(view, dQ, 9, L2), knn_ref.search(Q, X2, 9, L2)), "L2 on the rewritten rows"
    assert knn_ref.same(gpu_search(view, dQ, 9, IP), knn_ref.search(Q, X2, 9, IP))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ids, dist = view.search(dQ, 9, "l2")
    side.synchronize()
    assert knn_ref.same((ids.cpu().numpy(), dist.cpu().numpy()), knn_ref.search(Q, X2, 9, L2)), "a side stream"
    # the real use: an embedding table under training
    rows = np.array([3, 599, 0, 250, 17], np.int64)
    grad = (5 * rng.standard_normal((rows.size, 17))).astype(np.float32)
    glx.embedding_update(glx.EMB_SGD, dX, _cuda(rows), _cuda(grad), alpha=0.5)
    torch.cuda.synchronize()
    X3 = dX.cpu().numpy()
    changed = np.flatnonzero((X3 != X2).any(1))
    assert changed.tolist() == sorted(rows.tolist())
    Q3 = np.concatenate([Q, X3[rows]])  # queries at the moved rows: their nearest row is themselves, at dist ~0
    got = gpu_search(view, Q3, 9, L2)
    assert knn_ref.same(got, knn_ref.search(Q3, X3, 9, L2)), "L2 after embedding_update"
    assert got[0][len(Q):, 0].tolist() == rows.tolist()
