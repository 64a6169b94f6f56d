"""CPU checks of the KNN contract's restatement (tests/knn_ref.py) itself: the chain against float64 within the derived
bound, ids against a float64 brute force on well-separated data, the tie / NaN order, the padding, and the merge.
Then a restatement of the host schedule of glx_knn.hip (its constants read from the source) and, with it, a check that
every case of tests/test_gpu_knn_paths.py lands on the path it is written for; and the reference-side conditions of
that file's subnormal cases, which hold or fail without a GPU."""
import os
import re

import numpy as np
import pytest

import glx
import knn_ref
import test_gpu_knn_paths as paths

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


# ---- the host schedule (the arithmetic at the top of knn_search_device), restated ---------------------------------
KNN_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graph-learn_amd", "csrc")
KNN_HIP = (os.path.join(KNN_CSRC, "glx_knn.h"), os.path.join(KNN_CSRC, "glx_knn.hip"))
CONST_NAMES = ("kBQ", "kBR", "kBK", "kSortN", "kSelThreads", "kDefaultChunkRows", "kMaxChunkRows",
               "kDefaultFirstChunkRows", "kCandBudgetBytes")


def read_constants(paths=KNN_HIP):
    """The constexpr integers of glx_knn.h and glx_knn.hip, by name; a retune that moves a case off its path fails
    here."""
    src = ""
    for path in paths:
        with open(path) as f:
            src += f.read()
    out = {}
    for name in CONST_NAMES:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, "glx_knn.hip no longer defines " + name
        expr = re.sub(r"\(\s*(?:size_t|u?int\d+_t|int)\s*\)", "", m.group(1)).strip()
        assert re.fullmatch(r"[0-9\s<()+*]+", expr), (name, expr)
        out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


CONSTS = read_constants()


def _up(x, m):
    return (x + m - 1) // m * m


def schedule(num_rows, num_queries, k, chunk_knob=-1, qblock_knob=-1):
    """-> (qb, first, chunk, KP): queries per block, rows of the first chunk, rows of every later chunk (= the
    candidate buffer's capacity per query), the running list's length."""
    c = CONSTS
    KP = 1
    while KP < k:
        KP <<= 1
    rows_up = _up(max(num_rows, 1), c["kBR"])
    budget_keys = c["kCandBudgetBytes"] // 8
    if chunk_knob > 0:
        chunk = _up(chunk_knob, c["kBR"])
        qb = budget_keys // chunk // c["kBQ"] * c["kBQ"]
    else:
        qb = min(_up(num_queries, c["kBQ"]), budget_keys // c["kDefaultChunkRows"])
        chunk = min(budget_keys // qb // c["kBR"] * c["kBR"], c["kMaxChunkRows"])
    chunk = min(chunk, rows_up)
    if qblock_knob > 0:
        qb = _up(qblock_knob, c["kBQ"])
    qb = min(max(qb, c["kBQ"]), _up(num_queries, c["kBQ"]))
    first = chunk if chunk_knob > 0 else min(chunk, c["kDefaultFirstChunkRows"])
    return qb, first, chunk, KP


def chunks_of(num_rows, first, chunk):
    """the row counts of the chunks the table is walked in"""
    out, row0 = [], 0
    while row0 < num_rows:
        row1 = min(row0 + (first if row0 == 0 else chunk), num_rows)
        out.append(row1 - row0)
        row0 = row1
    return out


def test_schedule_restates_the_cases_the_gpu_suite_already_runs():
    """shapes whose path the comments of tests/test_gpu_knn.py and DESIGN.md name"""
    c = CONSTS
    assert (c["kBQ"], c["kBR"], c["kSortN"], c["kSelThreads"]) == (128, 128, 1024, 512)
    assert schedule(1000, 200, 1024) == (256, 1024, 1024, 1024)  # test_shape_grid: one chunk, one batch
    assert schedule(1000, 200, 300, 128, 128) == (128, 128, 128, 512)  # test_many_chunks
    qb, first, chunk, KP = schedule(4596, 30, 50)  # test_table_layout
    assert (first, KP) == (2048, 64) and chunks_of(4596, first, chunk) == [2048, 2548]
    assert schedule(10 ** 7, 10, 10)[2] == c["kMaxChunkRows"]  # few queries: the chunk grows to its limit
    assert schedule(10 ** 7, 10 ** 5, 10)[::2] == (4096, 8192)  # many: the default block and chunk


def test_wide_cases_fold_a_full_width_list_over_several_chunks():
    w, N = paths.WIDE, CONSTS["kSortN"]
    assert any(k > N // 2 for k in w["ks"]) and any(k <= N // 2 for k in w["ks"]) and N in w["ks"]
    for knob in w["chunk_knobs"]:
        for k in w["ks"]:
            qb, first, chunk, KP = schedule(w["num_rows"], w["num_queries"], k, knob)
            sizes = chunks_of(w["num_rows"], first, chunk)
            assert len(sizes) >= 3 and qb >= w["num_queries"], (knob, k, sizes)
            assert max(sizes) <= N  # one sorted batch per chunk: this test is about folds, not batches
            assert (KP == N) == (k > N // 2)
            partly_empty = k > first + chunk  # ... when the third chunk merges in
            if KP == N or knob == min(w["chunk_knobs"]):
                assert partly_empty, (knob, k)
            assert sum(sizes[:-1]) > k  # ... and full before the last chunk: a full list is merged into as well
    assert len(chunks_of(w["num_rows"], *schedule(w["num_rows"], w["num_queries"], 1024, 128)[1:3])) == 11


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", paths.WIDE["dims"])
def test_best_last_rows_all_pass_the_threshold(dim, metric):
    """for query 0 no row is worse than a row before it, so each chunk's rows pass the threshold the chunks before
    left (equality passes)"""
    X, Q = paths.arranged(21, paths.WIDE["num_rows"], paths.WIDE["num_queries"], dim, metric, "best_last")
    d = knn_ref.scores(Q[:1], X, metric)[0]
    assert not np.isnan(d).any()
    assert np.all(d[1:] <= d[:-1]) if metric == knn_ref.L2 else np.all(d[1:] >= d[:-1])


def test_batch_cases_put_several_sorted_batches_into_one_chunk():
    b, N = paths.BATCHES, CONSTS["kSortN"]
    assert {1, 2, 3, N} <= set(b["ks"])
    qb, first, chunk, _ = schedule(b["num_rows"], b["num_queries"], 1, b["chunk_knobs"][0])
    sizes = chunks_of(b["num_rows"], first, chunk)
    assert b["chunk_knobs"][0] == -1 and first == CONSTS["kDefaultFirstChunkRows"]
    assert len(sizes) == 2 and sizes[0] == 2 * N and 0 < sizes[1] < N, sizes  # two full batches, then one
    qb, first, chunk, _ = schedule(b["num_rows"], b["num_queries"], 1, b["chunk_knobs"][1])
    sizes = chunks_of(b["num_rows"], first, chunk)
    assert sizes == [b["num_rows"]] and 2 * N < sizes[0] < 3 * N, sizes  # three batches, the last padded
    assert qb >= b["num_queries"]


def test_query_block_cases_reach_a_second_default_block():
    qc = paths.QBLOCKS
    default_qb = CONSTS["kCandBudgetBytes"] // 8 // CONSTS["kDefaultChunkRows"]
    assert default_qb == 4096  # the test slices its outputs at the block border
    for num_rows in qc["tables"]:
        qb, first, chunk, _ = schedule(num_rows, qc["num_queries"], max(qc["ks"]))
        assert qb == default_qb < qc["num_queries"] < 2 * qb
        assert qb * chunk * 8 <= 80 << 20  # the candidate workspace stays small
    assert len(chunks_of(qc["tables"][0], *schedule(qc["tables"][0], qc["num_queries"], 1)[1:3])) == 1
    qb, first, chunk, _ = schedule(qc["tables"][1], qc["num_queries"], 1)
    assert chunks_of(qc["tables"][1], first, chunk) == [CONSTS["kDefaultFirstChunkRows"], qc["tables"][1] - first]


def test_merge_cases_span_several_batches_with_absent_entries_anywhere():
    N = CONSTS["kSortN"]
    assert all(parts * k > N for parts, k in paths.MERGE_SHAPES)  # more than one sorted batch
    assert (16, N) in paths.MERGE_SHAPES and any(parts * k % N for parts, k in paths.MERGE_SHAPES)
    for parts, k in paths.MERGE_SHAPES:
        for metric in METRICS:
            ids, dist = paths.merge_inputs(parts, k, metric)
            absent = ids == -1
            assert absent[:, 1, :].all() and 0 < (~absent[:, 2, :]).sum() < k
            rest = absent[:, 3:, :]
            assert rest.any() and not rest.all()
            assert rest[:, :, 0].any() and rest[:, :, k // 2].any()  # ... not as tail padding
            assert {0x00000000, 0x80000000, 0x7f800000, 0xff800000} <= set(np.unique(knn_ref.bits(dist)).tolist())
            assert np.isnan(dist).any()


def test_merge_does_not_need_sorted_lists():
    """the contract orders the parts * k entries of a query whatever order they stand in: against a plain sort"""
    ids, dist = paths.merge_inputs(5, 300, knn_ref.IP, nq=4)
    for metric in METRICS:
        oi, od = knn_ref.merge(ids, dist, metric)
        for q in range(4):
            entries = [(bool(np.isnan(dist[p, q, j])), 0.0 if np.isnan(dist[p, q, j]) else
                        float(dist[p, q, j]) * (1 if metric == knn_ref.L2 else -1), p, j)
                       for p in range(5) for j in range(300) if ids[p, q, j] != -1]
            entries.sort()
            top = entries[:300]
            assert oi[q, :len(top)].tolist() == [int(ids[p, q, j]) for _, _, p, j in top]
            assert np.array_equal(knn_ref.bits(od[q, :len(top)]),
                                  knn_ref.bits(np.array([dist[p, q, j] for _, _, p, j in top], np.float32)))
            assert np.all(oi[q, len(top):] == -1)


def test_subnormal_cases_cover_matrix_core_and_valu_columns_and_hold_on_the_reference():
    s = paths.SUBNORMAL
    tiles = sorted(set(-(-d // CONSTS["kBK"]) for d in s["dims"]))
    assert tiles == [1, 2] and any(d % 2 for d in s["dims"]) and any(d % 2 == 0 for d in s["dims"])
    assert len(chunks_of(s["num_rows"], *schedule(s["num_rows"], s["num_queries"], 1, -1)[1:3])) == 1
    assert len(chunks_of(s["num_rows"], *schedule(s["num_rows"], s["num_queries"], 1, 128)[1:3])) == 3
    assert set(paths.SUBNORMAL_CASES) == {("a", knn_ref.IP), ("b", knn_ref.L2), ("b", knn_ref.IP)}
    for dim in s["dims"]:
        for case, metric in paths.SUBNORMAL_CASES:
            X, Q = paths.subnormal_inputs(case, dim)
            paths.check_subnormal_reference(case, X, knn_ref.scores(Q, X, metric))
    # under L2 case a collapses to qn (why it is IP only): a flushing host shows here as well
    X, Q = paths.subnormal_inputs("a", 3)
    assert len(np.unique(knn_ref.scores(Q[:1], X, knn_ref.L2))) == 1
    # what the check is for: scores flushed to zero do not pass it
    X, Q = paths.subnormal_inputs("b", 3)
    with pytest.raises(AssertionError):
        paths.check_subnormal_reference("b", X, np.zeros((20, 300), np.float32))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_half_subnormal_tables_upcast_exactly(dtype):
    stored, up = paths.half_subnormal_table(dtype)
    limit = paths.MIN_NORMAL if dtype == "bfloat16" else np.float32(2.0 ** -14)
    assert np.all(np.abs(up) < limit) and np.count_nonzero(up) > up.size // 2


def test_the_empty_table_pads_every_slot():
    for metric in METRICS:
        ids, dist = knn_ref.search(np.ones((3, 5), np.float32), np.zeros((0, 5), np.float32), 4, metric)
        assert np.all(ids == -1) and np.all(dist == knn_ref.pad_dist(metric))
    assert chunks_of(0, *schedule(0, 3, 1024)[1:3]) == []  # no score or select launch
