"""Every KNN search path on owned tables whose row swizzle MOVES rows (tests/knn_layout_cases.py: 8,192 + 300 rows and
3 * 4,096 + 5; on 4,096 + n rows, as in the other KNN tests, the swizzle is the identity) and on a padded row pitch.
Ids, list entries, norms and tie order follow the LOGICAL row, whatever slot stores it.

No tolerance anywhere: a comparison is exact against float64 on integer data (a), (c), (d), or bit for bit between an
owned table and a view of the same stored values (b); a NaN matches a NaN, outputs start as canaries.
tests/test_knn_swizzle_cpu.py checks that the inputs make a layout mistake show.

Where a case asks for refine=64 and k = 300, refine is 300: the entry points take k <= refine only."""
import functools

import numpy as np
import pytest
import torch

import glx
import knn_ivf_ref
import knn_layout_cases as cases
import knn_ref
from test_gpu_knn import METRICS
from test_gpu_knn_half import run
from test_gpu_knn_ivf import check_lists, exported, same_index
from test_gpu_knn_ivf_half import run as ivf_run
from test_gpu_knn_ivf_list import brute64
from test_gpu_knn_ivfpq import check_searches, exported_pq, pq_search, same_pq

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16,
         "float8_e4m3fn": torch.float8_e4m3fn, "float8_e5m2": torch.float8_e5m2}
HALF_LIST = {"schedule": "list", "precision": "half"}


def flat_options(dtype, k):
    """the option sets of Features.search a table of this dtype takes"""
    refine = max(64, k)
    if dtype == "float32":
        return [{}, {"split": True}, {"tile": "narrow"}, {"split": True, "refine": refine}]
    return [{}, {"precision": "half"}, {"precision": "half", "tile": "narrow"}, {"precision": "half", "refine": refine}]


def integers(dim, num_rows=cases.N):
    """copies of the cached, read-only case: torch does not wrap a read-only array quietly"""
    return tuple(a.copy() for a in cases.integer_case(dim, num_rows=num_rows))


def owned(X, dtype, ids=None):
    return glx.Features(X, ids=ids, dtype=None if dtype == "float32" else dtype)


def mapped(want, ids):
    """the expected (rows, dist) through a table's id map; an absent slot stays -1"""
    if ids is None:
        return want
    return np.where(want[0] >= 0, ids[np.maximum(want[0], 0)], -1), want[1]


# ---- (a) exact, against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("id_map", [False, True])
@pytest.mark.parametrize("dim", cases.DIMS)
@pytest.mark.parametrize("dtype", sorted(TORCH))
def test_flat_searches_equal_float64(dtype, dim, id_map):
    X, Q = integers(dim)
    ids = cases.hashed_ids(cases.N) if id_map else None
    f = owned(X, dtype, ids)
    for metric in METRICS:
        for k in cases.KS:
            want = cases.want(dim, metric, k, ids=ids)
            for kw in flat_options(dtype, k):
                assert knn_ref.same(run(f, Q, k, metric, **kw), want), (metric, k, kw)


@functools.lru_cache(maxsize=None)
def planted_index(dim, num_rows=cases.N):
    X, _ = cases.integer_case(dim, num_rows=num_rows)
    return knn_ivf_ref.build(X, cases.NLIST, niter=0, centroids=cases.centroids(dim))


@functools.lru_cache(maxsize=None)
def ivf_want(dim, metric, nprobe, k, num_rows=cases.N):
    """float64 over the probed lists' rows, ties to the smaller logical row (brute64 of test_gpu_knn_ivf_list.py)"""
    X, Q = cases.integer_case(dim, num_rows=num_rows)
    index = planted_index(dim, num_rows)
    ids, dist = brute64(Q, X, index, knn_ivf_ref.probes(Q, index, metric, nprobe), k, metric)
    return ids, dist.astype(np.float32)


def build_planted(f, dim, num_rows=cases.N):
    """the index over the planted centroids; its lists are the restatement's: by LOGICAL row, each ascending"""
    ix = f.build_ivf(cases.NLIST, niter=0, centroids=cases.centroids(dim))
    got = exported(ix)
    assert same_index(got, planted_index(dim, num_rows))
    check_lists(got, num_rows)
    return ix


@pytest.mark.parametrize("id_map", [False, True])
@pytest.mark.parametrize("dim", cases.DIMS)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_ivf_flat_build_and_searches_equal_float64(dtype, dim, id_map):
    X, Q = integers(dim)
    ids = cases.hashed_ids(cases.N) if id_map else None
    ix = build_planted(owned(X, dtype, ids), dim)
    for metric in METRICS:
        for nprobe in (1, 3, 8):
            for k in cases.KS:
                want = mapped(ivf_want(dim, metric, nprobe, k), ids)
                for schedule in ("query", "list"):
                    got = ivf_run(ix, Q, k, metric, nprobe=nprobe, schedule=schedule)
                    assert knn_ref.same(got, want), (metric, nprobe, k, schedule)


@pytest.mark.parametrize("id_map", [False, True])
@pytest.mark.parametrize("dim", cases.DIMS)
@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float8_e4m3fn"])
def test_ivf_half_precision_scan_equals_float64(dtype, dim, id_map):
    X, Q = integers(dim)
    ids = cases.hashed_ids(cases.N) if id_map else None
    ix = build_planted(owned(X, dtype, ids), dim)
    for metric in METRICS:
        for nprobe in (3, 8):
            for k in cases.KS:
                want = mapped(ivf_want(dim, metric, nprobe, k), ids)
                for refine in (0, max(64, k)):
                    got = ivf_run(ix, Q, k, metric, nprobe=nprobe, refine=refine, **HALF_LIST)
                    assert knn_ref.same(got, want), (metric, nprobe, k, refine)


# ---- (b) bit for bit, an owned table against a view of the same stored values ----------------------------------------
LAYOUT_DTYPES = ["float32", "bfloat16", "float8_e5m2"]
both_layouts = pytest.mark.parametrize("dtype,dim", [(t, d) for t in LAYOUT_DTYPES for d in cases.DIMS])


def layouts(dtype, dim):
    """(owned table: swizzled; view: swizzle_rows == 0; the stored values as float32; queries) of gaussian_case(dim),
    rounded once by torch"""
    X, Q = (a.copy() for a in cases.gaussian_case(dim))
    stored = torch.from_numpy(X).to(TORCH[dtype])
    return glx.Features(stored), glx.Features(stored.cuda(), view=True), stored.float().numpy(), Q


@both_layouts
def test_flat_searches_of_an_owned_table_and_a_view_are_the_same_bits(dtype, dim):
    own, view, _, Q = layouts(dtype, dim)
    for metric in METRICS:
        for k in (1, 50):
            for kw in flat_options(dtype, k):
                got = run(own, Q, k, metric, **kw)
                assert cases.moved(got[0], cases.N).any(1).sum() >= 60  # rows that moved are among the answers
                assert knn_ref.same(got, run(view, Q, k, metric, **kw)), (metric, k, kw)


@both_layouts
def test_ivf_flat_of_an_owned_table_and_a_view_are_the_same_bits(dtype, dim):
    own, view, _, Q = layouts(dtype, dim)
    oix, vix = own.build_ivf(7, niter=2), view.build_ivf(7, niter=2)
    index = exported(oix)
    assert same_index(exported(vix), index)
    check_lists(index, cases.N)
    for metric in METRICS:
        for k in (1, 50):
            for nprobe in (1, 3, 7):
                for schedule in ("query", "list"):
                    kw = dict(nprobe=nprobe, schedule=schedule)
                    assert knn_ref.same(ivf_run(oix, Q, k, metric, **kw), ivf_run(vix, Q, k, metric, **kw)), (metric, k, kw)
            if dtype == "float32":
                continue
            for nprobe in (3, 7):
                for refine in (0, 64):
                    kw = dict(nprobe=nprobe, refine=refine, **HALF_LIST)
                    assert knn_ref.same(ivf_run(oix, Q, k, metric, **kw), ivf_run(vix, Q, k, metric, **kw)), (metric, k, kw)


@both_layouts
def test_ivf_pq_of_an_owned_table_and_a_view_are_the_same_bits(dtype, dim):
    """the codes follow logical rows; the searches equal the restatement over the index's own lists, codebooks and codes
    (13 queries, the NaN query among them: the restatement builds a table per query and list)"""
    own, view, V, Q = layouts(dtype, dim)
    Q = np.ascontiguousarray(Q[5:18])
    m = 4 if dim % 4 == 0 else 1
    oix, vix = own.build_ivf(7, niter=2), view.build_ivf(7, niter=2)
    opx, vpx = (ix.build_pq(m, niter=1, train_rows=700) for ix in (oix, vix))
    index, pq = exported(oix), exported_pq(opx)
    assert same_index(exported(vix), index) and same_pq(exported_pq(vpx), pq)
    pq_cases = [(1, 3, 0), (50, 3, 0), (50, 3, 200)]
    for metric in METRICS:
        for k, nprobe, refine in pq_cases:
            got = pq_search(opx, Q, k, metric, nprobe, refine)
            assert knn_ref.same(got, pq_search(vpx, Q, k, metric, nprobe, refine)), (metric, k, refine)
    check_searches(opx, V, Q, index, pq, pq_cases)
    check_searches(vpx, V, Q, index, pq, pq_cases)


# ---- (c) a padded row pitch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", cases.DIMS)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float8_e4m3fn"])
def test_padded_row_pitch(monkeypatch, dtype, dim):
    """GLX_FEATURE_ROW_PAD=4 (read at every table creation) adds 16 bytes to a row: a pitch of dim + 4, + 8, + 16
    elements, rows 16-byte aligned at dim 32 (the vector loads, with a pitch that is not dim) and not at dim 17 (the
    element loads).  One option set per kernel file, against the float64 answers of (a): the padded table answers
    exactly as the table without the pad, whose tests compare with the same arrays.  Setting the variable in this
    process reaches getenv (os.environ writes through putenv), as in the child of test_gpu_agg_arg.py's test of this
    name; a split scan made to step by dim instead of the pitch failed here, and only here, at both dims."""
    X, Q = integers(dim)
    monkeypatch.setenv("GLX_FEATURE_ROW_PAD", "4")
    f = owned(X, dtype)
    ix = build_planted(f, dim)
    monkeypatch.delenv("GLX_FEATURE_ROW_PAD")
    if dtype == "float32":
        flat = [{}, {"split": True}, {"tile": "narrow"}]
    else:
        flat = [{}, {"precision": "half"}, {"precision": "half", "tile": "narrow"}]
    probed = [{"schedule": "query"}, {"schedule": "list"}] + ([] if dtype == "float32" else [HALF_LIST])
    for metric in METRICS:
        for k in cases.KS:
            want = cases.want(dim, metric, k)
            for kw in flat:
                assert knn_ref.same(run(f, Q, k, metric, **kw), want), (metric, k, kw)
            for kw in probed:
                assert knn_ref.same(ivf_run(ix, Q, k, metric, nprobe=3, **kw), ivf_want(dim, metric, 3, k)), (metric, k, kw)


# ---- (d) one larger swizzle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_three_blocks_two_masks(dtype):
    """3 * 4,096 + 5 rows at dim 17: blocks 1 and 2 move under different masks, five rows stay behind them"""
    dim, n = 17, cases.N3
    X, Q = integers(dim, n)
    f = owned(X, dtype)
    ix = build_planted(f, dim, n)
    flat = [{}] + ([] if dtype == "float32" else [{"precision": "half"}])
    for metric in METRICS:
        for k in cases.KS:
            want = cases.want(dim, metric, k, num_rows=n)
            for kw in flat:
                assert knn_ref.same(run(f, Q, k, metric, **kw), want), (metric, k, kw)
            for nprobe in (3, 8):
                got = ivf_run(ix, Q, k, metric, nprobe=nprobe, schedule="list")
                assert knn_ref.same(got, ivf_want(dim, metric, nprobe, k, n)), (metric, k, nprobe)
