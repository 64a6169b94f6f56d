"""Conditions on the inputs of tests/test_gpu_knn_swizzle.py (tests/knn_layout_cases.py), checked without a GPU: the
swizzle moves rows on these tables, and a kernel that dropped it on the read, indexed the norms by slot, emitted the slot
as the id or broke ties by slot would return something else than the float64 answer the GPU tests compare with.  Without
these the GPU tests could pass on a table whose swizzle is the identity, as every KNN test on 4,096 + n rows does."""
import os
import re

import numpy as np
import pytest

import knn_ivf_ref
import knn_layout_cases as cases
import knn_ref
from test_gpu_knn_ivf_list import brute64

METRICS = [knn_ref.L2, knn_ref.IP]
COMMON_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graph-learn_amd", "csrc",
                        "glx_common.h")


def top(Q, X, k, metric, norms_of=None):
    return knn_ref.take_k(cases.scores64(Q, X, metric, norms_of), k, metric)


def differs(a, b):
    """per query: the two (ids, dist) answers are not the same"""
    return (a[0] != b[0]).any(1) | (a[1] != b[1]).any(1)


def test_the_restated_swizzle_is_the_headers():
    with open(COMMON_H) as f:
        src = f.read()
    assert int(re.search(r"#define\s+GLX_SWIZZLE_BITS\s+(\d+)", src).group(1)) == cases.SWIZZLE_BITS
    body = src[src.index("glx_swizzle_row(int64_t r"):][:400]
    assert "if (r >= swizzle_rows) return r;" in body and "r >> GLX_SWIZZLE_BITS" in body
    assert "hi * 0x%Xu) >> (32 - GLX_SWIZZLE_BITS)" % cases.SWIZZLE_MUL in body and "r ^ (int64_t)m" in body


@pytest.mark.parametrize("num_rows", [cases.N, cases.N3])
def test_the_swizzle_moves_every_row_of_the_blocks_behind_block_0(num_rows):
    rows = np.arange(num_rows)
    slot = cases.swizzle(rows, num_rows)
    assert np.array_equal(np.sort(slot), rows)  # a bijection on [0, num_rows)
    assert np.array_equal(cases.swizzle(slot, num_rows), rows)  # an involution
    at_home = slot == rows
    assert np.array_equal(~at_home, cases.moved(rows, num_rows))
    assert (~at_home).sum() == cases.swizzle_bound(num_rows) - cases.BLOCK
    assert np.array_equal(slot >> cases.SWIZZLE_BITS, rows >> cases.SWIZZLE_BITS)  # inside its block
    assert slot[4096] == 4096 + 0x9E3 and slot[4096:4104].tolist() == [4096 + 2528 + i for i in (3, 2, 1, 0, 7, 6, 5, 4)]
    if num_rows == cases.N3:
        assert slot[4096] - 4096 != slot[8192] - 8192  # two blocks, two masks


def test_on_4096_plus_500_rows_the_swizzle_moves_nothing():
    """why the cases of 4,096 + 300 and 4,096 + 500 rows in the other KNN tests never saw a moved row"""
    for n in (4096 + 300, 4096 + 500):
        assert np.array_equal(cases.swizzle(np.arange(n), n), np.arange(n))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", cases.DIMS)
def test_every_layout_mistake_changes_the_expected_answer(dim, metric):
    X, Q = cases.integer_case(dim)
    ids, dist = good = cases.want(dim, metric, 20)
    assert knn_ref.same(good, top(Q, X, 20, metric))
    reaches = cases.moved(ids, cases.N).any(1)  # the queries with a moved row among their 20 best
    assert reaches.sum() >= 60 and reaches[:70].all()
    for name, rows, norms_of in cases.wrong_tables(X):
        if name == "norms by slot" and metric == knn_ref.IP:
            continue
        bad = top(Q, rows, 20, metric, norms_of)
        assert differs(bad, good)[reaches].all(), name
    # the slot as the id
    assert (cases.swizzle(ids, cases.N) != ids).any(1)[reaches].all()
    # ties by slot: adjacent rows r1 < r2 of block 1 at one distance whose slots descend
    tied = (dist[:, 1:] == dist[:, :-1]) & cases.moved(ids[:, 1:], cases.N) & cases.moved(ids[:, :-1], cases.N)
    assert np.all(ids[:, 1:][tied] > ids[:, :-1][tied])
    descend = tied & (cases.swizzle(ids[:, 1:], cases.N) < cases.swizzle(ids[:, :-1], cases.N))
    assert descend[0].any() and descend.any(1).sum() >= 1
    assert ids[0, :9].tolist() == list(range(4096, 4104)) + [8192]
    # ... and across blocks 0 and 1: a row of [100, 300) right before its copy in [4196, 4396)
    pairs = (dist[:, 1:] == dist[:, :-1]) & (ids[:, :-1] < 300) & (ids[:, 1:] == ids[:, :-1] + 4096)
    assert pairs.any(1).sum() >= 5
    by_slot = np.lexsort((cases.swizzle(np.arange(cases.N), cases.N), dist_key(Q[:1], X, metric)[0]))[:20]
    assert not np.array_equal(by_slot, ids[0])


def dist_key(Q, X, metric):
    d = cases.scores64(Q, X, metric)
    return d if metric == knn_ref.L2 else -d


@pytest.mark.parametrize("dim", cases.DIMS)
def test_the_planted_lists_span_the_blocks(dim):
    """some list holds rows of block 0, of block 1 and of the tail; some list has more than 128 rows (a second row tile
    of the list-major scan) and some fewer; a list in slot order is not the list in row order; with one list probed,
    most queries still reach a moved row"""
    X, Q = cases.integer_case(dim)
    index = knn_ivf_ref.build(X, cases.NLIST, niter=0, centroids=cases.centroids(dim))
    ptr, rows = index["list_ptr"], index["list_rows"]
    sizes = np.diff(ptr)
    assert sizes[-1] == 0 and sizes[0] < 128 < sizes[1] < 256 < sizes.max()
    for l in range(cases.NLIST - 1):
        r = rows[ptr[l]:ptr[l + 1]]
        assert np.array_equal(X[r, 0], np.full(r.size, cases.CENTROID_COL0[l], np.float32))
        assert (r < 4096).any() and cases.moved(r, cases.N).any() and (r >= 8192).any(), l
        assert np.all(np.diff(r) > 0) and not np.all(np.diff(cases.swizzle(r, cases.N)) > 0), l
    for metric in METRICS:
        for nprobe in (1, 3):
            lists = knn_ivf_ref.probes(Q, index, metric, nprobe)
            ids = brute64(Q, X, index, lists, 20, metric)[0]
            assert cases.moved(ids, cases.N).any(1).sum() >= 60, (metric, nprobe)


@pytest.mark.parametrize("metric", METRICS)
def test_the_larger_table_reaches_block_2(metric):
    ids = cases.want(17, metric, 20, num_rows=cases.N3)[0]
    in_block_2 = (ids >= 2 * cases.BLOCK) & (ids < 3 * cases.BLOCK)
    assert in_block_2.any(1).sum() >= 60 and ((ids >= cases.BLOCK) & (ids < 2 * cases.BLOCK)).any(1).sum() >= 60
    assert np.all(cases.swizzle(ids[in_block_2], cases.N3) != ids[in_block_2])
