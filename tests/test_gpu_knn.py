"""glx_knn_search / glx_knn_merge on the GPU against the restatement of the contract (tests/knn_ref.py): ids exactly and
dist bit for bit (the sign of zero included; a NaN matches a NaN), unless a test says otherwise."""
import numpy as np
import pytest

import glx
import knn_ref

pytestmark = pytest.mark.gpu

METRIC_NAMES = {knn_ref.L2: "l2", knn_ref.IP: "ip"}
METRICS = [knn_ref.L2, knn_ref.IP]
NAN = np.float32(np.nan)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_search(f, Q, k, metric, host=False):
    """(ids, dist) as numpy; the output buffers start as canaries, so an unwritten element shows"""
    n = Q.shape[0]
    if host:
        out = (np.full((n, k), -7, np.int64), np.full((n, k), NAN, np.float32))
        f.search(np.ascontiguousarray(Q), k, METRIC_NAMES[metric], out=out)
        return out
    out = (_cuda(np.full((n, k), -7, np.int64)), _cuda(np.full((n, k), NAN, np.float32)))
    f.search(Q if glx._is_torch(Q) else _cuda(Q), k, METRIC_NAMES[metric], out=out)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


class Tuned:
    """glx.tune knobs for the duration of a block"""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for name, v in self.knobs.items():
            glx.tune(name, v)

    def __exit__(self, *exc):
        for name in self.knobs:
            glx.tune(name, -1)


def _data(rng, n, dim):
    """small dims draw from a handful of values (ties everywhere), larger ones from a normal distribution"""
    if dim <= 3:
        return (rng.integers(-4, 5, (n, dim)) / 4).astype(np.float32)
    return rng.standard_normal((n, dim)).astype(np.float32)


NQS, KS = [1, 63, 64, 65, 200], [1, 2, 20, 1024]


@pytest.mark.parametrize("num_rows", [1, 127, 128, 129, 1000])
@pytest.mark.parametrize("dim", [1, 2, 3, 31, 32, 33, 130])
def test_shape_grid(dim, num_rows):
    """tile and column remainders, one row, one query, k beyond the table; both metrics on every combination"""
    rng = np.random.default_rng(1000 * dim + num_rows)
    X, Q = _data(rng, num_rows, dim), _data(rng, max(NQS), dim)
    f = glx.Features(X)
    dQ = _cuda(Q)
    for metric in METRICS:
        dist = knn_ref.scores(Q, X, metric)
        perm = knn_ref.order(dist, metric)
        for nq in NQS:
            for k in KS:
                want = knn_ref.take_k(dist[:nq], k, metric, perm=perm[:nq])
                got = gpu_search(f, dQ[:nq], k, metric)
                assert knn_ref.same(got, want), (dim, num_rows, nq, k, metric)


@pytest.mark.parametrize("arrival", ["best_last", "best_first", "random"])
@pytest.mark.parametrize("metric", METRICS)
def test_many_chunks(metric, arrival):
    """128-row chunks over 1,000 rows; best-last makes every row of every chunk beat the threshold.  Also two query
    blocks (knn_query_block) and a k beyond one chunk."""
    rng = np.random.default_rng(7)
    X, Q = _data(rng, 1000, 33), _data(rng, 200, 33)
    Q[1:] = Q[0] + 0.01 * Q[1:]  # every query ranks the rows nearly alike
    by_q0 = knn_ref.order(knn_ref.scores(Q[:1], X, metric), metric)[0]
    if arrival == "best_last":
        X = X[by_q0[::-1]]
    elif arrival == "best_first":
        X = X[by_q0]
    X = np.ascontiguousarray(X)
    f = glx.Features(X)
    dist = knn_ref.scores(Q, X, metric)
    perm = knn_ref.order(dist, metric)
    with Tuned(knn_chunk_rows=128, knn_query_block=128):
        for k in (1, 20, 300):
            assert knn_ref.same(gpu_search(f, Q, k, metric), knn_ref.take_k(dist, k, metric, perm=perm)), k
    assert knn_ref.same(gpu_search(f, Q, 20, metric), knn_ref.take_k(dist, 20, metric, perm=perm))


def _ties_ascend(ids, dist):
    same = knn_ref.bits(dist[:, 1:] + np.float32(0)) == knn_ref.bits(dist[:, :-1] + np.float32(0))  # + 0: -0 == +0
    return np.all(ids[:, 1:][same] > ids[:, :-1][same])


@pytest.mark.parametrize("metric", METRICS)
def test_ties(metric):
    rng = np.random.default_rng(3)
    base = rng.standard_normal((3, 5)).astype(np.float32)
    Q = np.concatenate([base, rng.standard_normal((4, 5)).astype(np.float32)])
    tables = {
        "300 copies of 3 rows": np.tile(base, (300, 1)),
        "all equal": np.tile(base[:1], (700, 1)),
        # scores of +0.0 and -0.0: products that underflow to either sign, and exact zeros
        "signed zeros": np.tile(np.array([[0, 0, 0, 0, 0], [-1e-30, -0.0, -0.0, -0.0, -0.0], [1e-30, 0, 0, 0, 0]], np.float32),
                                (50, 1)),  # (a -0.0f partial sum survives only -0.0f products)
    }
    for name, X in tables.items():
        q = np.full((2, 5), 1e-30, np.float32) if name == "signed zeros" else Q
        f = glx.Features(X)
        with Tuned(knn_chunk_rows=256):
            for k in (1, 7, 400):
                got = gpu_search(f, q, k, metric)
                assert knn_ref.same(got, knn_ref.search(q, X, k, metric)), (name, k)
                m = min(k, X.shape[0])
                assert _ties_ascend(got[0][:, :m], got[1][:, :m]), (name, k)
    if metric == knn_ref.IP:
        assert np.signbit(got[1][0, :3]).tolist() == [False, True, False]  # the zeros keep their signs


@pytest.mark.parametrize("metric", METRICS)
def test_special_values(metric):
    rng = np.random.default_rng(4)
    dim = 33
    X = rng.standard_normal((300, dim)).astype(np.float32)
    Q = rng.standard_normal((6, dim)).astype(np.float32)
    X[10, -1] = np.inf  # in the LAST column of an odd dim: the column the matrix cores do not run
    X[11, -1] = -np.inf
    X[12, 0] = np.inf
    Q[1, :] = 0  # 0 * inf
    X[20] = 0
    X[20, -1] = -1e-30  # with Q[2]: a chain that underflows to -0.0f in the last column
    X[21] = 0
    X[21, 4] = -1e-30  # ... and in a matrix-core column (-0.0f products behind it keep the sign)
    X[21, 5:] = -0.0
    Q[2] = 1e-30
    X[30:40] = np.nan
    X[45, 7] = np.nan
    Q[3, 2] = np.nan  # a NaN query: every score a NaN, rows in order
    Q[4] = 3e38  # overflows to inf (and inf - inf under L2)
    f = glx.Features(X)
    for k in (1, 10, 300):
        assert knn_ref.same(gpu_search(f, Q, k, metric), knn_ref.search(Q, X, k, metric)), k
    # a table in which only 5 scores are numbers: the NaNs are listed behind them, by row
    Y = np.full((300, dim), np.nan, np.float32)
    good = [7, 50, 123, 200, 299]
    Y[good] = X[good]
    ids, dist = gpu_search(glx.Features(Y), Q[:1], 10, metric)
    assert knn_ref.same((ids, dist), knn_ref.search(Q[:1], Y, 10, metric))
    assert sorted(ids[0, :5].tolist()) == good and ids[0, 5:].tolist() == [0, 1, 2, 3, 4]
    assert not np.isnan(dist[0, :5]).any() and np.isnan(dist[0, 5:]).all()


def test_k_at_the_limits():
    X = np.arange(12, dtype=np.float32).reshape(4, 3)
    Q = np.ones((2, 3), np.float32)
    f = glx.Features(X)
    for metric in METRICS:
        ids, dist = gpu_search(f, Q, 1024, metric)
        assert knn_ref.same((ids, dist), knn_ref.search(Q, X, 1024, metric))
        assert np.all(ids[:, 4:] == -1) and np.all(dist[:, 4:] == knn_ref.pad_dist(metric))
    L = glx.lib()
    ids, dist = np.zeros((2, 1025), np.int64), np.zeros((2, 1025), np.float32)
    args = (Q.ctypes.data, 2)
    outs = (ids.ctypes.data, dist.ctypes.data, 0, None)
    assert L.glx_knn_search(f._h, 1, *args, 1025, *outs) == 3 and b"k must be" in L.glx_last_error()
    assert L.glx_knn_search(f._h, 1, *args, 0, *outs) == 3
    assert L.glx_knn_search(None, 1, *args, 1, *outs) == 3 and b"NULL" in L.glx_last_error()
    assert L.glx_knn_search(f._h, 2, *args, 1, *outs) == 3 and b"metric" in L.glx_last_error()
    assert L.glx_knn_search(f._h, 1, *args, 1, ids.ctypes.data, dist.ctypes.data, 7, None) == 3
    assert L.glx_knn_search(f._h, 1, Q.ctypes.data, -1, 1, *outs) == 3
    assert L.glx_knn_search(f._h, 1, None, 0, 1, None, None, 0, None) == 0  # no queries: a no-op success
    with pytest.raises(ValueError):
        f.search(np.ones((2, 4), np.float32), 1)
    with pytest.raises(ValueError):
        f.search(Q, 1, metric="cosine")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_half_tables_give_the_bits_of_the_upcast_table(dtype):
    import torch
    rng = np.random.default_rng(5)
    X = rng.standard_normal((700, 35)).astype(np.float32)
    Q = rng.standard_normal((70, 35)).astype(np.float32)
    up = torch.from_numpy(X).to(getattr(torch, dtype)).to(torch.float32).numpy()
    f = glx.Features(X, dtype=dtype)
    with Tuned(knn_chunk_rows=256):
        for metric in METRICS:
            assert knn_ref.same(gpu_search(f, Q, 25, metric), knn_ref.search(Q, up, 25, metric)), metric


def test_table_layout():
    rng = np.random.default_rng(6)
    # an id-mapped table answers ids, not rows: a hash map (scattered ids) and an arithmetic one
    X = rng.standard_normal((500, 9)).astype(np.float32)
    Q = rng.standard_normal((40, 9)).astype(np.float32)
    for ids in (rng.permutation(10 ** 6)[:500].astype(np.int64) - 1000, 5 + 3 * np.arange(500, dtype=np.int64)):
        f = glx.Features(X, ids=ids)
        for metric in METRICS:
            assert knn_ref.same(gpu_search(f, Q, 600, metric), knn_ref.search(Q, X, 600, metric, ids=ids))
    # from 4,096 rows on an owned table is stored swizzled; a view reads the caller's rows in order
    X = rng.standard_normal((4096 + 500, 6)).astype(np.float32)
    X[4000:4200] = X[100:300]  # ties across the swizzle's blocks: the order is by LOGICAL row
    Q = X[rng.integers(0, X.shape[0], 30)] + np.float32(0.25)
    owned, dX = glx.Features(X), _cuda(X)
    view = glx.Features(dX, view=True)
    for metric in METRICS:
        want = knn_ref.search(Q, X, 50, metric)
        assert knn_ref.same(gpu_search(owned, Q, 50, metric), want)
        assert knn_ref.same(gpu_search(view, Q, 50, metric), want)


def test_call_forms():
    import torch
    rng = np.random.default_rng(8)
    X = rng.standard_normal((900, 40)).astype(np.float32)
    Q = rng.standard_normal((130, 40)).astype(np.float32)
    f = glx.Features(X)
    for metric in METRICS:
        want = knn_ref.search(Q, X, 33, metric)
        dev, dev2 = gpu_search(f, Q, 33, metric), gpu_search(f, Q, 33, metric)
        host = gpu_search(f, Q, 33, metric, host=True)
        assert knn_ref.same(dev, want) and knn_ref.same(host, want)
        assert np.array_equal(dev[1].view(np.uint32), dev2[1].view(np.uint32))
        assert np.array_equal(dev[1].view(np.uint32), host[1].view(np.uint32))
        dQ = _cuda(Q)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ids, dist = f.search(dQ, 33, METRIC_NAMES[metric])
        side.synchronize()
        assert knn_ref.same((ids.cpu().numpy(), dist.cpu().numpy()), want)
    # the default out= buffers
    ids, dist = f.search(Q, 5, "l2")
    assert isinstance(ids, np.ndarray) and knn_ref.same((ids, dist), knn_ref.search(Q, X, 5, knn_ref.L2))


def test_l2_norm_cache_belongs_to_its_table():
    rng = np.random.default_rng(9)
    XA = rng.standard_normal((600, 17)).astype(np.float32)
    XB = (3 * rng.standard_normal((250, 17))).astype(np.float32)
    Q = rng.standard_normal((20, 17)).astype(np.float32)
    fa, fb = glx.Features(XA), glx.Features(XB)
    assert knn_ref.same(gpu_search(fa, Q, 9, knn_ref.L2), knn_ref.search(Q, XA, 9, knn_ref.L2))
    assert knn_ref.same(gpu_search(fb, Q, 9, knn_ref.L2), knn_ref.search(Q, XB, 9, knn_ref.L2))
    assert knn_ref.same(gpu_search(fa, Q, 9, knn_ref.IP), knn_ref.search(Q, XA, 9, knn_ref.IP))
    assert knn_ref.same(gpu_search(fa, Q, 9, knn_ref.L2, host=True), knn_ref.search(Q, XA, 9, knn_ref.L2))
    assert knn_ref.same(gpu_search(fb, Q, 9, knn_ref.L2), knn_ref.search(Q, XB, 9, knn_ref.L2))


@pytest.mark.parametrize("metric", METRICS)
def test_merge_of_row_ranges_equals_the_whole_search(metric):
    rng = np.random.default_rng(10)
    X = rng.integers(-2, 3, (900, 3)).astype(np.float32)  # ties across the ranges
    X[100] = np.nan
    Q = rng.integers(-2, 3, (70, 3)).astype(np.float32)
    whole = glx.Features(X)
    cuts = [0, 250, 330, 900]
    for k in (1, 40, 300):  # 300: beyond two of the ranges, their lists arrive padded
        parts = [gpu_search(glx.Features(X[a:b], ids=np.arange(a, b, dtype=np.int64)), Q, k, metric)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        pi, pd = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        want = gpu_search(whole, Q, k, metric)
        assert knn_ref.same(want, knn_ref.search(Q, X, k, metric))
        assert knn_ref.same(knn_ref.merge(pi, pd, metric), want)
        assert knn_ref.same(glx.knn_merge(pi, pd, METRIC_NAMES[metric]), want), k
        got = glx.knn_merge(_cuda(pi), _cuda(pd), METRIC_NAMES[metric])
        assert knn_ref.same((got[0].cpu().numpy(), got[1].cpu().numpy()), want), k


@pytest.mark.parametrize("dim", [3, 130])
def test_dist_lies_inside_the_float64_bound(dim):
    rng = np.random.default_rng(11)
    X = rng.standard_normal((400, dim)).astype(np.float32)
    Q = rng.standard_normal((50, dim)).astype(np.float32)
    f = glx.Features(X)
    Q64, X64 = Q.astype(np.float64), X.astype(np.float64)
    ip64, mag = Q64 @ X64.T, np.abs(Q64) @ np.abs(X64).T
    qn, xn = (Q64 * Q64).sum(1)[:, None], (X64 * X64).sum(1)[None, :]
    ids, dist = gpu_search(f, Q, 400, knn_ref.IP)
    err = np.abs(dist.astype(np.float64) - np.take_along_axis(ip64, ids, 1))
    assert np.all(err <= (dim + 2) * 2.0 ** -24 * np.take_along_axis(mag, ids, 1))
    ids, dist = gpu_search(f, Q, 400, knn_ref.L2)
    want = np.take_along_axis(np.maximum(qn + xn - 2 * ip64, 0), ids, 1)
    bound = (dim + 4) * 2.0 ** -24 * np.take_along_axis(qn + xn + 2 * mag, ids, 1)
    assert np.all(np.abs(dist.astype(np.float64) - want) <= bound)
