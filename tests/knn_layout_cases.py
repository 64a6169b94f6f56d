"""The cases of the KNN layout tests (tests/test_knn_swizzle_cpu.py, tests/test_gpu_knn_swizzle.py): tables on which the
row swizzle of an owned table MOVES rows, a float64 statement of the search contract on them, and the tables a kernel
that got the layout wrong would effectively search.  Block 0 of the swizzle is the identity, so the smallest owned table
with a row that is not stored at its own number has two whole blocks of 4,096 rows.
numpy only; fixed seeds; the arrays are cached and read-only: nothing here is drawn or changed at test time."""
import functools

import numpy as np

import knn_ref

SWIZZLE_BITS = 12  # GLX_SWIZZLE_BITS
SWIZZLE_MUL = 0x9E3779B1  # the multiplier of glx_swizzle_row
BLOCK = 1 << SWIZZLE_BITS
N = 2 * BLOCK + 300  # block 0 stays, every row of block 1 moves, a tail of 300 rows is not swizzled
N3 = 3 * BLOCK + 5  # blocks 1 and 2 move under different masks
DIMS = (17, 32)  # a float32 pitch that is not 16-byte aligned with a tail group; aligned rows and two 16-column steps
KS = (20, 300)
NLIST = 8
CENTROID_COL0 = (-3, -2, -1, 0, 1, 2, 3, 3)  # column 0 of the planted centroids: the last one repeats, its list is empty


def swizzle_bound(num_rows):
    return (num_rows >> SWIZZLE_BITS) << SWIZZLE_BITS


def swizzle(rows, num_rows):
    """glx_swizzle_row of an owned table of num_rows rows: the storage slot of every row of `rows`"""
    rows = np.asarray(rows, np.int64)
    mask = ((((rows >> SWIZZLE_BITS) * SWIZZLE_MUL) & 0xFFFFFFFF) >> (32 - SWIZZLE_BITS)).astype(np.int64)
    return np.where(rows < swizzle_bound(num_rows), rows ^ mask, rows)


def moved(rows, num_rows):
    """which of `rows` the swizzle stores at another slot: every row of the blocks from 1 on, below the bound"""
    rows = np.asarray(rows, np.int64)
    return (rows >= BLOCK) & (rows < swizzle_bound(num_rows))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def integer_case(dim, seed=0, num_rows=N):
    """(X[num_rows, dim], Q[130, dim]) of integers in [-3, 3]: exact in float32, bfloat16, float16, e4m3 and e5m2 and
    in every accumulator, so float64 gives the contract's bits and ties.  Planted:
      X[4096:4104] and X[8192] all hold one row of +-3: ties inside block 1 whose slots DESCEND while their rows ascend
        (the mask of block 1 ends in binary 011), and a tie with the first row behind block 1; query 0 is that row, so
        under both metrics these nine rows are its best, in row order;
      X[100:300] = X[4196:4396]: ties between block 0 and block 1;
      queries 1 .. 69 are copies of moved rows, ten of them of rows of [4196, 4396);
      column 0 is drawn so that centroids() makes eight lists of very different lengths, one of them empty."""
    assert dim >= 2 and num_rows >= 2 * BLOCK + 1
    rng = np.random.default_rng(1000 * dim + seed)
    X = rng.integers(-3, 4, (num_rows, dim)).astype(np.float32)
    sizes = [90, 140, 700, num_rows - 4930, 2000, 1500, 500, 0]
    X[:, 0] = rng.permutation(np.repeat(np.array(CENTROID_COL0, np.float32), sizes))
    X[100:300] = X[4196:4396]
    X[4096:4104] = rng.choice(np.array([-3, 3], np.float32), dim)
    X[2 * BLOCK] = X[4096]
    Q = rng.integers(-3, 4, (130, dim)).astype(np.float32)
    Q[0] = X[4096]
    rows = rng.choice(np.arange(BLOCK, swizzle_bound(num_rows)), 69, replace=False)
    rows[:10] = 4196 + 19 * np.arange(10)
    Q[1:70] = X[rows]
    return _frozen(X, Q)


def centroids(dim):
    """the planted centroids: zero but for column 0, so that column 0 of a row of integer_case names its list"""
    C = np.zeros((NLIST, dim), np.float32)
    C[:, 0] = CENTROID_COL0
    return C


@functools.lru_cache(maxsize=None)
def gaussian_case(dim, seed=0):
    """(X[N, dim], Q[200, dim]) standard normal, with the special values of the other KNN tests inside block 1: one
    +inf (in the last column), one NaN, one row of -0.0; one NaN in one query"""
    rng = np.random.default_rng(2000 * dim + seed)
    X = rng.standard_normal((N, dim)).astype(np.float32)
    X[BLOCK + 100, dim - 1], X[BLOCK + 700, 5], X[BLOCK + 900] = np.inf, np.nan, -0.0
    Q = rng.standard_normal((200, dim)).astype(np.float32)
    Q[17, 3] = np.nan
    return _frozen(X, Q)


def hashed_ids(num_rows):
    """scattered node ids (a hash id map), some of them negative"""
    return np.random.default_rng(5).permutation(10 ** 6)[:num_rows].astype(np.int64) - 1000


def wrong_tables(X):
    """What a kernel that got the layout wrong would effectively search, as (name, rows, norms_of) triples: row r scores
    against rows[r], and under L2 takes its norm from norms_of[r].
      "unswizzled read": the rows are fetched at their own number, where another row is stored;
      "norms by slot"  : the right rows, xn[] indexed by the slot (L2 only: the inner product has no norms)."""
    S = np.ascontiguousarray(X[swizzle(np.arange(X.shape[0]), X.shape[0])])
    return [("unswizzled read", S, S), ("norms by slot", X, S)]


def scores64(Q, X, metric, norms_of=None):
    """dist[nq, n] float32 from float64 arithmetic: the inner product, or the contract's L2 expression
    max(qn + xn - 2 ip, 0) with xn from norms_of (default: X itself).  Exact on integer_case."""
    Q64, X64 = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    ip = Q64 @ X64.T
    if metric == knn_ref.IP:
        return ip.astype(np.float32)
    xn = (np.asarray(X if norms_of is None else norms_of, np.float64) ** 2).sum(1)
    return np.maximum((Q64 * Q64).sum(1)[:, None] + xn[None, :] - 2 * ip, 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ranked(dim, metric, num_rows):
    X, Q = integer_case(dim, num_rows=num_rows)
    dist = scores64(Q, X, metric)
    return _frozen(dist, knn_ref.order(dist, metric))


def want(dim, metric, k, num_rows=N, ids=None):
    """the contract's (ids, dist) of integer_case(dim, num_rows=num_rows): float64 scores, ties to the smaller LOGICAL
    row; ids: the table's id map"""
    dist, perm = _ranked(dim, metric, num_rows)
    return knn_ref.take_k(dist, k, metric, ids=ids, perm=perm)
