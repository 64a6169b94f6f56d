"""Restatement of the IVF-Flat index contract (include/glx.h, "IVF-Flat index") in numpy on top of tests/knn_ref.py: the
deterministic build (sample, initial centroids, L2 k = 1 assignment, sequential float32 mean, stable lists) and the
probed search (probe lists from knn_ref.search over the centroids, knn_ref.take_k over the union of their rows).
X is the table in storage-row order, a half table as its exact float32 upcast."""
import numpy as np

import knn_ref


def sample_rows(N, T):
    """the storage row of every element of a T-element sample of N rows"""
    return (np.arange(T, dtype=np.int64) * N) // T


def train_size(N, nlist, train_rows=None):
    T = min(N, 256 * nlist) if not train_rows else int(train_rows)
    return min(max(T, nlist), N)


def assign(R, C):
    """the first centroid of every row of R under the search contract with L2 and k = 1"""
    return knn_ref.search(R, C, 1, knn_ref.L2)[0][:, 0]


def mean_rows(R):
    """(+0.0f + R[0] + R[1] + ...) / n, each step rounded to float32, in the order given"""
    acc = np.cumsum(np.concatenate([np.zeros((1, R.shape[1]), np.float32), R]), axis=0, dtype=np.float32)[-1]
    return acc / np.float32(R.shape[0])


def build(X, nlist, niter=10, train_rows=None, centroids=None):
    """-> dict(centroids[nlist, dim] float32, list_ptr[nlist + 1] int64, list_rows[N] int64)"""
    X = np.ascontiguousarray(X, np.float32)
    N = X.shape[0]
    assert 1 <= nlist <= N
    T = train_size(N, nlist, train_rows)
    S = X[sample_rows(N, T)]
    if centroids is not None:
        C = np.array(centroids, np.float32)
        assert C.shape == (nlist, X.shape[1])
    else:
        C = S[(np.arange(nlist, dtype=np.int64) * T) // nlist].copy()
    with np.errstate(all="ignore"):
        for _ in range(niter):
            a = assign(S, C)
            for l in np.unique(a):
                C[l] = mean_rows(S[a == l])  # boolean selection keeps ascending sample order = ascending storage row
    a = assign(X, C)
    list_ptr = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    return {"centroids": C, "list_ptr": list_ptr, "list_rows": np.argsort(a, kind="stable").astype(np.int64)}


def probes(Q, index, metric, nprobe):
    """the probed lists of every query [nq, nprobe], in the contract's order"""
    nlist = index["list_ptr"].shape[0] - 1
    assert 1 <= nprobe <= nlist
    if nprobe == nlist:
        return np.tile(np.arange(nlist, dtype=np.int64), (Q.shape[0], 1))
    return knn_ref.search(Q, index["centroids"], nprobe, metric)[0]


def search(Q, X, index, k, metric, nprobe, ids=None, dist=None):
    """(ids[nq, k], dist[nq, k]): the k best rows among the rows of the probed lists.  dist: knn_ref.scores(Q, X, metric)
    when the caller has it already."""
    Q = np.ascontiguousarray(Q, np.float32)
    dist = knn_ref.scores(Q, X, metric) if dist is None else dist
    ptr, rows = index["list_ptr"], index["list_rows"]
    oi = np.empty((Q.shape[0], k), np.int64)
    od = np.empty((Q.shape[0], k), np.float32)
    for q, lists in enumerate(probes(Q, index, metric, nprobe)):
        cand = np.sort(np.concatenate([rows[ptr[l]:ptr[l + 1]] for l in lists] + [np.zeros(0, np.int64)]))
        out_ids = cand if ids is None else np.asarray(ids, np.int64)[cand]
        oi[q], od[q] = (v[0] for v in knn_ref.take_k(dist[q:q + 1, cand], k, metric, ids=out_ids))
    return oi, od


def found(got_ids, true_ids):
    """per query, the set of true top-k ids a search returned"""
    return [set(g.tolist()) & set(t.tolist()) - {-1} for g, t in zip(got_ids, true_ids)]
