"""Restatement of the IVF-PQ index contract (include/glx.h, "IVF-PQ index") in numpy, composed from tests/knn_ref.py
(scores, search, take_k) and tests/knn_ivf_ref.py (build, probes, sample_rows): the deterministic codebooks (codebook j
IS knn_ivf_ref.build over the sample's residual sub-vectors j with 256 lists), the codes in list order, the ADC score (an
ascending float32 cumsum over look-up tables that are knn_ref.scores of sub-vectors) and the search with and without the
exact re-rank.  X is the table in storage-row order, a half table as its exact float32 upcast; `index` is a
knn_ivf_ref.build dict (or the exported lists of a device index)."""
import numpy as np

import knn_ivf_ref
import knn_ref

CODEWORDS = 256


def train_size(N, train_rows=None):
    T = min(N, 65536) if not train_rows else int(train_rows)
    return min(max(T, CODEWORDS), N)


def row_lists(index):
    """the list of every storage row"""
    ptr, rows = index["list_ptr"], index["list_rows"]
    out = np.empty(rows.shape[0], np.int64)
    out[rows] = np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr))
    return out


def residuals(X, index, rows):
    """x - centroid of x's list for the given storage rows: one float32 subtraction per column"""
    X = np.ascontiguousarray(X, np.float32)
    with np.errstate(all="ignore"):
        return X[rows] - np.asarray(index["centroids"], np.float32)[row_lists(index)[rows]]


def build(X, index, m, niter=10, train_rows=None, codebooks=None):
    """-> dict(codebooks[m, 256, dsub] float32, codes[N, m] uint8 in list order)"""
    X = np.ascontiguousarray(X, np.float32)
    N, dim = X.shape
    assert 1 <= m <= 64 and dim % m == 0 and N >= CODEWORDS
    dsub = dim // m
    T = train_size(N, train_rows)
    R = residuals(X, index, knn_ivf_ref.sample_rows(N, T))
    RL = residuals(X, index, index["list_rows"])
    books = np.empty((m, CODEWORDS, dsub), np.float32)
    codes = np.empty((N, m), np.uint8)
    if codebooks is not None:
        assert tuple(codebooks.shape) == books.shape
    for j in range(m):
        cols = slice(j * dsub, (j + 1) * dsub)
        start = None if codebooks is None else codebooks[j]
        books[j] = knn_ivf_ref.build(R[:, cols], CODEWORDS, niter, train_rows=T, centroids=start)["centroids"]
        codes[:, j] = knn_ivf_ref.assign(RL[:, cols], books[j])
    return {"codebooks": books, "codes": codes}


def adc(q, index, pq, metric, lists):
    """(rows, adc) of one query over the given lists: the candidates in ascending storage row"""
    ptr, list_rows = index["list_ptr"], index["list_rows"]
    books, codes = pq["codebooks"], pq["codes"]
    m, _, dsub = books.shape
    C = np.asarray(index["centroids"], np.float32)
    q = np.ascontiguousarray(q, np.float32)

    def tables(v):
        return [knn_ref.scores(v[None, j * dsub:(j + 1) * dsub], books[j], metric)[0] for j in range(m)]

    ip_tables = tables(q) if metric == knn_ref.IP else None
    rows, vals = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    with np.errstate(all="ignore"):
        for l in lists:
            pos = np.arange(ptr[l], ptr[l + 1])
            if pos.size == 0:
                continue
            if metric == knn_ref.IP:
                lut, start = ip_tables, knn_ref.scores(q[None], C[l:l + 1], knn_ref.IP)[0, 0]
            else:
                lut, start = tables(q - C[l]), np.float32(0)
            terms = np.stack([lut[j][codes[pos, j]] for j in range(m)], axis=1)
            chain = np.concatenate([np.full((pos.size, 1), start, np.float32), terms], axis=1)
            vals.append(np.cumsum(chain, axis=1, dtype=np.float32)[:, -1])
            rows.append(list_rows[pos])
    rows, vals = np.concatenate(rows), np.concatenate(vals)
    by_row = np.argsort(rows, kind="stable")
    return rows[by_row], vals[by_row]


def search(Q, X, index, pq, k, metric, nprobe, refine=0, ids=None, dist=None):
    """(ids[nq, k], dist[nq, k]).  refine = 0: the k best by ADC order with the adc as dist.  refine > 0: the `refine`
    best by ADC order re-scored exactly (dist: knn_ref.scores(Q, X, metric) when the caller has it already)."""
    Q = np.ascontiguousarray(Q, np.float32)
    assert refine == 0 or refine >= k
    if refine > 0 and dist is None:
        dist = knn_ref.scores(Q, X, metric)
    oi = np.empty((Q.shape[0], k), np.int64)
    od = np.empty((Q.shape[0], k), np.float32)
    for q, lists in enumerate(knn_ivf_ref.probes(Q, index, metric, nprobe)):
        rows, vals = adc(Q[q], index, pq, metric, lists)
        if refine > 0:
            best = knn_ref.take_k(vals[None, :], refine, metric, ids=rows)[0][0]
            rows = np.sort(best[best >= 0])
            vals = dist[q, rows]
        out_ids = rows if ids is None else np.asarray(ids, np.int64)[rows]
        oi[q], od[q] = (v[0] for v in knn_ref.take_k(vals[None, :], k, metric, ids=out_ids))
    return oi, od
