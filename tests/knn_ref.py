"""Restatement of the KNN search contract (include/glx.h, "exact KNN search"): the fmaf chain, the L2 formula, the total
order, the padding and the merge.  The chain needs a real single-rounding fmaf, so the scores come from a few lines of C
compiled on first use (gcc -O2 -ffp-contract=off, libm's fmaf) into a temporary directory; float64 emulation would
round twice.  Everything else is numpy."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

L2, IP = 0, 1
METRICS = {"l2": L2, "ip": IP}

_C = r"""
#include <math.h>
#include <stdlib.h>
static float chain(const float* a, const float* b, int d) {
  float acc = 0.0f;
  for (int c = 0; c < d; ++c) acc = fmaf(a[c], b[c], acc);
  return acc;
}
/* out[q, r] = dist of query q and row r; metric 0 = L2, 1 = IP */
int knn_scores(const float* Q, const float* X, int nq, int n, int d, int metric, float* out) {
  float* xn = (float*)malloc(sizeof(float) * (n > 0 ? n : 1));
  if (!xn) return 1;
  for (int r = 0; r < n; ++r) xn[r] = chain(X + (size_t)r * d, X + (size_t)r * d, d);
  for (int q = 0; q < nq; ++q) {
    const float* qv = Q + (size_t)q * d;
    const float qn = chain(qv, qv, d);
    for (int r = 0; r < n; ++r) {
      const float ip = chain(qv, X + (size_t)r * d, d);
      if (metric == 1) {
        out[(size_t)q * n + r] = ip;
      } else {
        const float s = qn + xn[r];
        const float dd = fmaf(-2.0f, ip, s);
        out[(size_t)q * n + r] = dd < 0.0f ? 0.0f : dd;
      }
    }
  }
  free(xn);
  return 0;
}
"""

_lib = None


def _clib():
    global _lib
    if _lib is None:
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("knn_ref needs a C compiler (gcc or cc) for a single-rounding fmaf")
        d = tempfile.mkdtemp(prefix="knn_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, so = os.path.join(d, "knn_ref.c"), os.path.join(d, "knn_ref.so")
        with open(src, "w") as f:
            f.write(_C)
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src, "-lm"], check=True)
        L = ctypes.CDLL(so)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.knn_scores.argtypes = [vp, vp, ci, ci, ci, ci, vp]
        _lib = L
    return _lib


def scores(Q, X, metric):
    """dist[nq, n] float32 of float32 queries Q[nq, d] against float32 rows X[n, d] under the contract."""
    Q = np.ascontiguousarray(Q, np.float32)
    X = np.ascontiguousarray(X, np.float32)
    assert Q.ndim == 2 and X.ndim == 2 and Q.shape[1] == X.shape[1]
    out = np.empty((Q.shape[0], X.shape[0]), np.float32)
    rc = _clib().knn_scores(Q.ctypes.data, X.ctypes.data, Q.shape[0], X.shape[0], Q.shape[1], int(metric), out.ctypes.data)
    assert rc == 0
    return out


def order(dist, metric):
    """Per query, the positions of dist[nq, n] best first: better dist, then (float equality, +0 == -0) the smaller
    position; NaN after every number, by position."""
    nan = np.isnan(dist)
    key = np.where(nan, np.float32(0), dist if metric == L2 else -dist)
    pos = np.broadcast_to(np.arange(dist.shape[1]), dist.shape)
    out = np.empty(dist.shape, np.int64)
    for q in range(dist.shape[0]):
        out[q] = np.lexsort((pos[q], key[q], nan[q]))  # the last key is the primary one
    return out


def pad_dist(metric):
    return np.float32(np.inf) if metric == L2 else np.float32(-np.inf)


def take_k(dist, k, metric, ids=None, perm=None):
    """(ids[nq, k], dist[nq, k]) from a full score matrix; slots past n hold id -1 and the pad distance."""
    nq, n = dist.shape
    perm = order(dist, metric) if perm is None else perm
    m = min(k, n)
    rows = perm[:, :m]
    oi = np.full((nq, k), -1, np.int64)
    od = np.full((nq, k), pad_dist(metric), np.float32)
    oi[:, :m] = rows if ids is None else np.asarray(ids, np.int64)[rows]
    od[:, :m] = np.take_along_axis(dist, rows, axis=1)
    return oi, od


def search(Q, X, k, metric, ids=None):
    return take_k(scores(Q, X, metric), k, metric, ids)


def merge(ids, dist, metric):
    """KnnResponse::Merge under the contract: ids / dist [parts, nq, k] -> the k best per query; ties to the lower part,
    then the earlier position; id -1 entries are absent."""
    parts, nq, k = ids.shape
    flat_i = np.transpose(ids, (1, 0, 2)).reshape(nq, parts * k)
    flat_d = np.transpose(dist, (1, 0, 2)).reshape(nq, parts * k)
    oi = np.full((nq, k), -1, np.int64)
    od = np.full((nq, k), pad_dist(metric), np.float32)
    for q in range(nq):
        keep = np.flatnonzero(flat_i[q] != -1)
        perm = keep[order(flat_d[q, keep][None, :], metric)[0]][:k]
        oi[q, :perm.size] = flat_i[q, perm]
        od[q, :perm.size] = flat_d[q, perm]
    return oi, od


def bits(d):
    """float32 bits with every NaN mapped to one pattern (which NaN a NaN distance is, is the hardware's)."""
    d = np.ascontiguousarray(d, np.float32)
    return np.where(np.isnan(d), np.uint32(0x7fc00000), d.view(np.uint32))


def same(got, want):
    """(ids, dist) pairs equal: ids exactly, dist bit for bit (NaNs as NaNs)."""
    return np.array_equal(np.asarray(got[0]), want[0]) and np.array_equal(bits(np.asarray(got[1])), bits(want[1]))


def brute64(Q, X, k, metric):
    """ids of a float64 brute force (for well-separated data only: no tie handling beyond a stable sort)."""
    Q64, X64 = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    if metric == IP:
        s = -(Q64 @ X64.T)
    else:
        s = ((Q64[:, None, :] - X64[None, :, :]) ** 2).sum(-1)
    return np.argsort(s, axis=1, kind="stable")[:, :k].astype(np.int64)
