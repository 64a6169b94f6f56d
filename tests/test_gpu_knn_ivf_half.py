"""The half-precision list-major IVF-Flat search (KnnIvf.search(schedule="list", precision="half"),
glx_knn_ivf_search_prec) on the GPU: against a float64 brute force on data whose arithmetic is exact in every scan type,
and bit for bit against the flat half-precision scan on Gaussian data with inf / NaN / -0.0."""
import numpy as np
import pytest
import torch

import glx
import knn_ivf_ref
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, NAN, Tuned, _cuda
from test_gpu_knn_ivf_list import SIZES, brute64

pytestmark = pytest.mark.gpu

INVALID = 3


def run(ix, Q, k, metric, host=False, **kw):
    """(ids, dist) as numpy; the output buffers start as canaries, so an unwritten element shows"""
    out = (np.full((len(Q), k), -7, np.int64), np.full((len(Q), k), NAN, np.float32))
    if host:
        return ix.search(np.ascontiguousarray(Q), k, METRIC_NAMES[metric], out=out, **kw)
    out = ix.search(_cuda(Q), k, METRIC_NAMES[metric], out=(_cuda(out[0]), _cuda(out[1])), **kw)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


HALF = {"schedule": "list", "precision": "half"}


@pytest.mark.parametrize("dim", [1, 16, 17, 72])  # the tail group only; one step; a step and a tail; a second stage
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float8_e4m3fn"])
def test_exact_integer_data_equals_a_float64_brute_force(dtype, metric, dim):
    """Integers in [-3, 3]: every product and sum is exact in every scan type, so float64 gives the contract's bits and
    ties.  The planted lists of test_gpu_knn_ivf_list: column 0 names a row's list, 129 queries share their ranks."""
    rng = np.random.default_rng(200 + dim)
    C = np.zeros((8, dim), np.float32)
    C[:, 0] = [-3, -2, -1, 0, 1, 2, 3, 3]
    X = rng.integers(-3, 4, (sum(SIZES), dim)).astype(np.float32)
    X[:, 0] = rng.permutation(np.repeat(C[:, 0], SIZES))
    Q = rng.integers(-3, 4, (130, dim)).astype(np.float32)
    Q[:129, 0] = 0
    ix = glx.Features(X, dtype=dtype).build_ivf(8, niter=0, centroids=C)
    ptr, rows = ix.lists()
    index = {"centroids": C, "list_ptr": ptr, "list_rows": rows}
    assert np.diff(ptr).tolist() == SIZES
    for nprobe in (1, 2, 8):
        lists = knn_ivf_ref.probes(Q, index, metric, nprobe)
        for k in (1, 20, 300):
            want_ids, want_dist = brute64(Q, X, index, lists, k, metric)
            ids, dist = run(ix, Q, k, metric, nprobe=nprobe, **HALF)
            assert np.array_equal(ids, want_ids), (nprobe, k)
            assert np.array_equal(dist, want_dist.astype(np.float32)), (nprobe, k)


@pytest.fixture(scope="module")
def gaussian():
    """1,500 x 33 with one +inf, one NaN and a row of -0.0, a NaN in one query -> (queries, {dtype: (stored values as
    float32, index)}); "as_bf16" is the bfloat16 table of the float8_e5m2 table's values"""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((1500, 33)).astype(np.float32)
    X[100, 32], X[700, 5], X[900] = np.inf, np.nan, -0.0
    Q = rng.standard_normal((200, 33)).astype(np.float32)
    Q[17, 3] = np.nan
    tabs = {}
    for name, dt in (("bfloat16", torch.bfloat16), ("float8_e5m2", torch.float8_e5m2)):
        stored = torch.from_numpy(X).to(dt)
        tabs[name] = (stored.float().numpy(), glx.Features(stored).build_ivf(7, niter=2))
    V = tabs["float8_e5m2"][0]
    tabs["as_bf16"] = (V, glx.Features(torch.from_numpy(V).to(torch.bfloat16)).build_ivf(7, niter=2))
    return Q, tabs


CASES = [(m, k, refine) for m in METRICS for k, refine in ((1, 0), (50, 0), (10, 64))]


@pytest.mark.parametrize("dtype", ["bfloat16", "float8_e5m2"])
def test_bits_are_the_flat_half_scans(gaussian, dtype):
    Q, tabs = gaussian
    V, ix = tabs[dtype]
    f = ix.features
    ptr, rows = ix.lists()
    index = {"centroids": ix.centroids(), "list_ptr": ptr, "list_rows": rows}
    for metric, k, refine in CASES:
        tag = (metric, k, refine)
        # (a) every list probed: the flat half scan itself
        flat = f.search(Q, k, METRIC_NAMES[metric], precision="half", refine=refine)
        assert knn_ref.same(run(ix, Q, k, metric, nprobe=7, refine=refine, **HALF), flat), tag
        # (b) three lists probed: the flat half scan of a table that holds exactly the probed rows
        got = run(ix, Q, k, metric, nprobe=3, refine=refine, **HALF)
        lists = knn_ivf_ref.probes(Q, index, metric, 3)
        for q in (0, 17, 64, 130, 199):
            cand = np.sort(np.concatenate([rows[ptr[l]:ptr[l + 1]] for l in lists[q]]))
            sub = glx.Features(torch.from_numpy(V[cand]).to(getattr(torch, f.dtype)), ids=cand)
            want = sub.search(Q[q:q + 1], k, METRIC_NAMES[metric], precision="half", refine=refine)
            assert knn_ref.same((got[0][q:q + 1], got[1][q:q + 1]), want), tag + (q,)
        # (c) the same bits again, through host pointers, and with one round per probe rank in 64-query blocks
        assert knn_ref.same(run(ix, Q, k, metric, nprobe=3, refine=refine, **HALF), got), tag
        assert knn_ref.same(run(ix, Q, k, metric, host=True, nprobe=3, refine=refine, **HALF), got), tag
        with Tuned(knn_list_cand_cap=1, knn_query_block=64):
            assert knn_ref.same(run(ix, Q, k, metric, nprobe=3, refine=refine, **HALF), got), tag
        # (d) a float8 table returns what the bfloat16 table of the same values returns
        if dtype == "float8_e5m2":
            assert knn_ref.same(run(tabs["as_bf16"][1], Q, k, metric, nprobe=3, refine=refine, **HALF), got), tag


@pytest.mark.parametrize("metric", METRICS)
def test_refine_over_every_probed_row_is_the_float32_search(gaussian, metric):
    """refine = 1024 keeps every row a query probes whenever its three lists hold at most 1,024 rows: the re-rank then
    sees what the float32 search sees.  The largest three lists of this index hold 1,088 rows together, so the few
    queries that probe exactly those are left to the parity with the flat scan above."""
    Q, tabs = gaussian
    ix = tabs["bfloat16"][1]
    ptr, rows = ix.lists()
    lists = knn_ivf_ref.probes(Q, {"centroids": ix.centroids(), "list_ptr": ptr, "list_rows": rows}, metric, 3)
    whole = np.diff(ptr)[lists].sum(1) <= 1024
    assert whole.sum() >= 50  # of 200: the comparison below is not an empty one
    want = run(ix, Q, 10, metric, nprobe=3, schedule="query")
    got = run(ix, Q, 10, metric, nprobe=3, refine=1024, **HALF)
    assert knn_ref.same((got[0][whole], got[1][whole]), (want[0][whole], want[1][whole]))


def test_arguments(gaussian):
    Q, tabs = gaussian
    ix = tabs["bfloat16"][1]
    ix32 = glx.Features(tabs["bfloat16"][0]).build_ivf(7, niter=0, centroids=ix.centroids())
    L = glx.lib()
    with pytest.raises(ValueError):
        ix.search(Q, 5, nprobe=2, schedule="list", precision="fast")
    # (index, schedule, precision, refine) -> the word the refusal names
    for index, schedule, precision, refine, word in ((ix, 0, 1, 0, b"schedule"), (ix32, 1, 1, 0, b"float32"),
                                                     (ix, 1, 0, 5, b"refine")):
        ids, dist = np.full((200, 5), -7, np.int64), np.full((200, 5), NAN, np.float32)
        rc = L.glx_knn_ivf_search_prec(index._h, 1, Q.ctypes.data, 200, 5, 2, schedule, precision, refine,
                                       ids.ctypes.data, dist.ctypes.data, 0, None)
        assert rc == INVALID and word in L.glx_last_error(), word
        assert np.all(ids == -7) and np.all(np.isnan(dist)), word
    with pytest.raises(glx.GlxError):
        ix.search(Q, 5, nprobe=2, schedule="query", precision="half")
    with pytest.raises(glx.GlxError):
        ix.search(Q, 5, nprobe=2, schedule="list", precision="float32", refine=5)
    for schedule in (0, 1):  # GLX_KNN_PREC_F32 is glx_knn_ivf_search_ex
        ids, dist = np.full((200, 5), -7, np.int64), np.full((200, 5), NAN, np.float32)
        rc = L.glx_knn_ivf_search_prec(ix._h, 1, Q.ctypes.data, 200, 5, 2, schedule, 0, 0, ids.ctypes.data,
                                       dist.ctypes.data, 0, None)
        assert rc == 0
        assert knn_ref.same((ids, dist), run(ix, Q, 5, knn_ref.IP, host=True, nprobe=2, schedule=("query", "list")[schedule]))
