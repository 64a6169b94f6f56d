"""GLX_KNN_PREC_HALF over float8 tables (contract K-knn-half): the bits of the bfloat16 table of the same values.  Raw
distance bits, but NaNs as NaNs between two refine answers: a NaN there is the exact chain's, its payload the hardware's."""
import numpy as np
import pytest
import torch

import glx
import knn_ref
from test_gpu_knn import METRIC_NAMES, METRICS, Tuned, _cuda

pytestmark = pytest.mark.gpu
FP8 = {"float8_e4m3fn": torch.float8_e4m3fn, "float8_e5m2": torch.float8_e5m2}
both, types = pytest.mark.parametrize("metric", METRICS), pytest.mark.parametrize("dtype", FP8)


def run(f, Q, k, metric, **kw):
    ids, dist = f.search(Q if torch.is_tensor(Q) else _cuda(Q), k, METRIC_NAMES[metric], **kw)
    return ids.cpu().numpy(), dist.cpu().numpy()


def raw_same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def parity(f8, f16, Q, k, metric):
    """the half scan of both tables, the float8 one twice and under another chunking too -> its refine = 0 answer"""
    got = run(f8, Q, k, metric, precision="half")
    assert raw_same(got, run(f16, Q, k, metric, precision="half")) and raw_same(got, run(f8, Q, k, metric, precision="half"))
    with Tuned(knn_chunk_rows=128, knn_query_block=128):
        assert raw_same(got, run(f8, Q, k, metric, precision="half"))
    half = dict(precision="half", refine=1024)
    assert knn_ref.same(run(f8, Q, k, metric, **half), run(f16, Q, k, metric, **half))
    return got


def tables(codes, dtype, offset=0):
    """uint8 codes [n, dim] as (a torch float8 tensor as the table, the bfloat16 table of the same values): owned, or
    (offset 1) views at an odd element offset and a pitch of dim elements, which take the element-by-element front"""
    x8 = torch.from_numpy(codes).view(FP8[dtype])  # torch converts on the CPU only
    if not offset:
        return glx.Features(x8.cuda()), glx.Features(x8.float().cuda(), dtype="bfloat16")

    def view(x, tdt):
        flat = torch.cat([x.new_zeros(offset), x.reshape(-1)]).cuda()
        return glx.Features(flat[offset:].view(x.shape).view(tdt), view=True)
    return view(x8.view(torch.uint8), FP8[dtype]), view(x8.float().to(torch.bfloat16), torch.bfloat16)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dim", [1, 7, 8, 17, 64, 80, 130])
@both
@types
def test_bit_parity_with_the_bfloat16_scan(dtype, metric, dim, offset):
    """random codes (NaN, inf and subnormal codes among them), two row tiles and a 44-row tail, a query tile and two
    queries; dim: below a group, a tail group, one group, a step and a tail, one stage, two, three with a 2-column tail"""
    rng = np.random.default_rng(dim)
    parity(*tables(rng.integers(0, 256, (300, dim), dtype=np.uint8), dtype, offset),
           rng.standard_normal((130, dim)).astype(np.float32), 20, metric)


@pytest.mark.parametrize("dim", [8, 17])
@both
@types
def test_every_code(dtype, metric, dim):
    """all 256 codes in code order: a row's values lie within a few binades, so with small-integer queries every product,
    sum and norm is exact and the L2 distance rounds twice, as knn_l2 does: s = qn + xn, then fmaf(-2, ip, s)"""
    codes = (np.arange(-(-256 // dim) * dim) % 256).astype(np.uint8).reshape(-1, dim)  # the last row starts again at code 0
    n, Q = len(codes), np.random.default_rng(dim).integers(-3, 4, (16, dim)).astype(np.float32)
    ids, dist = parity(*tables(codes, dtype), Q, n, metric)
    X = torch.from_numpy(codes).view(FP8[dtype]).float().double().numpy()
    nan, keep = np.flatnonzero(np.isnan(X).any(1)), np.flatnonzero(np.isfinite(X).all(1))
    assert len(nan) and np.all(ids[:, n - len(nan):] == nan)  # NaN rows last, by row, each one NaN score
    assert np.all(dist.view(np.uint32)[:, n - len(nan):] == 0x7fc00000) and not np.isnan(dist[:, :n - len(nan)]).any()
    want = Q.astype(np.float64) @ X[keep].T
    if metric == knn_ref.L2:
        s = ((Q * Q).sum(1, dtype=np.float64)[:, None] + (X[keep] ** 2).sum(1)[None, :]).astype(np.float32)
        want = np.maximum(s - 2 * want, 0)
    got = np.take_along_axis(dist, np.argsort(ids, 1), 1)[:, keep]  # ids are rows here: dist by row
    assert np.array_equal(got, want.astype(np.float32))


@both
@types
def test_against_the_exact_search(dtype, metric):
    """integers of [-4, 4] are exact in all three types and so is the half score: the default answer, padding (k > num_rows)
    included, also from bfloat16 queries (the scan type).  Gaussian data: refine >= num_rows re-scores every row"""
    k, rng = 20, np.random.default_rng(3)
    for dim in (8, 17, 80):
        f = glx.Features(rng.integers(-4, 5, (300, dim)).astype(np.float32), dtype=dtype)
        Q = rng.integers(-4, 5, (130, dim)).astype(np.float32)
        for kw in ({}, {"refine": k}, {"refine": 1024}):
            assert raw_same(run(f, Q, k, metric, precision="half", **kw), run(f, Q, k, metric)), (dim, kw)
        assert raw_same(run(f, Q, 400, metric, precision="half"), run(f, Q, 400, metric))
        assert raw_same(run(f, _cuda(Q).to(torch.bfloat16), k, metric, precision="half"), run(f, Q, k, metric))
    f = glx.Features(rng.standard_normal((300, 33)).astype(np.float32), dtype=dtype)
    Q = rng.standard_normal((130, 33)).astype(np.float32)
    assert raw_same(run(f, Q, k, metric, precision="half", refine=1024), run(f, Q, k, metric))
