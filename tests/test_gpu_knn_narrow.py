"""GLX_KNN_TILE_NARROW (contract K-knn-narrow): the exact search through 32-query tiles against float64 on small-integer
data, and raw-bit parity with the wide tile on Gaussian data with special values, in every precision and refine mode."""
import numpy as np
import pytest
import torch

import glx
import knn_ref

pytestmark = pytest.mark.gpu
METRICS = {"l2": knn_ref.L2, "ip": knn_ref.IP}
TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16,
         "float8_e4m3fn": torch.float8_e4m3fn, "float8_e5m2": torch.float8_e5m2}
# (num_queries, num_rows, dim, k, knn_chunk_rows): the query tile's edge and a second and third tile; less than a wave's
# rows, the row tile's edge, several tiles per walk; an odd last column, the stage edges (32 / 64 columns), load tails,
# more stages than the LDS keeps queries for (dim 130 exact, 260 half); k = 1, padding (k > num_rows); several chunks
CASES = [(1, 1, 1, 1, 0), (31, 255, 2, 20, 0), (32, 256, 31, 20, 0), (33, 257, 33, 300, 0), (65, 700, 65, 20, 256),
         (33, 700, 130, 1, 0), (33, 257, 260, 20, 0)]


def search(f, Q, k, metric, **kw):
    ids, dist = f.search(torch.from_numpy(Q).cuda(), k, metric, **kw)
    return ids.cpu().numpy(), dist.cpu().numpy()


def chunked(rows, call):
    if not rows:
        return call()
    glx.tune("knn_chunk_rows", rows)
    try:
        return call()
    finally:
        glx.tune("knn_chunk_rows", -1)


def table(X, dtype, offset):
    """X as a table of dtype: owned, or (offset > 0) a view whose base is offset elements into an allocation"""
    x = torch.from_numpy(X).to(TORCH[dtype])
    if not offset:
        return glx.Features(x.cuda())
    pad = offset * x.element_size()
    flat = torch.cat([torch.zeros(pad, dtype=torch.uint8), x.view(torch.uint8).reshape(-1)]).cuda()
    return glx.Features(flat[pad:].view(TORCH[dtype]).view(x.shape), view=True)


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16", "float8_e4m3fn"])
def test_exact_against_float64(dtype, case):
    """integers of [-4, 4]: every product, partial sum and norm is exact in every type, and ties are everywhere"""
    nq, n, dim, k, rows = case
    rng = np.random.default_rng(dim)
    X, Q = (rng.integers(-4, 5, (m, dim)).astype(np.float32) for m in (n, nq))
    f = table(X, dtype, 0)
    for name, metric in METRICS.items():
        X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
        d64 = Q64 @ X64.T if metric == knn_ref.IP else ((Q64[:, None, :] - X64[None, :, :]) ** 2).sum(-1)
        want = knn_ref.take_k(d64.astype(np.float32), k, metric)
        got = chunked(rows, lambda: search(f, Q, k, name, tile="narrow"))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


MODES = [("float32", "float32", False), ("bfloat16", "float32", False)] + [
    (dt, "half", refine) for dt in ("bfloat16", "float16", "float8_e5m2") for refine in (False, True)]


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("mode", MODES, ids=str)
def test_bit_parity_with_the_wide_tile(mode, case):
    """Gaussian data with an inf, a NaN, a -0.0 and a subnormal in the table and in the queries; the 700-row tables are
    views off alignment (one element; 8 bytes in the half modes), which take the element-load front"""
    (dtype, precision, refine), (nq, n, dim, k, rows) = mode, case
    rng = np.random.default_rng(n + dim)
    X, Q = (rng.standard_normal((m, dim)).astype(np.float32) for m in (n, nq))
    for A in (X, Q):
        for i, v in enumerate((np.inf, np.nan, -0.0, 1e-40)):
            A.flat[(7 * i + 3) % A.size] = v
    f = table(X, dtype, (4 if precision == "half" else 1) if n == 700 else 0)
    kw = dict(precision=precision, refine=k if refine else 0)
    for name in METRICS:
        wide = search(f, Q, k, name, **kw)
        narrow = chunked(rows, lambda: search(f, Q, k, name, tile="narrow", **kw))
        assert np.array_equal(narrow[0], wide[0]), name
        if refine:  # a NaN there is the exact chain's, its payload the hardware's
            assert np.array_equal(knn_ref.bits(narrow[1]), knn_ref.bits(wide[1])), name
        else:
            assert np.array_equal(narrow[1].view(np.int32), wide[1].view(np.int32)), name


def test_surface():
    rng = np.random.default_rng(0)
    X, Q = rng.standard_normal((300, 33)).astype(np.float32), rng.standard_normal((5, 33)).astype(np.float32)
    f = glx.Features(X)
    refusals = []
    for tile in ("wide", "narrow"):
        with pytest.raises(glx.GlxError) as e:
            f.search(Q, 3, "ip", precision="half", tile=tile)
        refusals.append((e.value.code, str(e.value)))
    assert refusals[0] == refusals[1] and refusals[0][0] == 3
    ids, dist = f.search(Q[:0], 3, "l2", tile="narrow")
    assert ids.shape == (0, 3) and dist.shape == (0, 3)
    host = f.search(Q, 3, "l2", tile="narrow")  # host pointers in and out
    assert knn_ref.same(host, knn_ref.search(Q, X, 3, knn_ref.L2))
    again = search(f, Q, 3, "l2", tile="narrow")
    assert np.array_equal(host[0], again[0]) and np.array_equal(host[1].view(np.int32), again[1].view(np.int32))
