"""CPU tests of the aggregation oracle (oracle/glx_oracle.c) on NaN, inf, signed-zero, subnormal and overflowing
inputs (tests/agg_special_values.py):

  (a) a plain numpy restatement of the reference's InitFunc / AggFunc / FinalFunc and of the stitch against
      Oracle.aggregate / Oracle.aggregate_stitch -- a second, independent statement of the same fold;
  (b) live against the reference's own Aggregator::Aggregate (oracle/_ref/libglref.so, when built);
  (c) against the committed golden tests/golden/agg_special.npz that the reference produced (make_golden.py
      gen_agg_special), which is also what the GPU tests compare with.

Non-NaN elements compare bit for bit (sign of zero included) and NaN positions exactly; NaN payloads are compared
where the output is a move (Max / Min selections, default_attr fills) -- agg_special_values.mismatch."""
import os

import numpy as np
import pytest

import agg_special_values as sv
from oracle_bindings import AGGREGATORS, Oracle, RefLib, have_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_special.npz")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def test_value_set_hits_every_case():
    """The scenario block of build_case really reduces every scenario, in every column position it claims."""
    for D in (1, 3, 8, 64):
        X, ids, seg, Sg, _ = sv.build_case(D, 1, 0.0)
        seen = set()
        for s in range(Sg):
            rows = ids[seg == s]
            if rows.size == 0 or (rows >= X.shape[0]).any() or (rows < 0).any():
                continue
            for j in range(D):
                seen.add(tuple(X[rows, j].view(np.uint32).tolist()))
        for sc in sv.SCENARIOS:
            assert tuple(np.array(sc, np.float32).view(np.uint32).tolist()) in seen, (D, sc)
        assert np.isnan(X).any() and np.isinf(X).any() and (X.view(np.uint32) == 0x80000000).any()
        sub = (np.abs(X) < sv.TINY) & (X != 0)
        assert sub.any()
        assert (np.bincount(seg, minlength=Sg) == 0).any() and (ids == 10 ** 9).any()


@pytest.mark.parametrize("D", [1, 3, 8, 64])
@pytest.mark.parametrize("dflt", sv.DEFAULTS + [1.25])
def test_numpy_model_equals_oracle(orc, D, dflt):
    X, ids, seg, Sg, d = sv.build_case(D, 10 + D, dflt)
    for name in AGGREGATORS:
        want, wc = sv.model_aggregate(X, name, ids, seg, Sg, d)
        got, gc = orc.aggregate(X, name, ids, seg, Sg, float(d))
        assert np.array_equal(gc, wc), (D, name)
        m = sv.mismatch(got, want, name, wc)
        assert not m, (D, dflt, name, m)


def test_numpy_model_knows_the_reference_quirks(orc):
    """Hand-checked answers of the operator the model restates: Max / Min skip a NaN and depend on the order of +-0,
    Min over +inf alone is FLT_MAX and Max over -inf alone -37, Sum turns -0 into +0, Prod keeps its sign,
    subnormal products and means survive."""
    cases = [("MaxAggregator", [-0.0, 0.0], 0x80000000), ("MaxAggregator", [0.0, -0.0], 0x00000000),
             ("MinAggregator", [-0.0, 0.0], 0x80000000), ("MinAggregator", [0.0, -0.0], 0x00000000),
             ("MaxAggregator", [sv.NAN[0], sv.NAN[1]], 0xC2140000), ("MinAggregator", [sv.INF], 0x7F7FFFFF),
             ("MaxAggregator", [-sv.INF], 0xC2140000), ("MaxAggregator", [1.0, sv.NAN[0], 2.0], 0x40000000),
             ("SumAggregator", [-0.0], 0x00000000), ("ProdAggregator", [-0.0], 0x80000000),
             ("ProdAggregator", [1e-20, 1e-20], 0x000116C2),
             ("MeanAggregator", [sv.SUB, sv.SUB, sv.SUB], 0x00000001), ("MeanAggregator", [sv.FLT_MAX, sv.FLT_MAX], 0x7F800000),
             ("SumAggregator", [sv.INF, -sv.INF], None), ("ProdAggregator", [sv.INF, 0.0], None)]
    for name, seq, want in cases:
        X = np.array(seq, np.float32).reshape(-1, 1)
        ids = np.arange(len(seq), dtype=np.int64)
        seg = np.zeros(len(seq), np.int32)
        e, _ = sv.model_aggregate(X, name, ids, seg, 1, 0.0)
        o, _ = orc.aggregate(X, name, ids, seg, 1)
        got = int(e.view(np.uint32)[0, 0])
        if want is None:
            assert np.isnan(e[0, 0]) and np.isnan(o[0, 0]), (name, seq)
        else:
            assert got == want and int(o.view(np.uint32)[0, 0]) == want, (name, seq, hex(got))
    # the product 1e-20 * 1e-20 is subnormal, not flushed
    assert 0 < abs(float(np.float32(1e-20) * np.float32(1e-20))) < sv.TINY


def _stitch_parts(rng, P, Sg, D):
    pool = np.array(sv.POOL, np.float32)
    parts = pool[rng.integers(0, pool.shape[0], (P, Sg, D))]
    cnts = rng.integers(0, 4, (P, Sg)).astype(np.int32)
    cnts[:, 0] = 0  # a segment no shard saw
    cnts[0, 1] = 0
    return parts, cnts


@pytest.mark.parametrize("P,Sg,D", [(1, 9, 3), (3, 40, 8), (8, 25, 17)])
@pytest.mark.parametrize("dflt", sv.DEFAULTS)
def test_numpy_model_equals_oracle_stitch(orc, P, Sg, D, dflt):
    rng = np.random.default_rng(P * 100 + D)
    parts, cnts = _stitch_parts(rng, P, Sg, D)
    for name in AGGREGATORS:
        for ref_fold in (False, True):
            want, wc = sv.model_stitch(name, parts, cnts, np.float32(dflt), reference_fold=ref_fold)
            got, gc = orc.aggregate_stitch(name, parts, cnts, dflt, reference_fold=ref_fold)
            assert np.array_equal(gc, wc), (name, ref_fold)
            m = sv.mismatch(got, want, name, wc)
            assert not m, (P, D, dflt, name, ref_fold, m)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_half_upcast_equals_torch_vectorised_conversion(dtype):
    """agg_special_values.half_upcast (the GPU tests' expectation for half tables) against torch's conversion of a
    contiguous tensor of whole vectors, special values and random bit patterns included."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    extra = sv.f32([0x7F800001, 0xFF800123, 0x80000001, 0x477FF000, 0x477FEFFF, 0x33000001, 0x387FE000, 0x7F7F8000])
    x = np.concatenate([np.array(sv.POOL, np.float32), extra,
                        rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = np.concatenate([x, np.zeros(-x.size % 64, np.float32)])
    want = torch.from_numpy(x).to(getattr(torch, dtype)).float().numpy()
    assert np.array_equal(sv.bits(sv.half_upcast(x, dtype)), sv.bits(want))


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("D", [1, 3, 8, 17])
@pytest.mark.parametrize("dflt", sv.DEFAULTS)
def test_oracle_equals_reference_on_special_values(orc, D, dflt):
    """The oracle against the reference's own Aggregator::Aggregate on the special-value tables (the reference takes
    the floats in binary, NaN payloads included), hashed raw ids."""
    X, ids, seg, Sg, d = sv.build_case(D, 900 + D, dflt)
    raw = np.arange(X.shape[0], dtype=np.int64) * 3 - 11
    req = np.where((ids >= 0) & (ids < X.shape[0]), ids * 3 - 11, ids)  # unknown ids stay unknown
    ref = RefLib(default_float_attr=float(d))
    ntype = "agg_sp_%d_%d" % (D, sv.DEFAULTS.index(dflt))  # a node type of its own: the reference's storage outlives ref
    try:
        ref.add_nodes(ntype, raw, X)
        for name in AGGREGATORS:
            want, wc = ref.aggregate(ntype, name, req, seg, Sg, D)
            got, gc = orc.aggregate(X, name, req, seg, Sg, float(d), ids=raw)
            assert np.array_equal(gc, wc), (D, name)
            m = sv.mismatch(got, want, name, wc)
            assert not m, (D, dflt, name, m)
    finally:
        ref.close()


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built (needs /root/reference)")
def test_oracle_stitch_equals_reference_on_special_values(orc):
    rng = np.random.default_rng(4)
    parts, cnts = _stitch_parts(rng, 3, 30, 8)
    ref = RefLib()
    try:
        for name in AGGREGATORS:
            want, wc = ref.aggregate_stitch(name, parts, cnts)
            got, gc = orc.aggregate_stitch(name, parts, cnts, 0.0, reference_fold=True)
            assert np.array_equal(gc, wc), name
            m = sv.mismatch(got, want, name, wc)
            assert not m, (name, m)
    finally:
        ref.close()


def test_oracle_equals_golden_special_values(orc):
    """tests/golden/agg_special.npz: the reference's answers on the special-value tables."""
    g = np.load(GOLD)
    assert int(g["num_cases"]) >= 8
    for c in range(int(g["num_cases"])):
        X, ids, seg = g["c%d_X" % c], g["c%d_ids" % c], g["c%d_seg" % c]
        Sg, d = int(g["c%d_num_segments" % c]), float(g["c%d_default" % c])
        for name in AGGREGATORS:
            want, wc = g["c%d_%s_emb" % (c, name)], g["c%d_%s_cnt" % (c, name)]
            got, gc = orc.aggregate(X, name, ids, seg, Sg, d)
            assert np.array_equal(gc, wc), (c, name)
            m = sv.mismatch(got, want, name, wc)
            assert not m, (c, name, m)
            # the recorded default fills keep the NaN payload of the default
            if np.isnan(d):
                assert (want[wc == 0].view(np.uint32) == np.float32(d).view(np.uint32)).all()


def test_golden_special_values_regenerate_identically():
    """The recipe (make_golden.py gen_agg_special) reproduces the committed file's arrays, when the reference is built."""
    if not have_ref():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    import sys
    import tempfile
    sys.path.insert(0, os.path.dirname(GOLD))
    import make_golden
    with tempfile.TemporaryDirectory() as tmp:
        old = make_golden.OUT_DIR
        make_golden.OUT_DIR = tmp
        ref = RefLib(storage_mode=2)
        try:
            make_golden.gen_agg_special(ref)
        finally:
            ref.close()
            make_golden.OUT_DIR = old
        a, b = np.load(os.path.join(tmp, "agg_special.npz")), np.load(GOLD)
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
