"""CPU tests of the FP8 special-value inputs (tests/fp8_special_values.py): every scenario value is a number of its
type, the plain float32 model of the reduce -- alone, no GPU -- produces every outcome the GPU tests rely on (so none of
them holds vacuously), the model equals the oracle on the upcast tables, and the circulant table holds every code in
every column."""
import numpy as np
import pytest

import agg_special_values as sv
import fp8_special_values as f8
from oracle_bindings import AGGREGATORS, Oracle

torch = pytest.importorskip("torch")
FP8 = [(n, getattr(torch, n)) for n in f8.NAMES]


@pytest.mark.parametrize("name,tdt", FP8)
def test_every_scenario_value_is_a_number_of_the_type(name, tdt):
    """float32 -> float8 -> float32 gives the same bits back; a NaN stays a NaN; lengths reach past every agg_unroll"""
    nans = f8._NanCodes(name)
    longest = 0
    for sc in f8.scenarios(tdt):
        x = np.array(sc, np.float32)
        back = torch.from_numpy(x).to(tdt).float().numpy()
        nan = np.isnan(x)
        assert np.array_equal(sv.bits(back)[~nan], sv.bits(x)[~nan]), (name, sc)
        assert np.isnan(back[nan]).all() and not np.isnan(back[~nan]).any(), (name, sc)
        codes = f8.encode(sc, tdt, nans)  # the codes the tables hold: the same numbers, NaN codes where the NaNs are
        up = f8.upcast(codes, tdt)
        assert np.array_equal(sv.bits(up)[~nan], sv.bits(x)[~nan]) and np.isnan(up[nan]).all(), (name, sc)
        assert np.array_equal(f8.nan_mask(codes, name), nan), (name, sc)
        longest = max(longest, len(sc))
    assert longest == 17 and nans.at >= 3 * len(f8.NAN_CODES[name])  # beyond agg_unroll = 15; every NaN code, often
    with pytest.raises(ValueError):
        f8.code_of([0.3], tdt)


@pytest.mark.parametrize("name,tdt", FP8)
def test_the_nan_codes_are_the_codes_that_upcast_to_nan(name, tdt):
    allc = np.arange(256, dtype=np.uint8)
    up = f8.upcast(allc, tdt)
    assert np.array_equal(np.isnan(up), f8.nan_mask(allc, name))
    assert sv.bits(up)[f8.NEG_ZERO] == 0x80000000
    assert np.isinf(up).sum() == (2 if name == "float8_e5m2" else 0)
    finite = up[np.isfinite(up)]
    assert finite.max() == f8.HI[name] and finite.min() == -f8.HI[name]
    assert np.abs(finite[finite != 0]).min() == f8.SUB[name]
    assert up[up > -37].min() == f8.ABOVE_37[name] and up[up < -37].max() == -40.0
    p = f8.pool(tdt)
    assert len(set(p.tolist())) == len(p) and set(f8.NAN_CODES[name]) <= set(p.tolist())


@pytest.mark.parametrize("name,tdt", FP8)
def test_build_case_reduces_every_scenario_with_every_nan_code(name, tdt):
    for D in (1, 3, 8, 64):
        codes, ids, seg, Sg, _ = f8.build_case(tdt, D, 1, 0.0)
        assert codes.dtype == np.uint8 and codes.shape[1] == D
        up = f8.upcast(codes, tdt)
        seen = set()
        for s in range(Sg):
            rows = ids[seg == s]
            if rows.size == 0 or (rows >= codes.shape[0]).any() or (rows < 0).any():
                continue
            for j in range(D):
                col = up[rows, j]
                seen.add(tuple(np.where(np.isnan(col), np.uint32(0x7FC00000), sv.bits(col)).tolist()))
        for sc in f8.scenarios(tdt):
            x = np.array(sc, np.float32)
            key = tuple(np.where(np.isnan(x), np.uint32(0x7FC00000), sv.bits(x)).tolist())
            assert key in seen, (name, D, sc)
        assert set(f8.NAN_CODES[name]) <= set(codes.reshape(-1).tolist())
        assert (codes == f8.NEG_ZERO).any()
        assert (np.bincount(seg, minlength=Sg) == 0).any() and (ids == 10 ** 9).any() and (ids == -1).any()
        only_unknown = [s for s in range(Sg) if (seg == s).any() and (ids[seg == s] == 10 ** 9).all()]
        assert only_unknown


def _inputs(up, ids, seg, Sg, d):
    """per segment: the [n, D] float32 values it folds (default_attr rows for unknown ids)"""
    known = (ids >= 0) & (ids < up.shape[0])
    vals = np.where(known[:, None], up[np.where(known, ids, 0)], np.float32(d)).astype(np.float32)
    return [vals[seg == s] for s in range(Sg)]


@pytest.mark.parametrize("name,tdt", FP8)
def test_the_model_alone_produces_every_outcome_the_gpu_tests_rely_on(name, tdt):
    """A condition on the inputs: on build_case(tdt, 8, ...) the sequential float32 model shows, in at least one column
    each, the outcomes a wrong kernel would change."""
    codes, ids, seg, Sg, d = f8.build_case(tdt, 8, 5, 1.25)
    up = f8.upcast(codes, tdt)
    pieces = _inputs(up, ids, seg, Sg, d)
    out = {op: sv.model_aggregate(up, op, ids, seg, Sg, d)[0] for op in sv.AGGREGATORS}
    seen = dict(max_start=0, min_start=0, prod_inf=0, prod_subnormal=0, prod_zero=0, max_neg_zero=0, min_neg_zero=0,
                nan_dropped=0, nan_kept=0, sum_nan_without_nan=0)
    for s, piece in enumerate(pieces):
        if piece.shape[0] == 0:
            continue
        has_nan, all_nan = np.isnan(piece).any(0), np.isnan(piece).all(0)
        mx, mn, pr, sm = (out[op][s] for op in ("MaxAggregator", "MinAggregator", "ProdAggregator", "SumAggregator"))
        seen["max_start"] += int(((mx == -37.0) & ~has_nan).sum())
        seen["min_start"] += int((mn == sv.FLT_MAX).sum())
        clean = ~has_nan & ~(piece == 0).any(0)
        seen["prod_inf"] += int((np.isinf(pr) & ~np.isinf(piece).any(0) & ~has_nan).sum())
        seen["prod_subnormal"] += int(((pr != 0) & (np.abs(pr) < sv.TINY) & clean).sum())
        seen["prod_zero"] += int(((pr == 0) & clean).sum())
        seen["max_neg_zero"] += int((sv.bits(mx) == 0x80000000).sum())
        seen["min_neg_zero"] += int((sv.bits(mn) == 0x80000000).sum())
        seen["nan_dropped"] += int((has_nan & ~all_nan & ~np.isnan(mx) & (mx != -37.0)).sum())
        seen["nan_kept"] += int((has_nan & np.isnan(sm)).sum())
        seen["sum_nan_without_nan"] += int((~has_nan & np.isnan(sm)).sum())
    assert not np.isnan(out["MaxAggregator"]).any() and not np.isnan(out["MinAggregator"]).any()  # a select never takes one
    if name == "float8_e4m3fn":  # no inf: inf + -inf cannot happen, and Sum cannot overflow at these lengths
        assert seen.pop("sum_nan_without_nan") == 0
    assert all(v > 0 for v in seen.values()), (name, seen)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [1, 3, 8, 64])
def test_numpy_model_equals_oracle_on_upcast_tables(orc, name, tdt, D):
    """the oracle is the C restatement built from this repository: it needs no reference build, so nothing skips here"""
    dims = [1, 3, 8, 64]
    for k, dflt in enumerate([sv.DEFAULTS[dims.index(D)], sv.DEFAULTS[(dims.index(D) + 2) % 4], 1.25]):
        codes, ids, seg, Sg, d = f8.build_case(tdt, D, 10 + D + k, dflt, blocks=1 if k else 2)
        up = f8.upcast(codes, tdt)
        for op in AGGREGATORS:
            want, wc = sv.model_aggregate(up, op, ids, seg, Sg, d)
            got, gc = orc.aggregate(up, op, ids, seg, Sg, float(d))
            assert np.array_equal(gc, wc), (name, D, op)
            m = f8.mismatch(got, want, op, wc)
            assert not m, (name, D, dflt, op, m)


def test_circulant_holds_each_code_once_per_column():
    for D in (256, 255):
        c = f8.circulant(D)
        assert c.shape == (256, D) and c.dtype == np.uint8
        assert all(np.array_equal(np.sort(c[:, j]), np.arange(256)) for j in range(D))


def test_mismatch_rule():
    want = np.array([[1.0, -0.0, np.nan, 2.0]], np.float32)
    other_payload = want.copy()
    other_payload.view(np.uint32)[0, 2] = 0xFFC00001
    for op in ("SumAggregator", "ProdAggregator", "lookup"):
        assert not f8.mismatch(other_payload, want, op, np.array([1]))      # an arithmetic / upcast NaN: any payload
        assert f8.mismatch(other_payload, want, op, np.array([0]))          # a default_attr fill: every bit
    assert f8.mismatch(other_payload, want, "MaxAggregator", np.array([1]))  # a select: every bit
    zero = want.copy()
    zero[0, 1] = 0.0
    moved = want.copy()
    moved[0, 2], moved[0, 3] = 2.0, np.nan
    for op in ("SumAggregator", "MaxAggregator", "lookup"):
        assert f8.mismatch(zero, want, op, np.array([1])) and f8.mismatch(moved, want, op, np.array([1]))
