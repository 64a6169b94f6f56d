"""GPU tests of FP8 feature tables (float8_e4m3fn / float8_e5m2) on NaN, inf, signed-zero, subnormal and range-edge
codes (tests/fp8_special_values.py): lookup, all five aggregators at every kernel shape and knob -- 4 and 8 columns per
lane, scalar, legacy, the MFMA ablation, XCD stripes and slices, the Max / Min repeat-skip on and off -- aggregate_arg,
a captured plan, the exact and the IVF-Flat KNN search.

Every table is a uint8 code table uploaded as a torch float8 tensor as it is, so no rounding sits between the case
and the kernel.  Every expectation is the oracle (or the numpy restatement of the contract) on the float32 table of the
upcast values, torch's CPU upcast.  No tolerance anywhere (fp8_special_values.mismatch): non-NaN elements bit for bit,
sign of zero included; NaN positions exactly; whatever Max / Min select and every default_attr fill, every bit.  The
payload of an upcast NaN code is the hardware's (glx_common.h): printed, not asserted."""
import numpy as np
import pytest
import torch

import agg_backward_ref as ref
import agg_special_values as sv
import fp8_special_values as f8
import glx
import knn_ivf_ref
import knn_ref
from oracle_bindings import AGGREGATORS, Oracle
from test_gpu_agg_arg import OPS, _counts, _special_properties
from test_gpu_agg_arg import check as check_arg
from test_gpu_agg_special_values import _np, _requests, _want
from test_gpu_half_features import KNOB_DEFAULTS as REDUCE_KNOB_DEFAULTS
from test_gpu_half_features import KNOBS
from test_gpu_knn import METRICS, gpu_search
from test_gpu_knn_ivf import check_against_both, exported, same_index

pytestmark = pytest.mark.gpu
ORC = Oracle()
FP8 = [(n, getattr(torch, n)) for n in f8.NAMES]
KNOB_DEFAULTS = dict(REDUCE_KNOB_DEFAULTS, agg_repeats=0, agg_half_ld16=0)
FOUR_COLUMNS = [dict(agg_half_ld16=2), dict(agg_half_ld16=2, agg_xcd_slices=2)]  # 2: 4 columns per lane for every type
DIMS = [1, 3, 8, 64, 128, 256, 260, 264]  # scalar, scalar, 4 columns per lane up to 128; 256 and 264 (two column tiles)
# take 8 by default; 260 is no multiple of 8 and keeps 4


@pytest.fixture
def knobs():
    def set_knobs(**kw):
        for k, v in KNOB_DEFAULTS.items():
            glx.tune(k, kw.get(k, v))
    set_knobs()
    yield set_knobs
    set_knobs()


def _tensor(codes, tdt):
    return torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).view(tdt)


def _features(codes, tdt, host=False, ids=None, view=False):
    """the code table as an FP8 table: x_dtype == store_dtype, the bytes are stored as they are"""
    t = _tensor(codes, tdt)
    f = glx.Features(t.cuda(), view=True) if view else glx.Features(t if host else t.cuda(), ids=ids)
    assert f.dtype == f8.name_of(tdt)
    return f


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(got, want, op, label):
    e, c = _np(got[0]), _np(got[1])
    we, wc = want
    assert np.array_equal(c, wc), (label, op, "counts")
    m = f8.mismatch(e, we, op, wc)
    assert not m, "%s %s\n%s" % (label, op, m)


def _dense_seg(n, Sg):
    return (np.arange(n) // (n // Sg)).astype(np.int32)


# ---- 1. every kernel shape and knob ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", DIMS)
def test_every_knob_equals_oracle(knobs, name, tdt, D):
    d = sv.DEFAULTS[DIMS.index(D) % len(sv.DEFAULTS)]
    codes, ids, seg, Sg, d = f8.build_case(tdt, D, 7 * D + len(name), d)
    up = f8.upcast(codes, tdt)
    f = _features(codes, tdt)
    reqs = [(label, _cuda(i), _cuda(s), n, i, s) for label, i, s, n in _requests(ids, seg, Sg)]
    settings = KNOBS + FOUR_COLUMNS if D >= 32 else [dict(), dict(agg_legacy=1), dict(agg_mfma=1)]
    cache = {}
    for s in settings:
        knobs(**s)
        for op in AGGREGATORS:
            for label, ti, ts, n, hi, hs in reqs:
                got = f.aggregate(op, ti, ts, n, default_attr=float(d))
                _check(got, _want(cache, up, op, hi, hs, n, d), op, (name, D, label, s))


# ---- 2. every code in every byte of a dword and every lane slot ------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("how", ["owned", "view", "owned255", "view255"])
def test_every_code_in_every_slot(knobs, name, tdt, how):
    """circulant(256): 8 columns per lane by default (and under agg_half_ld16 = 1, whatever the default rule says), 4
    under agg_half_ld16 = 2, the legacy kernel and the MFMA ablation; 255 columns of it (an odd pitch: vec4 is false) take the scalar path.  Lookup of every row, and a dense
    fan-out of 1 through every operator: Prod of one row is 1 * x, which keeps -0 and the NaN positions."""
    codes = f8.circulant(256)
    if how.endswith("255"):
        codes = np.ascontiguousarray(codes[:, :255])
    up = f8.upcast(codes, tdt)
    f = _features(codes, tdt, view=how.startswith("view"))
    ids = np.arange(256, dtype=np.int64)
    ti, seg = _cuda(ids), np.arange(256, dtype=np.int32)
    want = {op: ORC.aggregate(up, op, ids, seg, 256, -0.0) for op in AGGREGATORS}
    for s in (dict(), dict(agg_half_ld16=2), dict(agg_half_ld16=1), dict(agg_legacy=1), dict(agg_mfma=1)):
        knobs(**s)
        got = _np(f.lookup(ti, default_attr=-0.0))
        m = f8.mismatch(got, up, "lookup", np.ones(256, np.int32))
        assert not m, (name, how, s, m)
        assert np.array_equal(np.isnan(got), f8.nan_mask(codes, name)), (name, how, s)
        for op in AGGREGATORS:
            _check(f.aggregate(op, ti, None, 256, default_attr=-0.0), want[op], op, (name, how, s))


# ---- 3. hashed ids, host pointers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [3, 8, 128, 264])
def test_hashed_ids_and_host_pointers(name, tdt, D):
    for k, d in enumerate(sv.DEFAULTS):
        codes, ids, seg, Sg, d = f8.build_case(tdt, D, 100 + D + k, d, blocks=1)
        up = f8.upcast(codes, tdt)
        raw = np.arange(codes.shape[0], dtype=np.int64) * 5 - 17
        req = np.where((ids >= 0) & (ids < codes.shape[0]), ids * 5 - 17, ids)
        fd = _features(codes, tdt, ids=_cuda(raw))
        fh = _features(codes, tdt, host=True, ids=raw)  # host float8 tensor and host ids: the host staging path
        for op in AGGREGATORS:
            want = ORC.aggregate(up, op, req, seg, Sg, float(d), ids=raw)
            _check(fd.aggregate(op, _cuda(req), _cuda(seg), Sg, default_attr=float(d)), want, op, (name, D, d, "device"))
            _check(fh.aggregate(op, req, seg, Sg, default_attr=float(d)), want, op, (name, D, d, "host"))


# ---- 4. the Max / Min repeat-skip (G == 64 && VEC == 4) on FP8 rows --------------------------------------------------
REPEAT_LENGTHS = [1, 2, 63, 64, 65, 130, 300]
NAN_ROW, MIXED_ROW, EDGE_ROW, LOW_ROW, NZERO_ROW, PLANTED = 0, 1, 2, 3, 4, 5
REPEAT_ROWS = 80


def _repeat_table(name, tdt, D):
    rng = np.random.default_rng(D)
    special = f8.pool(tdt)
    codes = special[rng.integers(0, special.shape[0], (REPEAT_ROWS, D))]
    plain = rng.random((REPEAT_ROWS, D)) < 0.5
    ordinary = (rng.standard_normal(int(plain.sum())) * 3).astype(np.float32)
    codes[plain] = torch.from_numpy(ordinary).to(tdt).view(torch.uint8).numpy()  # ordinary numbers of the type
    hi, sub = f8.HI[name], f8.SUB[name]
    nan = f8.NAN_CODES[name]
    codes[NAN_ROW] = np.resize(np.array(nan, np.uint8), D)  # an all-NaN-code row, every NaN code
    num = f8.code_of([-0.0, 0.0, hi, -40.0, sub, -sub, -hi], tdt)
    mixed = [nan[0], num[0], num[1], num[2], num[3], num[4], nan[-1], num[5], num[6]]
    codes[MIXED_ROW] = np.resize(np.array(mixed, np.uint8), D)
    edge = [f8.INF, -f8.INF] if name == "float8_e5m2" else [hi, -hi]  # the inf row (e4m3fn has none: its largest numbers)
    codes[EDGE_ROW] = np.resize(f8.code_of(edge + edge[:1], tdt), D)
    codes[LOW_ROW] = f8.code_of([-40.0], tdt)[0]  # Max keeps its -37
    codes[NZERO_ROW] = f8.NEG_ZERO
    return np.ascontiguousarray(codes)


def _repeat_segment(rng, pattern, n):
    """n ids of a segment in which few distinct rows repeat many times"""
    if pattern == 0:  # one row, a planted one
        return np.full(n, rng.integers(0, PLANTED), np.int64)
    if pattern == 1:  # ABAB
        a, b = rng.integers(0, REPEAT_ROWS, 2)
        return np.where(np.arange(n) % 2 == 0, a, b).astype(np.int64)
    if pattern == 2:  # the NaN row repeated around one ordinary row and the mixed row
        ids = np.full(n, NAN_ROW, np.int64)
        ids[n // 2] = PLANTED + 1
        ids[n // 3::7] = MIXED_ROW
        return ids
    if pattern == 3:  # three rows, one of them unknown, drawn with replacement
        return np.array([rng.integers(0, REPEAT_ROWS), REPEAT_ROWS + 5, rng.integers(0, PLANTED)], np.int64)[rng.integers(0, 3, n)]
    if pattern == 4:  # position 64 + k repeats position k: a repeat only across the 64-position chunk boundary
        return rng.permutation(REPEAT_ROWS)[:64][np.arange(n) % 64].astype(np.int64)
    return rng.integers(0, PLANTED, 3)[rng.integers(0, 3, n)].astype(np.int64)  # three planted rows


REPEAT_PATTERNS = 6


@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [256, 512])
def test_repeat_skip_on_and_off(knobs, name, tdt, D):
    """agg_half_ld16 = 2 puts these rows on 4 columns per lane (G = 64 at D = 256: the repeat-skip is on); the default
    takes 8 (G = 32: off).  Crossed with agg_repeats 0 / 1 / 2, all six equal the oracle and therefore each other."""
    codes = _repeat_table(name, tdt, D)
    up = f8.upcast(codes, tdt)
    f = _features(codes, tdt)
    rng = np.random.default_rng(3 * D)
    reqs = []
    for L in REPEAT_LENGTHS:  # dense: two segments of every pattern per length
        Sg = 2 * REPEAT_PATTERNS
        ids = np.concatenate([_repeat_segment(rng, s % REPEAT_PATTERNS, L) for s in range(Sg)])
        reqs.append(("dense %d" % L, ids, None, Sg))
    sizes = [L for p in range(REPEAT_PATTERNS) for L in REPEAT_LENGTHS] + [0, 17, 0]
    sizes = [0] + [sizes[i] for i in rng.permutation(len(sizes))]
    ids = np.concatenate([_repeat_segment(rng, (s + 1) % REPEAT_PATTERNS, n) for s, n in enumerate(sizes) if n > 0])
    reqs.append(("ragged", ids, np.repeat(np.arange(len(sizes), dtype=np.int32), sizes), len(sizes)))
    dev = [(label, _cuda(i), _cuda(s), n, i, s) for label, i, s, n in reqs]
    cache = {}
    d = np.float32(sv.DEFAULTS[0])
    for ld16 in (2, 0):
        for repeats in (0, 1, 2):
            knobs(agg_half_ld16=ld16, agg_repeats=repeats)
            for op in AGGREGATORS:
                for label, ti, ts, n, hi, hs in dev:
                    got = f.aggregate(op, ti, ts, n, default_attr=float(d))
                    _check(got, _want(cache, up, op, hi, hs, n, d), op, (name, D, label, ld16, repeats))


# ---- 5. aggregate_arg ------------------------------------------------------------------------------------------------
ARG_DIMS = [3, 8, 100, 264]  # scalar, G = 2, G = 32, two column tiles


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", ARG_DIMS)
def test_aggregate_arg(D, name, tdt, op):
    k = ARG_DIMS.index(D)
    codes, ids, seg, Sg, d = f8.build_case(tdt, D, 200 + D, sv.DEFAULTS[k % len(sv.DEFAULTS)])
    up = f8.upcast(codes, tdt)
    f = _features(codes, tdt)
    n10 = len(ids) // 10
    for label, i, s, n in (("ragged", ids, seg, Sg), ("dense", ids[:n10 * 10].copy(), None, n10)):
        cnt = _counts(s, len(i), n)
        start = ref.segment_starts(None if s is None else cnt, len(i), n)
        emb, arg = ref.fold_arg(OPS[op], up, i, start, d)
        # emb, cnt and arg bit for bit, twice, and emb / cnt equal to Features.aggregate's
        got = check_arg(f, OPS[op], i, s, n, float(d), (emb, cnt, arg), label=(label, D, name))
        known = (i >= 0) & (i < up.shape[0])
        vals = np.where(known[:, None], up[np.where(known, i, 0)], np.float32(d)).astype(np.float32)
        seen = _special_properties(OPS[op], got[0], got[2], vals, start)
        if label == "ragged":  # the scenario blocks: every property is exercised, none holds vacuously
            if name == "float8_e4m3fn":  # waived: the type has no inf (only an infinite default_attr brings one in)
                del seen["inf_taken"], seen["inf_ignored"]
            assert all(v > 0 for v in seen.values()), seen


# ---- 6. lookup ---------------------------------------------------------------------------------------------------------
def _pool_table(tdt, V, D, rng):
    special = f8.pool(tdt)
    return np.ascontiguousarray(special[rng.integers(0, special.shape[0], (V, D))])


@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [1, 3, 8, 64, 264])
def test_lookup_keeps_what_it_must(name, tdt, D):
    rng = np.random.default_rng(D)
    V = 300
    codes = _pool_table(tdt, V, D, rng)
    up = f8.upcast(codes, tdt)
    raw = rng.permutation(5 * V)[:V].astype(np.int64) * 3 - 100
    for ids_kind in ("dense", "hashed"):
        known = np.arange(V, dtype=np.int64) if ids_kind == "dense" else raw
        q = np.concatenate([known[rng.integers(0, V, 700)], np.array([-1, 10 ** 9, -7], np.int64)])
        row_of = {int(k): i for i, k in enumerate(known)}
        rows = np.array([row_of.get(int(x), -1) for x in q])
        for host in (False, True):
            ids = None if ids_kind == "dense" else (raw if host else _cuda(raw))
            f = _features(codes, tdt, host=host, ids=ids)
            for dflt in sv.DEFAULTS:
                got = _np(f.lookup(q if host else _cuda(q), default_attr=dflt))
                want = np.where((rows >= 0)[:, None], up[np.maximum(rows, 0)], np.float32(dflt))
                m = f8.mismatch(got, want, "lookup", (rows >= 0).astype(np.int32))
                assert not m, (name, D, ids_kind, host, dflt, m)
                assert np.array_equal(np.isnan(got[rows >= 0]), f8.nan_mask(codes, name)[rows[rows >= 0]])


@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("offset,D", [(1, 128), (2, 128), (3, 128), (0, 127), (0, 129)])
def test_views_off_alignment_take_the_scalar_path(name, tdt, offset, D):
    """test_views_at_every_byte_offset_and_odd_pitch's layouts -- a base off by 1-3 bytes, a pitch that is no multiple of
    4 -- on a table of special codes: the scalar convert reads every code at every byte address"""
    rng = np.random.default_rng(100 * offset + D)
    V = 300
    codes = _pool_table(tdt, V, D, rng)
    up = f8.upcast(codes, tdt)
    buf = torch.zeros(V * D + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + V * D] = torch.from_numpy(codes.reshape(-1)).cuda()
    Xv = buf[offset:offset + V * D].view(tdt).view(V, D)
    assert Xv.data_ptr() % 4 == offset % 4 and Xv.is_contiguous()
    v = glx.Features(Xv, view=True)
    assert v.dtype == name
    q = rng.integers(-1, V + 1, 1500).astype(np.int64)
    known = (q >= 0) & (q < V)
    for dflt in sv.DEFAULTS[:2]:
        got = _np(v.lookup(_cuda(q), default_attr=dflt))
        want = np.where(known[:, None], up[np.where(known, q, 0)], np.float32(dflt))
        m = f8.mismatch(got, want, "lookup", known.astype(np.int32))
        assert not m, (name, offset, D, dflt, m)
        for op in AGGREGATORS:
            _check(v.aggregate(op, _cuda(q), None, 300, default_attr=dflt),
                   ORC.aggregate(up, op, q, _dense_seg(1500, 300), 300, dflt), op, (name, offset, D, dflt))


# ---- 7. upload of out-of-range float32 -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("host", [False, True])
def test_upload_of_out_of_range_float32_through_the_reduce(name, tdt, host):
    """the documented overflow rule -- NaN for e4m3fn, inf for e5m2 -- seen through the reduce, not only the lookup"""
    vals = np.concatenate([np.array([np.inf, -np.inf, 1e30, -1e30, 465.0, -465.0, 61441.0, -61441.0, -0.0, 1e-40, 1.0, -2.0],
                                    np.float32), sv.f32([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF])])
    rng = np.random.default_rng(7)
    V, D = 64, 8
    X = vals[rng.integers(0, vals.shape[0], (V, D))]
    X[:vals.shape[0], 0] = vals  # every value at least once
    up = torch.from_numpy(X).to(tdt).float().numpy()
    big = np.abs(X) > 1e6
    assert (np.isnan(up[big]).all() and not np.isinf(up).any()) if name == "float8_e4m3fn" else np.isinf(up[big]).all()
    f = glx.Features(torch.from_numpy(X) if host else torch.from_numpy(X).cuda(), dtype=name)
    assert f.dtype == name
    sizes = rng.integers(0, 6, 120)
    seg = np.repeat(np.arange(120, dtype=np.int32), sizes)
    ids = rng.integers(-1, V + 1, seg.shape[0]).astype(np.int64)
    dense = rng.integers(-1, V + 1, 300).astype(np.int64)
    for op in AGGREGATORS:
        for dflt in (sv.DEFAULTS[0], 1.25):
            _check(f.aggregate(op, _cuda(ids), _cuda(seg), 120, default_attr=dflt),
                   ORC.aggregate(up, op, ids, seg, 120, dflt), op, (name, host, "ragged", dflt))
            _check(f.aggregate(op, dense, None, 100, default_attr=dflt),
                   ORC.aggregate(up, op, dense, _dense_seg(300, 100), 100, dflt), op, (name, host, "dense", dflt))


# ---- 8. a captured plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg", ["SumAggregator", "MaxAggregator", "MeanAggregator"])
def test_plan_with_special_codes(agg):
    """test_gpu_agg_special_values.py::test_plan_with_special_values' graph over an e5m2 code table at D = 256"""
    import synth
    name, tdt = "float8_e5m2", torch.float8_e5m2
    V, D = 3000, 256
    rp, col, eid, w = synth.small_graph(V, 40000, seed=9, weighted=True, hub_degree=1000)
    g = glx.Graph(_cuda(rp), _cuda(col), _cuda(eid), _cuda(w))
    rng = np.random.default_rng(6)
    codes = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(tdt).view(torch.uint8).numpy().copy()
    special = f8.pool(tdt)
    mask = rng.random((V, D)) < 0.05
    codes[mask] = special[rng.integers(0, special.shape[0], int(mask.sum()))]
    codes[0] = f8.NEG_ZERO  # the hub row
    codes[0, ::7] = np.resize(np.array(f8.NAN_CODES[name], np.uint8), codes[0, ::7].shape[0])
    up = f8.upcast(codes, tdt)
    f = _features(codes, tdt)
    plan = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[f, f], agg=agg, seed=5)
    try:
        for run in range(2):
            seeds = _cuda(rng.integers(0, V, 512).astype(np.int64))
            hops = plan.run(seeds, call_counter=10 * run)
            hops = [{k: v.clone() for k, v in h.items()} for h in hops]
            want_ids = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, [25, 10], seed=5, call_counter=10 * run)
            torch.cuda.synchronize()
            for h in range(2):
                ids = want_ids[h][0].view(-1).cpu().numpy()
                n, k = want_ids[h][0].shape
                want = ORC.aggregate(up, agg, ids, (np.arange(n * k) // k).astype(np.int32), n)
                _check((hops[h]["emb"], hops[h]["cnt"]), want, agg, ("plan", run, h))
    finally:
        plan.close()


# ---- 9. KNN --------------------------------------------------------------------------------------------------------------
def _knn_tables(name, tdt, rng, dim=33):
    """test_gpu_knn.py::test_special_values' table from numbers of the type, as codes; and its queries (float32)"""
    hi, sub, nan = f8.HI[name], f8.SUB[name], f8.NAN_CODES[name]
    codes = torch.from_numpy(rng.standard_normal((300, dim)).astype(np.float32)).to(tdt).view(torch.uint8).numpy().copy()
    assert not f8.nan_mask(codes, name).any()
    pinf, ninf = f8.code_of([f8.INF, -f8.INF] if name == "float8_e5m2" else [hi, -hi], tdt)  # e4m3fn: no inf, the largest
    codes[10, -1] = pinf  # in the LAST column of an odd dim: the column the matrix cores do not run
    codes[11, -1] = ninf
    codes[12, 0] = pinf
    zero, nzero, psub, nsub = f8.code_of([0.0, -0.0, sub, -sub], tdt)
    codes[20] = zero
    codes[20, -1] = nsub  # a row of zeros with one smallest-subnormal element, in the last column ...
    codes[21] = zero
    codes[21, 4] = psub  # ... and in a matrix-core column, -0 behind it
    codes[21, 5:] = nzero
    codes[22] = nzero  # all -0
    codes[30:40] = np.resize(np.array(nan, np.uint8), (10, dim))  # every NaN code
    codes[45, 7] = nan[-1]
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    Q[1] = 0  # 0 * inf
    Q[2] = 1e-30
    Q[3, 2] = np.nan  # a NaN query: every score a NaN, rows in order
    Q[4] = 3e38  # overflows to inf (and inf - inf under L2)
    Q[5] = -1e-44  # a subnormal query: its products with the table underflow to zeros of either sign
    Q[6] = 1e-38
    few = np.resize(np.array(nan, np.uint8), (300, dim))  # only 5 rows hold numbers
    good = [7, 50, 123, 200, 299]
    few[good] = codes[good]
    return np.ascontiguousarray(codes), Q, np.ascontiguousarray(few), good


@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("metric", METRICS)
def test_exact_search_on_special_codes(name, tdt, metric):
    codes, Q, few, good = _knn_tables(name, tdt, np.random.default_rng(4))
    up = f8.upcast(codes, tdt)
    for f in (_features(codes, tdt), _features(codes, tdt, view=True)):  # a view builds its row norms per search
        for k in (1, 10, 300):
            assert knn_ref.same(gpu_search(f, Q, k, metric), knn_ref.search(Q, up, k, metric)), (name, k)
    # a table in which only 5 rows hold numbers: the NaNs are listed behind them, by row
    ids, dist = gpu_search(_features(few, tdt), Q[:1], 10, metric)
    assert knn_ref.same((ids, dist), knn_ref.search(Q[:1], f8.upcast(few, tdt), 10, metric))
    assert sorted(ids[0, :5].tolist()) == good and ids[0, 5:].tolist() == [0, 1, 2, 3, 4]
    assert not np.isnan(dist[0, :5]).any() and np.isnan(dist[0, 5:]).all()


@pytest.mark.parametrize("name,tdt", FP8)
def test_ivf_flat_on_special_codes(name, tdt):
    """as test_gpu_knn_ivf.py::test_special_values_and_half_tables does for float32: planted centroids, then
    build_ivf(7, niter=2) -- NaN and inf rows flow into the centroids -- against the restatement.  (IVF-PQ has no
    float32 special-value restatement to compare with.)"""
    codes, Q, few, good = _knn_tables(name, tdt, np.random.default_rng(16))
    up = f8.upcast(codes, tdt)
    f = _features(codes, tdt)
    C = up[[0, 1, 2, 3, 50, 100, 200]].copy()
    ix = f.build_ivf(7, niter=0, centroids=C)
    index = exported(ix)
    assert same_index(index, knn_ivf_ref.build(up, 7, niter=0, centroids=C))
    check_against_both(f, ix, up, Q, (1, 10, 300), (1, 3, 6), index=index)
    for metric in METRICS:  # the flat search is itself right here
        assert knn_ref.same(gpu_search(f, Q, 10, metric), knn_ref.search(Q, up, 10, metric))
    ix2 = f.build_ivf(7, niter=2)
    index2 = exported(ix2)
    assert same_index(index2, knn_ivf_ref.build(up, 7, niter=2))
    check_against_both(f, ix2, up, Q, (10,), (1, 6), index=index2)


# ---- 10. what the device's upcast of a NaN code looks like (reported, not asserted) ----------------------------------
def test_report_upcast_nan_payloads(capsys):
    lines = []
    for name, tdt in FP8:
        nan = np.array(f8.NAN_CODES[name], np.uint8)
        want = sv.bits(f8.upcast(nan, tdt))
        ids = torch.arange(4, device="cuda")
        for label, codes in (("packed convert", np.tile(np.resize(nan, 8), (4, 1))), ("scalar convert", np.tile(np.resize(nan, 7), (4, 1)))):
            got = sv.bits(_np(_features(codes, tdt).lookup(ids)))[0]
            assert np.isnan(got.view(np.float32)).all()
            lines.append("%s, %s: codes %s -> device %s; torch %s" % (
                name, label, ["%02x" % c for c in nan], ["%08x" % x for x in got[:len(nan)]], ["%08x" % x for x in want]))
    with capsys.disabled():
        print("\nNaN payloads of upcast FP8 NaN codes:\n  " + "\n  ".join(lines))
