"""GPU tests of the Max / Min reduce that does not load a row its segment has already folded (glx_aggregate.hip
agg_first_occurrences / agg_keep_batch; glx_tune("agg_repeats", 1) loads every position again, 2 skips at every segment
length, 0 -- the default -- where segments average 16 positions or more).  Every case is compared bit for bit,
embeddings and counts, under 2 and 0 with the same call under agg_repeats = 1, and with a numpy left-to-right fold in
float32; Sum, Mean and Prod on the same inputs must not see the knob at all.  The rows hold NaN, +-inf, +-0, values at
or below Max's -37 start and at or above Min's FLT_MAX start; the segments repeat rows in every way the survivor mask
can meet: all one row, none, ABAB, a repeat only across the 64-position chunk boundary, unknown ids."""
import numpy as np
import pytest
import torch

import glx

pytestmark = pytest.mark.gpu
F32 = np.finfo(np.float32)
DEFAULT_ATTR = 1.25
KNOB_DEFAULTS = dict(agg_repeats=0, agg_segs=0, agg_xcd_slices=0, agg_xcd_stripes=-1, agg_xcd_chunk=0)
FANOUTS = [1, 2, 10, 25, 63, 64, 65, 130]
SELECTS = ["MaxAggregator", "MinAggregator"]
OTHERS = ["SumAggregator", "MeanAggregator", "ProdAggregator"]
NAN_ROW, PINF_ROW, NINF_ROW, PZERO_ROW, NZERO_ROW, LOW_ROW, HIGH_ROW, MIXED_ROW, FINITE_ROW = range(9)
V = 300
PATTERNS = 8


@pytest.fixture
def knobs():
    def set_knobs(**kw):
        for k, v in KNOB_DEFAULTS.items():
            glx.tune(k, kw.get(k, v))
    try:
        yield set_knobs
    finally:
        set_knobs()


def table(D, seed=0):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((V, D)) * 3).astype(np.float32)
    X[rng.random((V, D)) < 0.02] = -50.0
    X[NAN_ROW] = np.nan
    X[PINF_ROW] = np.inf
    X[NINF_ROW] = -np.inf
    X[PZERO_ROW] = 0.0
    X[NZERO_ROW] = -0.0
    X[LOW_ROW] = np.resize(np.array([-37.0, -38.0, -50.0, -np.inf, -3.4e38], np.float32), D)  # Max keeps its -37
    X[HIGH_ROW] = np.resize(np.array([F32.max, np.inf], np.float32), D)  # Min keeps its FLT_MAX
    X[MIXED_ROW] = np.resize(np.array([np.nan, 2.0, -0.0, 0.0, np.inf, -40.0, 1e-45, -1e-45], np.float32), D)
    X[FINITE_ROW] = 0.5
    return X


_TABLES = {}


def features(D, dtype="float32"):
    """(Features, the float32 values its rows read as), made once per shape and storage type."""
    key = (D, dtype)
    if key not in _TABLES:
        X = table(D)
        if dtype == "float32":
            up = X
            f = glx.Features(torch.from_numpy(X).cuda(), device=0)
        else:
            up = torch.from_numpy(X).to(getattr(torch, dtype)).float().numpy()
            f = glx.Features(torch.from_numpy(X).cuda(), device=0, dtype=dtype)
        _TABLES[key] = (f, up)
    return _TABLES[key]


def segment(rng, pattern, n):
    """n raw ids of one segment; unknown ids are -1 and V + 5."""
    distinct = rng.permutation(V)[:n] if n <= V else rng.integers(0, V, n)
    if pattern == 0:  # all one row (often a planted one)
        return np.full(n, rng.integers(0, 12), np.int64)
    if pattern == 1:  # all distinct
        return distinct.astype(np.int64)
    if pattern == 2:  # ABAB...
        a, b = rng.integers(0, V, 2)
        return np.where(np.arange(n) % 2 == 0, a, b).astype(np.int64)
    if pattern == 3:  # distinct inside each 64-position piece, position 64 + k repeats position k
        ids = distinct.astype(np.int64)
        if n > 64:
            k = min(64, n - 64)
            ids[64:64 + k] = ids[:k]
        else:
            ids[-1] = ids[0]
        return ids
    if pattern == 4:  # an out-of-range id, repeated
        ids = distinct.astype(np.int64)
        ids[::3] = V + 5
        return ids
    if pattern == 5:  # -1 between valid rows
        ids = distinct.astype(np.int64)
        ids[1::2] = -1
        return ids
    if pattern == 6:  # the NaN row repeated around a finite one
        ids = np.full(n, NAN_ROW, np.int64)
        ids[n // 2] = FINITE_ROW
        ids[n // 3::7] = MIXED_ROW if n > 8 else NAN_ROW
        return ids
    return rng.integers(0, 12, 3)[rng.integers(0, 3, n)].astype(np.int64)  # draws with replacement from 3 rows


def request(sizes, offset, seed):
    rng = np.random.default_rng(seed)
    parts = [segment(rng, (s + offset) % PATTERNS, int(n)) for s, n in enumerate(sizes) if n > 0]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def fold_ref(op, up, ids, sizes):
    """The reference's serial loop: start value, left-to-right select, default_attr for unknown ids and empty segments."""
    D = up.shape[1]
    rows = np.where((ids >= 0) & (ids < V), ids, V)
    Xd = np.concatenate([up, np.full((1, D), DEFAULT_ATTR, np.float32)])
    out = np.empty((len(sizes), D), np.float32)
    init = np.float32(-37.0) if op == "MaxAggregator" else F32.max
    sizes = np.asarray(sizes)
    ends = np.cumsum(sizes)
    with np.errstate(invalid="ignore"):
        if len(sizes) and (sizes == sizes[0]).all() and sizes[0] > 0:  # dense: all segments at once
            x = Xd[rows.reshape(len(sizes), -1)]
            acc = np.full((len(sizes), D), init, np.float32)
            for j in range(x.shape[1]):
                r = x[:, j]
                acc = np.where((acc < r) if op == "MaxAggregator" else (r < acc), r, acc)
            return acc
        for s, n in enumerate(sizes):
            acc = np.full(D, init, np.float32)
            for r in Xd[rows[ends[s] - n:ends[s]]]:
                acc = np.where((acc < r) if op == "MaxAggregator" else (r < acc), r, acc)
            out[s] = acc if n > 0 else DEFAULT_ATTR
    return out


def run(f, op, ids, seg, Sg):
    e, c = f.aggregate(op, ids, seg, Sg, default_attr=DEFAULT_ATTR)
    torch.cuda.synchronize()
    return e, c


def check(knobs, f, up, h_ids, sizes, dense, label, others=True, **setting):
    Sg = len(sizes)
    ids = torch.from_numpy(h_ids).cuda()
    seg = None if dense else torch.from_numpy(np.repeat(np.arange(Sg, dtype=np.int32), sizes)).cuda()
    for op in SELECTS + (OTHERS if others else []):
        knobs(agg_repeats=1, **setting)
        e1, c1 = run(f, op, ids, seg, Sg)
        for mode in (2, 0):  # first occurrences only whatever the segment length; the default (by length)
            knobs(agg_repeats=mode, **setting)
            e0, c0 = run(f, op, ids, seg, Sg)
            assert torch.equal(c0, c1) and np.array_equal(c0.cpu().numpy(), np.asarray(sizes, np.int32)), (label, op, mode)
            assert torch.equal(e0.view(torch.int32), e1.view(torch.int32)), (label, op, mode)
        if op in SELECTS:
            want = fold_ref(op, up, h_ids, sizes)
            assert np.array_equal(e0.cpu().numpy().view(np.uint32), want.view(np.uint32)), (label, op)


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("fanout", FANOUTS)
def test_dense_responses(knobs, D, fanout):
    """1, 3, 4 and 5 segments (a workgroup holds four at D = 256) with every pattern in every place, and a few thousand."""
    f, up = features(D)
    for Sg in (1, 3, 4, 5):
        for offset in range(PATTERNS):
            check(knobs, f, up, request([fanout] * Sg, offset, 100 * fanout + offset), [fanout] * Sg, True,
                  (D, fanout, Sg, offset), others=offset == 0)
    Sg = 2051
    check(knobs, f, up, request([fanout] * Sg, 0, fanout), [fanout] * Sg, True, (D, fanout, Sg))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float8_e4m3fn", "float8_e5m2"])
def test_half_tables(knobs, dtype):
    f, up = features(256, dtype)
    for fanout, Sg in ((25, 1037), (130, 5)):
        check(knobs, f, up, request([fanout] * Sg, 3, fanout), [fanout] * Sg, True, (dtype, fanout, Sg))


def ragged_sizes(Sg, seed):
    sizes = np.random.default_rng(seed).integers(0, 30, Sg)
    sizes[[0, 2, Sg - 1]] = 0
    sizes[[1, 7]] = 1
    sizes[[3, 9]] = 70
    sizes[5] = 200
    return sizes


@pytest.mark.parametrize("D", [256, 512])
def test_explicit_ragged_segment_ids(knobs, D):
    """Lengths 0, 1, 70 and 200 among short ones: the mask is per segment and per 64-position piece."""
    f, up = features(D)
    for offset in (0, 3, 6):
        sizes = ragged_sizes(203, offset)
        check(knobs, f, up, request(sizes, offset, 9 + offset), sizes, False, (D, "ragged", offset), others=offset == 0)


@pytest.mark.parametrize("setting", [dict(agg_segs=3), dict(agg_xcd_stripes=1, agg_xcd_chunk=3),
                                     dict(agg_xcd_stripes=1, agg_xcd_chunk=1, agg_segs=3), dict(agg_xcd_slices=2)],
                         ids=["segs3", "stripes", "stripes_segs3", "slices2"])
def test_launch_knobs(knobs, setting):
    """Several segments per wave (one id chunk serves them: pieces start inside a chunk), XCD stripes forced on a small
    request, and two column slices (32 lanes per segment at D = 256: the launch that keeps loading every position)."""
    f, up = features(256)
    for fanout, Sg in ((10, 2051), (25, 1030), (65, 37), (130, 11)):
        check(knobs, f, up, request([fanout] * Sg, 2, fanout), [fanout] * Sg, True, (setting, fanout, Sg), **setting)
    sizes = ragged_sizes(203, 1)
    check(knobs, f, up, request(sizes, 1, 4), sizes, False, (setting, "ragged"), **setting)


def test_twice_and_on_a_second_stream(knobs):
    f, up = features(256)
    fanout, Sg = 25, 2051
    h_ids = request([fanout] * Sg, 5, 77)
    ids = torch.from_numpy(h_ids).cuda()
    knobs(agg_repeats=2)
    first, cnt = run(f, "MaxAggregator", ids, None, Sg)
    again, _ = run(f, "MaxAggregator", ids, None, Sg)
    side = torch.cuda.Stream(device=0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, other_cnt = f.aggregate("MaxAggregator", ids, None, Sg, default_attr=DEFAULT_ATTR)
        side.synchronize()
    want = fold_ref("MaxAggregator", up, h_ids, [fanout] * Sg)
    for e in (first, again, other):
        assert np.array_equal(e.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(cnt, other_cnt)
