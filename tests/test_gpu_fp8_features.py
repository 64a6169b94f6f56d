"""GPU tests of FP8 feature tables (GLX_DTYPE_F8E4M3 / GLX_DTYPE_F8E5M2): one-byte OCP float8 storage, float32
accumulation.  The upload's float32 -> float8 conversion must equal torch's bit for bit; the upcast must be exact at
every non-NaN code; every lookup, aggregation and KNN search of an FP8 table must equal -- bit for bit -- the same call
on the float32 table of its upcast values (and so the oracle on that table), for every kernel shape, alignment and knob
the launcher can select.  No tolerance anywhere."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import glx
from oracle_bindings import Oracle
from test_fp8_features_cpu import fp8_adversarial
from test_gpu_half_features import AGGS, KNOB_DEFAULTS, KNOBS, _table, _write_graph, beq, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu
FP8 = [("float8_e4m3fn", torch.float8_e4m3fn), ("float8_e5m2", torch.float8_e5m2)]
NAN_CODES = {"float8_e4m3fn": [0x7F, 0xFF], "float8_e5m2": [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]}


@pytest.fixture
def knobs():
    def set_knobs(**kw):
        for k, v in KNOB_DEFAULTS.items():
            glx.tune(k, kw.get(k, v))
    yield set_knobs
    set_knobs()


def _up(X, tdt):
    """the float32 table of X's values rounded to tdt by torch's CPU conversion (numpy)"""
    return torch.from_numpy(np.ascontiguousarray(X)).to(tdt).float().numpy()


def _pair(X, name, tdt, hashed_ids=None):
    """(FP8 Features converted on upload from float32, float32 Features of the upcast values, upcast numpy table)."""
    up = _up(X, tdt)
    assert not np.isnan(up).any()  # the tables of these tests stay inside both types' range
    ids = None if hashed_ids is None else torch.from_numpy(hashed_ids).cuda()
    f8 = glx.Features(torch.from_numpy(X).cuda(), ids=ids, dtype=name)
    f32 = glx.Features(torch.from_numpy(up).cuda(), ids=None if hashed_ids is None else torch.from_numpy(hashed_ids).cuda())
    assert f8.dtype == name and f32.dtype == "float32"
    return f8, f32, up


def _all_rows(f):
    return f.lookup(torch.arange(f.num_rows, device="cuda"))


def _assert_upcast_of(got, codes, name, tdt):
    """got: float32 lookups; codes: the uint8 codes they must be the upcast of (NaN-ness only at the NaN codes)"""
    codes = codes.reshape(-1)
    want = torch.from_numpy(codes).view(tdt).float().numpy().view(np.uint32)
    g = bits(got).reshape(-1).view(np.uint32)
    nan = np.isin(codes, NAN_CODES[name])
    assert np.array_equal(g[~nan], want[~nan]), name
    assert np.isnan(g[nan].view(np.float32)).all(), name
    assert not np.isnan(g[~nan].view(np.float32)).any(), name


# ---- 1. conversion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("host", [False, True])
def test_upload_conversion_equals_torch(name, tdt, host):
    x = np.concatenate([fp8_adversarial(t)[:-(1 << 20) + 4096] for _, t in FP8])  # 4096 of the random patterns each
    D = 8
    n = (x.shape[0] + D - 1) // D * D
    x = np.concatenate([x, np.zeros(n - x.shape[0], np.float32)]).reshape(-1, D)
    want = torch.from_numpy(x).contiguous().to(tdt)  # what torch's CPU conversion emits
    codes = want.view(torch.uint8).numpy()
    f = glx.Features(torch.from_numpy(x) if host else torch.from_numpy(x).cuda(), dtype=name)
    assert f.dtype == name
    _assert_upcast_of(_all_rows(f), codes, name, tdt)
    # the same FP8 matrix uploaded as it is (x_dtype == store_dtype) stores the same bytes
    g = glx.Features(want if host else want.cuda())
    assert g.dtype == name
    _assert_upcast_of(_all_rows(g), codes, name, tdt)


# ---- 2. upcast ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("how", ["upload", "host", "view"])
def test_upcast_of_every_code(name, tdt, how):
    codes = np.arange(256, dtype=np.uint8).reshape(64, 4)
    t = torch.from_numpy(codes).view(tdt)
    f = glx.Features(t.cuda(), view=True) if how == "view" else glx.Features(t if how == "host" else t.cuda())
    assert f.dtype == name
    got = _all_rows(f)
    _assert_upcast_of(got, codes, name, tdt)
    assert int(torch.isnan(got).sum()) == len(NAN_CODES[name])
    # the scalar path reads the same bytes: one column of the same table
    col = torch.from_numpy(np.arange(256, dtype=np.uint8).reshape(256, 1)).view(tdt)
    _assert_upcast_of(_all_rows(glx.Features(col.cuda())), np.arange(256, dtype=np.uint8), name, tdt)


# ---- 3. lookup ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("ids_kind", ["dense", "hashed", "arith"])
@pytest.mark.parametrize("D", [1, 3, 5, 8, 100, 256])
def test_lookup_equals_upcast_table(name, tdt, ids_kind, D):
    rng = np.random.default_rng(D)
    V = 700
    X = _table(rng, V, D)
    raw = {"dense": None, "hashed": rng.permutation(10 * V)[:V].astype(np.int64) * 7 + 3,
           "arith": (np.arange(V, dtype=np.int64) * 5 + 11)}[ids_kind]
    f8, f32, up = _pair(X, name, tdt, raw)
    known = np.arange(V) if raw is None else raw
    q = np.concatenate([known[rng.integers(0, V, 2000)], np.array([-1, -7, 10 ** 9, 4, 12], np.int64)])
    qt = torch.from_numpy(q).cuda()
    assert beq(f8.lookup(qt, default_attr=-2.5), f32.lookup(qt, default_attr=-2.5)), (name, ids_kind, D)
    assert np.array_equal(f8.lookup(q, default_attr=-2.5).view(np.uint32), f32.lookup(q, default_attr=-2.5).view(np.uint32))


# ---- 4. aggregate, every operator --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [1, 3, 4, 5, 8, 12, 31, 32, 36, 100, 128, 256, 260, 264])
@pytest.mark.parametrize("ids_kind", ["dense", "hashed"])
def test_aggregate_every_operator_equals_oracle(name, tdt, D, ids_kind):
    rng = np.random.default_rng(31 * D + len(ids_kind))
    V = 1500
    X = _table(rng, V, D)
    raw = None if ids_kind == "dense" else rng.permutation(4 * V)[:V].astype(np.int64) * 3 - 5
    f8, f32, up = _pair(X, name, tdt, raw)
    known = np.arange(V) if raw is None else raw
    orc = Oracle()
    # dense response: 700 segments of 10
    Sg, f = 700, 10
    ids = known[rng.integers(0, V, Sg * f)]
    ids[rng.random(Sg * f) < 0.03] = -4  # unknown / negative ids
    ids[rng.random(Sg * f) < 0.03] = 10 ** 9
    h_seg = (np.arange(Sg * f) // f).astype(np.int32)
    # explicit ragged segment_ids with empty segments and one long segment
    Sr = 900
    sizes = rng.integers(0, 9, Sr)
    sizes[[0, 3, Sr - 1]] = 0
    sizes[7] = 200
    r_seg = np.repeat(np.arange(Sr, dtype=np.int32), sizes)
    r_ids = known[rng.integers(0, V, r_seg.shape[0])]
    r_ids[rng.random(r_ids.shape[0]) < 0.05] = -1
    oids = None if raw is None else raw
    for op in AGGS:
        ti = torch.from_numpy(ids).cuda()
        e, c = f8.aggregate(op, ti, None, Sg, default_attr=1.25)
        e32, c32 = f32.aggregate(op, ti, None, Sg, default_attr=1.25)
        oe, oc = orc.aggregate(up, op, ids, h_seg, Sg, 1.25, ids=oids)
        assert beq(e, e32) and torch.equal(c, c32), (name, D, op, "dense")
        assert np.array_equal(bits(e), oe.view(np.int32)) and np.array_equal(c.cpu().numpy(), oc), (name, D, op, "dense oracle")
        e, c = f8.aggregate(op, torch.from_numpy(r_ids).cuda(), torch.from_numpy(r_seg).cuda(), Sr, default_attr=1.25)
        oe, oc = orc.aggregate(up, op, r_ids, r_seg, Sr, 1.25, ids=oids)
        assert np.array_equal(bits(e), oe.view(np.int32)) and np.array_equal(c.cpu().numpy(), oc), (name, D, op, "ragged")
        # host (numpy) pointers take the same kernels
        he, hc = f8.aggregate(op, r_ids, r_seg, Sr, default_attr=1.25)
        assert np.array_equal(he.view(np.int32), oe.view(np.int32)) and np.array_equal(hc, oc), (name, D, op, "host")
        he, hc = f8.aggregate(op, ids, None, Sg, default_attr=1.25)
        assert np.array_equal(he.view(np.int32), bits(e32)) and np.array_equal(hc, c32.cpu().numpy()), (name, D, op, "host dense")


# ---- 5. every knob -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_every_knob_bit_equal(knobs, name, tdt, D):
    rng = np.random.default_rng(5 * D)
    V, Sg, f = 3000, 4099, 10
    X = _table(rng, V, D)
    f8, f32, up = _pair(X, name, tdt)
    ids = torch.from_numpy(rng.integers(-2, V + 2, Sg * f).astype(np.int64)).cuda()
    sizes = rng.integers(0, 14, 1500)
    sizes[[0, 9]] = 0
    r_seg = np.repeat(np.arange(1500, dtype=np.int32), sizes)
    r_ids = torch.from_numpy(rng.integers(-3, V + 3, r_seg.shape[0]).astype(np.int64)).cuda()
    r_seg_t = torch.from_numpy(r_seg).cuda()
    for op in ("SumAggregator", "MeanAggregator", "MaxAggregator"):
        knobs()
        base = f8.aggregate(op, ids, None, Sg, default_attr=1.25)
        base_r = f8.aggregate(op, r_ids, r_seg_t, 1500, default_attr=1.25)
        ref = f32.aggregate(op, ids, None, Sg, default_attr=1.25)
        ref_r = f32.aggregate(op, r_ids, r_seg_t, 1500, default_attr=1.25)
        assert beq(base[0], ref[0]) and torch.equal(base[1], ref[1]), (name, D, op)
        assert beq(base_r[0], ref_r[0]) and torch.equal(base_r[1], ref_r[1]), (name, D, op)
        for s in KNOBS + [dict(agg_half_ld16=2), dict(agg_half_ld16=2, agg_xcd_slices=2)]:  # 2: 4 columns per lane
            knobs(**s)
            e, c = f8.aggregate(op, ids, None, Sg, default_attr=1.25)
            assert beq(e, base[0]) and torch.equal(c, base[1]), (name, D, op, s)
            e, c = f8.aggregate(op, r_ids, r_seg_t, 1500, default_attr=1.25)
            assert beq(e, base_r[0]) and torch.equal(c, base_r[1]), (name, D, op, s, "ragged")


# ---- 6. full size --------------------------------------------------------------------------------------------------
def test_full_size_request_takes_stripes_bit_identical(knobs):
    """(4 << 20) + 130 ids at D = 256: the stripe / XCD path engages by default; same bits as the float32 upcast table."""
    rng = np.random.default_rng(11)
    V, f, D = 100_000, 10, 256
    Sg = (4 << 20) // f + 13
    ids = torch.from_numpy(rng.integers(-2, V + 2, Sg * f).astype(np.int64)).cuda()
    X = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32))
    f8 = glx.Features(X.cuda(), dtype="float8_e4m3fn")
    f32 = glx.Features(X.to(torch.float8_e4m3fn).float().cuda())
    knobs()
    e, c = f8.aggregate("MaxAggregator", ids, None, Sg)
    e32, c32 = f32.aggregate("MaxAggregator", ids, None, Sg)
    torch.cuda.synchronize()
    assert torch.equal(e.view(torch.int32), e32.view(torch.int32)) and torch.equal(c, c32)
    del e, c, e32, c32, f8, f32
    torch.cuda.empty_cache()


# ---- 7. misaligned views ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("offset,D", [(0, 128), (1, 128), (2, 128), (3, 128), (4, 128), (0, 127), (4, 129), (8, 130)])
def test_views_at_every_byte_offset_and_odd_pitch(name, tdt, offset, D):
    """A view's base is the caller's and its pitch is its dim: a base off by 1-3 bytes or a pitch that is no multiple
    of 4 bytes is where a 4-column load would be misaligned."""
    rng = np.random.default_rng(100 * offset + D)
    V = 1000
    Xq = torch.from_numpy(_table(rng, V, D)).to(tdt)
    buf = torch.zeros(V * D + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + V * D] = Xq.view(torch.uint8).reshape(-1).cuda()
    Xv = buf[offset:offset + V * D].view(tdt).view(V, D)
    assert Xv.data_ptr() % 4 == offset % 4 and Xv.is_contiguous()
    v = glx.Features(Xv, view=True)
    assert v.dtype == name
    f32 = glx.Features(Xq.float().cuda())
    ids = torch.from_numpy(rng.integers(-1, V + 1, 5000).astype(np.int64)).cuda()
    assert beq(v.lookup(ids, default_attr=0.5), f32.lookup(ids, default_attr=0.5))
    for op in AGGS:
        e, c = v.aggregate(op, ids, None, 500)
        e32, c32 = f32.aggregate(op, ids, None, 500)
        assert beq(e, e32) and torch.equal(c, c32), op
    for op in ("MaxAggregator", "MinAggregator"):
        assert all(torch.equal(a, b) for a, b in zip(v.aggregate_arg(op, ids, None, 500), f32.aggregate_arg(op, ids, None, 500))), op
    with pytest.raises(ValueError):
        glx.Features(Xv, view=True, dtype="float32")


# ---- 8. aggregate_arg ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [8, 256])
def test_aggregate_arg_equals_upcast_table(name, tdt, D):
    rng = np.random.default_rng(7 * D)
    V = 1200
    f8, f32, up = _pair(_table(rng, V, D), name, tdt)
    ids = torch.from_numpy(rng.integers(-2, V + 2, 300 * 10).astype(np.int64)).cuda()
    sizes = rng.integers(0, 9, 400)
    sizes[[0, 5]] = 0
    r_seg = torch.from_numpy(np.repeat(np.arange(400, dtype=np.int32), sizes)).cuda()
    r_ids = torch.from_numpy(rng.integers(-2, V + 2, int(sizes.sum())).astype(np.int64)).cuda()
    for op in ("MaxAggregator", "MinAggregator"):
        for req in ((ids, None, 300), (r_ids, r_seg, 400)):
            e, c, a = f8.aggregate_arg(op, *req, default_attr=1.25)
            e32, c32, a32 = f32.aggregate_arg(op, *req, default_attr=1.25)
            assert beq(e, e32) and torch.equal(c, c32) and torch.equal(a, a32), (name, D, op)
            assert beq(e, f8.aggregate(op, *req, default_attr=1.25)[0]), (name, D, op)


# ---- 9. plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", FP8)
def test_plan_with_fp8_tables_equals_float32_plan(name, tdt):
    import synth
    V, D = 3000, 256
    rp, col, eid, w = synth.small_graph(V, 40000, seed=9, weighted=True, hub_degree=1000)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    g = glx.Graph(t(rp), t(col), t(eid), t(w))
    X = np.random.default_rng(3).standard_normal((V, D)).astype(np.float32)
    f8 = glx.Features(t(X), dtype=name)
    f32 = glx.Features(t(_up(X, tdt)))
    for agg in ("MeanAggregator", "MaxAggregator"):
        p8 = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[f8, f8], agg=agg, seed=5)
        p32 = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[f32, f32], agg=agg, seed=5)
        rng = np.random.default_rng(1)
        for run in range(2):
            seeds = t(rng.integers(0, V, 512).astype(np.int64))
            a = p8.run(seeds, call_counter=10 * run)
            a = [{k: v.clone() for k, v in h.items()} for h in a]
            b = p32.run(seeds, call_counter=10 * run)
            torch.cuda.synchronize()
            for h in range(2):
                assert a[h]["emb"].dtype == torch.float32
                assert torch.equal(a[h]["cnt"], b[h]["cnt"]), (agg, run, h)
                assert torch.equal(a[h]["emb"].view(torch.int32), b[h]["emb"].view(torch.int32)), (agg, run, h)
        p8.close()
        p32.close()


# ---- 10. KNN ---------------------------------------------------------------------------------------------------------
def _same_answer(a, b):
    return torch.equal(a[0], b[0]) and beq(a[1], b[1])


@pytest.mark.parametrize("name,tdt", FP8)
@pytest.mark.parametrize("D", [7, 128])
def test_exact_search_equals_upcast_table(name, tdt, D):
    rng = np.random.default_rng(13 * D)
    N = 1003
    f8, f32, up = _pair(_table(rng, N, D), name, tdt)
    for nq in (5, 130):  # 130 crosses the 128-query tile
        q = torch.from_numpy(rng.standard_normal((nq, D)).astype(np.float32)).cuda()
        for k in (1, 20):
            for metric in ("ip", "l2"):
                assert _same_answer(f8.search(q, k, metric), f32.search(q, k, metric)), (name, D, nq, k, metric)
    # a view builds its row norms per search: the same answer
    v = glx.Features(torch.from_numpy(up).to(tdt).cuda(), view=True)
    assert _same_answer(v.search(q, 20, "l2"), f32.search(q, 20, "l2"))


@pytest.mark.parametrize("name,tdt", FP8)
def test_ivf_indexes_equal_those_of_the_upcast_table(name, tdt):
    rng = np.random.default_rng(17)
    N, D = 1003, 128
    f8, f32, up = _pair(_table(rng, N, D), name, tdt)
    q = torch.from_numpy(rng.standard_normal((130, D)).astype(np.float32)).cuda()
    with f8.build_ivf(nlist=8) as i8, f32.build_ivf(nlist=8) as i32:
        assert np.array_equal(i8.centroids().view(np.uint32), i32.centroids().view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(i8.lists(), i32.lists()))
        for metric in ("ip", "l2"):
            for k in (1, 20):
                for nprobe in (1, 8):
                    assert _same_answer(i8.search(q, k, metric, nprobe=nprobe), i32.search(q, k, metric, nprobe=nprobe)), (
                        name, metric, k, nprobe)
                assert _same_answer(i8.search(q, k, metric, nprobe=8), f8.search(q, k, metric)), (name, metric, k)
    with f8.build_ivfpq(nlist=8, m=8) as p8, f32.build_ivfpq(nlist=8, m=8) as p32:
        assert np.array_equal(p8.ivf.centroids().view(np.uint32), p32.ivf.centroids().view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(p8.ivf.lists(), p32.ivf.lists()))
        assert np.array_equal(p8.codebooks().view(np.uint32), p32.codebooks().view(np.uint32))
        assert np.array_equal(p8.codes(), p32.codes())
        for metric in ("ip", "l2"):
            for k in (1, 20):
                for nprobe in (1, 8):
                    for refine in (0, 20):
                        assert _same_answer(p8.search(q, k, metric, nprobe=nprobe, refine=refine),
                                            p32.search(q, k, metric, nprobe=nprobe, refine=refine)), (name, metric, k, nprobe, refine)


# ---- 11. refusals ------------------------------------------------------------------------------------------------------
def test_what_refuses_fp8_names_the_dtype():
    L = glx.lib()
    comm = ctypes.c_void_p()
    assert L.glx_comm_init_local(0x4A1F0029, 0, 0, 1, ctypes.byref(comm)) == 0
    try:
        for name, tdt in FP8:
            f = glx.Features(torch.zeros((4, 8), device="cuda"), dtype=name)
            st = ctypes.c_void_p()
            assert L.glx_dist_store_create(comm, None, f._h, ctypes.byref(st)) == 3 and not st.value
            assert name.encode() in L.glx_last_error()
    finally:
        L.glx_comm_destroy(comm)
    from graphlearn.nn.pytorch.segment import segment_aggregate
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    for name, tdt in FP8:
        x8 = torch.zeros((4, 8), device="cuda").to(tdt)
        with pytest.raises(ValueError, match=name):  # the training path takes float32 matrices only
            segment_aggregate(x8, idx, 2, op="sum")
        with pytest.raises(ValueError, match=name):
            glx.Features(x8, dtype="bfloat16")
        with pytest.raises(ValueError, match=name):
            glx.Features(x8.cpu(), dtype="float32")
        with pytest.raises(ValueError):
            glx.Features(x8, view=True, dtype="float8_e5m2" if name == "float8_e4m3fn" else "float8_e4m3fn")


# ---- 12. Python end to end ---------------------------------------------------------------------------------------------
def test_python_end_to_end_e4m3(tmp_path):
    import graphlearn as gl
    from graphlearn import settings
    rng = np.random.default_rng(4)
    V, D = 120, 4
    X = (rng.standard_normal((V, D)) * 3).astype(np.float32)
    Xr = _up(X, torch.float8_e4m3fn)
    d = str(tmp_path)
    n1, e1 = _write_graph(d, X, "raw")
    n2, e2 = _write_graph(d, Xr, "rounded")

    def make(n, e):
        return gl.Graph().node(n, "entity", gl.Decoder(attr_types=["float"] * D, labeled=True)) \
            .edge(e, ("entity", "entity", "relation"), gl.Decoder(weighted=True), directed=False).init()

    with pytest.raises(ValueError):
        settings.set_feature_dtype("float8")
    settings.set_feature_dtype("float8_e4m3fn")
    try:
        g8 = make(n1, e1)
    finally:
        settings.set_feature_dtype("float32")
    g32 = make(n2, e2)
    try:
        assert g8.device_features("entity").dtype == "float8_e4m3fn"
        assert g32.device_features("entity").dtype == "float32"
        ids = np.array([[1, 2, 3], [10, 20, 119], [7, 7, 500]])
        for func in ("sum", "mean", "max", "min", "prod"):
            a = g8.get_nodes("entity", ids).embedding_agg(func)
            b = g32.get_nodes("entity", ids).embedding_agg(func)
            assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)), func
        q = np.array([0, 5, 119, 300, 64])
        a, b = g8.lookup_nodes("entity", q).float_attrs, g32.lookup_nodes("entity", q).float_attrs
        assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
        la = list(gl.NeighborLoader(g8, "entity", ["relation", "relation"], [4, 3], batch_size=32, shuffle=True))
        lb = list(gl.NeighborLoader(g32, "entity", ["relation", "relation"], [4, 3], batch_size=32, shuffle=True))
        assert len(la) == len(lb) == 4
        for ba, bb in zip(la, lb):
            assert torch.equal(ba.seeds, bb.seeds)
            for h in range(3):
                assert ba.x[h].dtype == torch.float32
                assert torch.equal(ba.x[h].view(torch.int32), bb.x[h].view(torch.int32)), h
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            g8.sharded_store("relation", "entity")
    finally:
        g8.close()
        g32.close()
