"""GPU tests of half-precision feature tables (GLX_DTYPE_BF16 / GLX_DTYPE_F16): bfloat16 or float16 storage,
float32 accumulation.  The upload's float32 -> half conversion must equal torch's bit for bit; every aggregation
and lookup of a half table must equal -- bit for bit -- the same call on the float32 table of its upcast values (and
so the oracle on that table), for every kernel shape and knob the launcher can select."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import glx
from oracle_bindings import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu
HALF = [("bfloat16", torch.bfloat16), ("float16", torch.float16)]
AGGS = ["SumAggregator", "MeanAggregator", "MaxAggregator", "MinAggregator", "ProdAggregator"]
KNOB_DEFAULTS = dict(agg_xcd_slices=0, agg_xcd_stripes=-1, agg_xcd_chunk=0, agg_segs=0, agg_unroll=0, agg_store=0,
                     agg_legacy=0, agg_mfma=0, agg_half_ld16=0)
# the XCD-stripe test's sweep (tests/test_gpu_agg_xcd_stripes.py SETTINGS) plus the other knobs of the reduce
KNOBS = [dict(), dict(agg_xcd_stripes=0), dict(agg_xcd_stripes=1)] + [
    dict(agg_xcd_stripes=1, agg_xcd_slices=n, agg_xcd_chunk=c) for n in (1, 2, 4) for c in (1, 3, 64)] + [
    dict(agg_xcd_stripes=1, agg_xcd_slices=n, agg_xcd_chunk=c, agg_segs=3) for n in (1, 2) for c in (1, 3)] + [
    dict(agg_xcd_stripes=1, agg_xcd_slices=8, agg_xcd_chunk=1)] + [
    dict(agg_unroll=u) for u in (6, 8, 10, 12, 15)] + [
    dict(agg_store=1), dict(agg_legacy=1), dict(agg_mfma=1), dict(agg_half_ld16=1), dict(agg_half_ld16=1, agg_xcd_slices=2)]


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def beq(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture
def knobs():
    def set_knobs(**kw):
        for k, v in KNOB_DEFAULTS.items():
            glx.tune(k, kw.get(k, v))
    yield set_knobs
    set_knobs()


def _table(rng, V, D):
    """float32 values that are NOT representable in either half type (so the rounding matters), some below Max's -37
    initialiser, plus exact zeros and ones."""
    X = (rng.standard_normal((V, D)) * 3).astype(np.float32)
    X[rng.random((V, D)) < 0.02] = -50.3
    X[rng.random((V, D)) < 0.01] = 0.0
    X[rng.random((V, D)) < 0.01] = 1.0
    return X


def _pair(X, tdt, hashed_ids=None, host=False):
    """(half Features converted on upload from float32, float32 Features of the upcast values, upcast numpy table)."""
    up = torch.from_numpy(X).to(tdt).float().numpy()
    name = "bfloat16" if tdt == torch.bfloat16 else "float16"
    src = torch.from_numpy(X) if host else torch.from_numpy(X).cuda()
    ids = None if hashed_ids is None else (hashed_ids if host else torch.from_numpy(hashed_ids).cuda())
    fh = glx.Features(src, ids=ids if not host else hashed_ids, dtype=name)
    f32 = glx.Features(torch.from_numpy(up).cuda(), ids=None if hashed_ids is None else torch.from_numpy(hashed_ids).cuda())
    assert fh.dtype == name and f32.dtype == "float32"
    return fh, f32, up


# ---- 1. conversion ---------------------------------------------------------------------------------------------
def _adversarial():
    f32 = np.finfo(np.float32)
    vals = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, f32.max, f32.min, f32.tiny, -f32.tiny, f32.smallest_subnormal,
            65504.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e5, -1e5, 6.1035156e-05, 5.9604645e-08, 2.9802322e-08,
            2.9802326e-08, 8.940697e-08, 1e-40, -1e-40, 3.0e38]
    u = [0x3F808000, 0x3F818000, 0x3F808001, 0xBF808000, 0x3F801000, 0x3F803000, 0x3F802000,  # bf16 / fp16 ties
         0x00800000, 0x00400000, 0x007FFFFF, 0x80000001, 0x33000000, 0x33000001, 0x337FFFFF, 0x387FC000, 0x387FE000,
         0x38800000, 0x477FEFFF, 0x477FF000, 0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0xFF7FFFFF,
         0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000, 0x7FC12345]
    x = np.concatenate([np.array(vals, np.float32), np.array(u, np.uint32).view(np.float32)])
    x = np.concatenate([x, np.float32(np.nan) * np.ones(2, np.float32), -np.abs(np.float32(np.nan)) * np.ones(2, np.float32)])
    rng = np.random.default_rng(0)
    rnd = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([x, rnd])


@pytest.mark.parametrize("name,tdt", HALF)
@pytest.mark.parametrize("host", [False, True])
def test_upload_conversion_equals_torch(name, tdt, host):
    x = _adversarial()
    D = 8
    n = (x.shape[0] + D - 1) // D * D
    x = np.concatenate([x, np.zeros(n - x.shape[0], np.float32)]).reshape(-1, D)
    want = torch.from_numpy(x).contiguous().to(tdt)  # what torch's CPU conversion emits, NaNs included
    f = glx.Features(torch.from_numpy(x) if host else torch.from_numpy(x).cuda(), dtype=name)
    assert f.dtype == name
    got = f.lookup(torch.arange(x.shape[0], device="cuda"))
    # the lookup upcasts: compare the upcast bits (exact) -- and NaN bits survive the upcast unchanged
    assert beq(got, want.float()), name
    # the same half matrix uploaded as is (x_dtype == store_dtype) stores the same bits
    g = glx.Features(want.cuda())
    assert g.dtype == name and beq(g.lookup(torch.arange(x.shape[0], device="cuda")), want.float())


# ---- 2. lookup ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", HALF)
@pytest.mark.parametrize("ids_kind", ["dense", "hashed", "arith"])
@pytest.mark.parametrize("D", [3, 8, 100, 256])
def test_lookup_equals_upcast_table(name, tdt, ids_kind, D):
    rng = np.random.default_rng(D)
    V = 700
    X = _table(rng, V, D)
    raw = {"dense": None, "hashed": rng.permutation(10 * V)[:V].astype(np.int64) * 7 + 3,
           "arith": (np.arange(V, dtype=np.int64) * 5 + 11)}[ids_kind]
    fh, f32, up = _pair(X, tdt, raw)
    known = np.arange(V) if raw is None else raw
    q = np.concatenate([known[rng.integers(0, V, 2000)], np.array([-1, -7, 10 ** 9, 4, 12], np.int64)])
    qt = torch.from_numpy(q).cuda()
    assert beq(fh.lookup(qt, default_attr=-2.5), f32.lookup(qt, default_attr=-2.5)), (name, ids_kind, D)
    assert np.array_equal(fh.lookup(q, default_attr=-2.5).view(np.uint32), f32.lookup(q, default_attr=-2.5).view(np.uint32))


# ---- 3. aggregate, every operator --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", HALF)
@pytest.mark.parametrize("D", [1, 3, 8, 12, 100, 128, 256, 264])
@pytest.mark.parametrize("ids_kind", ["dense", "hashed"])
def test_aggregate_every_operator_equals_oracle(name, tdt, D, ids_kind):
    rng = np.random.default_rng(31 * D + len(ids_kind))
    V = 1500
    X = _table(rng, V, D)
    raw = None if ids_kind == "dense" else rng.permutation(4 * V)[:V].astype(np.int64) * 3 - 5
    fh, f32, up = _pair(X, tdt, raw)
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
        e, c = fh.aggregate(op, ti, None, Sg, default_attr=1.25)
        e32, c32 = f32.aggregate(op, ti, None, Sg, default_attr=1.25)
        oe, oc = orc.aggregate(up, op, ids, h_seg, Sg, 1.25, ids=oids)
        assert beq(e, e32) and torch.equal(c, c32), (name, D, op, "dense")
        assert np.array_equal(bits(e), oe.view(np.int32)) and np.array_equal(c.cpu().numpy(), oc), (name, D, op, "dense oracle")
        e, c = fh.aggregate(op, torch.from_numpy(r_ids).cuda(), torch.from_numpy(r_seg).cuda(), Sr, default_attr=1.25)
        oe, oc = orc.aggregate(up, op, r_ids, r_seg, Sr, 1.25, ids=oids)
        assert np.array_equal(bits(e), oe.view(np.int32)) and np.array_equal(c.cpu().numpy(), oc), (name, D, op, "ragged")
        # host (numpy) pointers take the same kernels
        he, hc = fh.aggregate(op, r_ids, r_seg, Sr, default_attr=1.25)
        assert np.array_equal(he.view(np.int32), oe.view(np.int32)) and np.array_equal(hc, oc), (name, D, op, "host")


# ---- 4. every knob -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", HALF)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_every_knob_bit_equal(knobs, name, tdt, D):
    rng = np.random.default_rng(5 * D)
    V, Sg, f = 3000, 4099, 10
    X = _table(rng, V, D)
    fh, f32, up = _pair(X, tdt)
    ids = torch.from_numpy(rng.integers(-2, V + 2, Sg * f).astype(np.int64)).cuda()
    sizes = rng.integers(0, 14, 1500)
    sizes[[0, 9]] = 0
    r_seg = np.repeat(np.arange(1500, dtype=np.int32), sizes)
    r_ids = torch.from_numpy(rng.integers(-3, V + 3, r_seg.shape[0]).astype(np.int64)).cuda()
    r_seg_t = torch.from_numpy(r_seg).cuda()
    for op in ("SumAggregator", "MeanAggregator", "MaxAggregator"):
        knobs()
        base = fh.aggregate(op, ids, None, Sg, default_attr=1.25)
        base_r = fh.aggregate(op, r_ids, r_seg_t, 1500, default_attr=1.25)
        ref = f32.aggregate(op, ids, None, Sg, default_attr=1.25)
        ref_r = f32.aggregate(op, r_ids, r_seg_t, 1500, default_attr=1.25)
        assert beq(base[0], ref[0]) and torch.equal(base[1], ref[1]), (name, D, op)
        assert beq(base_r[0], ref_r[0]) and torch.equal(base_r[1], ref_r[1]), (name, D, op)
        for s in KNOBS:
            knobs(**s)
            e, c = fh.aggregate(op, ids, None, Sg, default_attr=1.25)
            assert beq(e, base[0]) and torch.equal(c, base[1]), (name, D, op, s)
            e, c = fh.aggregate(op, r_ids, r_seg_t, 1500, default_attr=1.25)
            assert beq(e, base_r[0]) and torch.equal(c, base_r[1]), (name, D, op, s, "ragged")


# ---- 5. full size --------------------------------------------------------------------------------------------------
def test_full_size_request_takes_stripes_bit_identical(knobs):
    """>= 4 M ids at D = 256: the stripe / XCD path engages by default; same bits as the float32 upcast table."""
    rng = np.random.default_rng(11)
    V, f, D = 100_000, 10, 256
    Sg = (4 << 20) // f + 13
    ids = torch.from_numpy(rng.integers(-2, V + 2, Sg * f).astype(np.int64)).cuda()
    X = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).cuda()
    for tdt, name in ((torch.bfloat16, "bfloat16"), (torch.float16, "float16")):
        fh = glx.Features(X, dtype=name)
        f32 = glx.Features(X.to(tdt).float())
        knobs()
        e, c = fh.aggregate("MaxAggregator", ids, None, Sg)
        e32, c32 = f32.aggregate("MaxAggregator", ids, None, Sg)
        torch.cuda.synchronize()
        assert torch.equal(e.view(torch.int32), e32.view(torch.int32)) and torch.equal(c, c32), name
        del e, c, e32, c32, fh, f32
        torch.cuda.empty_cache()


# ---- 6. plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", HALF)
def test_plan_with_half_tables_equals_float32_plan(name, tdt):
    import synth
    V, D = 3000, 256
    rp, col, eid, w = synth.small_graph(V, 40000, seed=9, weighted=True, hub_degree=1000)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    g = glx.Graph(t(rp), t(col), t(eid), t(w))
    X = np.random.default_rng(3).standard_normal((V, D)).astype(np.float32)
    fh = glx.Features(t(X), dtype=name)
    f32 = glx.Features(t(X).to(tdt).float())
    for agg in ("MeanAggregator", "MaxAggregator"):
        ph = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[fh, fh], agg=agg, seed=5)
        p32 = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[f32, f32], agg=agg, seed=5)
        rng = np.random.default_rng(1)
        for run in range(2):
            seeds = t(rng.integers(0, V, 512).astype(np.int64))
            a = ph.run(seeds, call_counter=10 * run)
            a = [{k: v.clone() for k, v in h.items()} for h in a]
            b = p32.run(seeds, call_counter=10 * run)
            torch.cuda.synchronize()
            for h in range(2):
                assert a[h]["emb"].dtype == torch.float32
                assert torch.equal(a[h]["cnt"], b[h]["cnt"]), (agg, run, h)
                assert torch.equal(a[h]["emb"].view(torch.int32), b[h]["emb"].view(torch.int32)), (agg, run, h)
        ph.close()
        p32.close()


# ---- 7. views ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", HALF)
def test_view_of_a_half_cuda_tensor(name, tdt):
    rng = np.random.default_rng(2)
    V, D = 1000, 128
    Xh = torch.from_numpy(_table(rng, V, D)).cuda().to(tdt)
    v = glx.Features(Xh, view=True)
    assert v.dtype == name
    f32 = glx.Features(Xh.float())
    ids = torch.from_numpy(rng.integers(-1, V + 1, 5000).astype(np.int64)).cuda()
    assert beq(v.lookup(ids), f32.lookup(ids))
    for op in AGGS:
        assert beq(v.aggregate(op, ids, None, 500)[0], f32.aggregate(op, ids, None, 500)[0]), op
    with pytest.raises(ValueError):
        glx.Features(Xh, view=True, dtype="float32")


# ---- 8. invalid input --------------------------------------------------------------------------------------------------
def test_invalid_pairs_and_distributed_store_refuse():
    L = glx.lib()
    x = np.zeros((4, 8), np.float32)
    h = ctypes.c_void_p()
    for xd, sd in ((1, 0), (2, 0), (1, 2), (2, 1), (3, 0), (0, 3), (-1, -1)):
        rc = L.glx_features_create_ex(0, 4, 8, x.ctypes.data, xd, sd, None, glx.PTR_HOST, None, ctypes.byref(h))
        assert rc == 3 and not h.value, (xd, sd)
    assert L.glx_features_view_ex(0, 4, 8, ctypes.c_void_p(16), 5, ctypes.byref(h)) == 3
    # a distributed store over a half table: GLX_INVALID_ARGUMENT naming the dtype
    comm = ctypes.c_void_p()
    assert L.glx_comm_init_local(0x4A1F0008, 0, 0, 1, ctypes.byref(comm)) == 0
    try:
        for name in ("bfloat16", "float16"):
            f = glx.Features(torch.zeros((4, 8), device="cuda"), dtype=name)
            st = ctypes.c_void_p()
            assert L.glx_dist_store_create(comm, None, f._h, ctypes.byref(st)) == 3 and not st.value
            assert name.encode() in L.glx_last_error()
        f = glx.Features(torch.zeros((4, 8), device="cuda"))
        st = ctypes.c_void_p()
        assert L.glx_dist_store_create(comm, None, f._h, ctypes.byref(st)) == 0
        L.glx_dist_store_destroy(st)
    finally:
        L.glx_comm_destroy(comm)


# ---- 9. Python end to end ----------------------------------------------------------------------------------------------
def _write_graph(d, X, tag):
    nodes = os.path.join(d, "ent_%s" % tag)
    with open(nodes, "w") as fo:
        fo.write("id:int64\tlabel:int64\tfeature:string\n")
        for v in range(X.shape[0]):
            fo.write("%d\t%d\t%s\n" % (v, v, ":".join("%.9g" % a for a in X[v])))
    edges = os.path.join(d, "rel_%s" % tag)
    with open(edges, "w") as fo:
        fo.write("src_id:int64\tdst_id:int64\tweight:float\n")
        for i in range(X.shape[0] - 5):
            for step in (2, 3, 5):
                fo.write("%d\t%d\t%f\n" % (i, i + step, (i + 1) / 100.0))
    return nodes, edges


def test_python_end_to_end_bfloat16(tmp_path):
    import graphlearn as gl
    from graphlearn import settings
    rng = np.random.default_rng(4)
    V, D = 120, 4
    X = (rng.standard_normal((V, D)) * 3).astype(np.float32)
    Xr = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    d = str(tmp_path)
    n1, e1 = _write_graph(d, X, "raw")
    n2, e2 = _write_graph(d, Xr, "rounded")

    def make(n, e):
        return gl.Graph().node(n, "entity", gl.Decoder(attr_types=["float"] * D, labeled=True)) \
            .edge(e, ("entity", "entity", "relation"), gl.Decoder(weighted=True), directed=False).init()

    with pytest.raises(ValueError):
        settings.set_feature_dtype("half")
    settings.set_feature_dtype("bfloat16")
    try:
        gh = make(n1, e1)
    finally:
        settings.set_feature_dtype("float32")
    g32 = make(n2, e2)
    try:
        assert gh.device_features("entity").dtype == "bfloat16"
        assert g32.device_features("entity").dtype == "float32"
        ids = np.array([[1, 2, 3], [10, 20, 119], [7, 7, 500]])
        for func in ("sum", "mean", "max", "min", "prod"):
            a = gh.get_nodes("entity", ids).embedding_agg(func)
            b = g32.get_nodes("entity", ids).embedding_agg(func)
            assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)), func
        q = np.array([0, 5, 119, 300, 64])
        a, b = gh.lookup_nodes("entity", q).float_attrs, g32.lookup_nodes("entity", q).float_attrs
        assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
        la = list(gl.NeighborLoader(gh, "entity", ["relation", "relation"], [4, 3], batch_size=32, shuffle=True))
        lb = list(gl.NeighborLoader(g32, "entity", ["relation", "relation"], [4, 3], batch_size=32, shuffle=True))
        assert len(la) == len(lb) == 4
        for ba, bb in zip(la, lb):
            assert torch.equal(ba.seeds, bb.seeds)
            for h in range(3):
                assert ba.x[h].dtype == torch.float32
                assert torch.equal(ba.x[h].view(torch.int32), bb.x[h].view(torch.int32)), h
        with pytest.raises(ValueError, match="bfloat16"):
            gh.sharded_store("relation", "entity")
    finally:
        gh.close()
        g32.close()
