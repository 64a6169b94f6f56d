"""GPU tests of the aggregation reduce and the lookup on NaN, inf, signed-zero, subnormal and overflowing rows
(tests/agg_special_values.py): every kernel the launcher can select -- legacy, grouped, XCD stripes and slices, the
MFMA ablation, the 3-source distributed reduce, the stitch, captured plans -- against the oracle and, on the golden
cases, against the reference's own answers (tests/golden/agg_special.npz).

Comparison (agg_special_values.mismatch): non-NaN elements bit for bit, sign of zero included; NaN positions exactly;
NaN payloads only where the output is a move -- the lookup, default_attr fills, whatever Max / Min select."""
import os
import threading

import numpy as np
import pytest
import torch

import agg_special_values as sv
import glx
from oracle_bindings import AGGREGATORS, Oracle
from test_gpu_half_features import KNOB_DEFAULTS, KNOBS

pytestmark = pytest.mark.gpu
ORC = Oracle()
DTYPES = [("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16)]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_special.npz")


@pytest.fixture
def knobs():
    def set_knobs(**kw):
        for k, v in KNOB_DEFAULTS.items():
            glx.tune(k, kw.get(k, v))
    set_knobs()
    yield set_knobs
    set_knobs()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


def _check(got, want, op, label):
    e, c = _np(got[0]), _np(got[1])
    we, wc = want
    assert np.array_equal(c, wc), (label, op, "counts")
    m = sv.mismatch(e, we, op, wc)
    assert not m, "%s %s\n%s" % (label, op, m)


def _upcast(X, tdt):
    return X if tdt == torch.float32 else sv.half_upcast(X, "bfloat16" if tdt == torch.bfloat16 else "float16")


def _requests(ids, seg, Sg):
    """The ragged request of build_case, and dense ones (segment_ids None) of fanout 1, 3 and 10 made from it."""
    sizes = np.bincount(seg, minlength=Sg)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    reqs = [("ragged", ids, seg, Sg)]
    three = [ids[starts[s]:starts[s + 1]] for s in range(Sg) if sizes[s] == 3]
    for f, stream in ((1, ids), (3, np.concatenate(three)), (10, ids)):
        n = stream.shape[0] // f
        reqs.append(("dense f%d" % f, stream[:n * f].copy(), None, n))
    return reqs


def _want(cache, up, op, ids, seg, Sg, d, raw=None):
    key = (op, id(ids))
    if key not in cache:
        s = seg if seg is not None else (np.arange(ids.shape[0]) // max(1, ids.shape[0] // max(Sg, 1))).astype(np.int32)
        cache[key] = ORC.aggregate(up, op, ids, s, Sg, float(d), ids=raw)
    return cache[key]


# ---- 1. every kernel shape and knob, every storage type --------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 8, 64, 128, 256, 264])
def test_every_knob_equals_oracle(knobs, name, tdt, D):
    d = sv.DEFAULTS[D % len(sv.DEFAULTS)]
    X, ids, seg, Sg, d = sv.build_case(D, 7 * D + len(name), d)
    up = _upcast(X, tdt)
    f = glx.Features(torch.from_numpy(X).cuda(), dtype=name)
    assert f.dtype == name
    reqs = [(label, torch.from_numpy(i).cuda(), None if s is None else torch.from_numpy(s).cuda(), n, i, s)
            for label, i, s, n in _requests(ids, seg, Sg)]
    settings = KNOBS if D >= 32 else [dict(), dict(agg_legacy=1), dict(agg_mfma=1)]
    cache = {}
    for s in settings:
        knobs(**s)
        for op in AGGREGATORS:
            for label, ti, ts, n, hi, hs in reqs:
                got = f.aggregate(op, ti, ts, n, default_attr=float(d))
                _check(got, _want(cache, up, op, hi, hs, n, d), op, (name, D, label, s))


# ---- 2. hashed ids, host pointers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", DTYPES)
@pytest.mark.parametrize("D", [3, 8, 128, 264])
def test_hashed_ids_and_host_pointers(name, tdt, D):
    for k, d in enumerate(sv.DEFAULTS):
        X, ids, seg, Sg, d = sv.build_case(D, 100 + D + k, d, blocks=1)
        up = _upcast(X, tdt)
        raw = np.arange(X.shape[0], dtype=np.int64) * 5 - 17
        req = np.where((ids >= 0) & (ids < X.shape[0]), ids * 5 - 17, ids)
        fd = glx.Features(torch.from_numpy(X).cuda(), ids=torch.from_numpy(raw).cuda(), dtype=name)
        fh = glx.Features(torch.from_numpy(X), ids=raw, dtype=name)  # host matrix and ids: the host staging path
        for op in AGGREGATORS:
            want = ORC.aggregate(up, op, req, seg, Sg, float(d), ids=raw)
            _check(fd.aggregate(op, torch.from_numpy(req).cuda(), torch.from_numpy(seg).cuda(), Sg, default_attr=float(d)),
                   want, op, (name, D, d, "device"))
            _check(fh.aggregate(op, req, seg, Sg, default_attr=float(d)), want, op, (name, D, d, "host"))


# ---- 3. the reference's own answers ----------------------------------------------------------------------------------
def test_golden_cases_equal_the_reference(knobs):
    g = np.load(GOLD)
    for c in range(int(g["num_cases"])):
        X, ids, seg = g["c%d_X" % c], g["c%d_ids" % c], g["c%d_seg" % c]
        Sg, d = int(g["c%d_num_segments" % c]), float(g["c%d_default" % c])
        f = glx.Features(torch.from_numpy(X).cuda())
        ti, ts = torch.from_numpy(ids).cuda(), torch.from_numpy(seg).cuda()
        for s in (dict(), dict(agg_legacy=1)):
            knobs(**s)
            for op in AGGREGATORS:
                want = (g["c%d_%s_emb" % (c, op)], g["c%d_%s_cnt" % (c, op)])
                _check(f.aggregate(op, ti, ts, Sg, default_attr=d), want, op, ("golden", c, s, "device"))
                _check(f.aggregate(op, ids, seg, Sg, default_attr=d), want, op, ("golden", c, s, "host"))


# ---- 4. the MFMA ablation: one non-finite element must not reach the other 15 segments of its workgroup ------------
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("fanout", [1, 3, 4, 10, 25])
@pytest.mark.parametrize("op", ["SumAggregator", "MeanAggregator"])
def test_mfma_nonfinite_stays_in_its_segment(knobs, D, fanout, op):
    rng = np.random.default_rng(D * 31 + fanout)
    V, Sg = 600, 16 * 5 + 7
    X = rng.standard_normal((V, D)).astype(np.float32)
    X[V - 2] = 1.0
    X[V - 2, 5] = np.inf
    X[V - 1] = 2.0
    X[V - 1, D - 3] = sv.NAN[2]
    ids = rng.integers(0, V - 2, Sg * fanout).astype(np.int64)
    target = 16 * 2 + 9  # segment 9 of the third 16-segment block
    ids[target * fanout] = V - 2  # the inf row first ...
    if fanout > 1:
        ids[target * fanout + fanout - 1] = V - 1  # ... and the NaN row last
        targets = [target]
    else:
        ids[target + 16] = V - 1  # ... and the NaN row in a segment of the next block
        targets = [target, target + 16]
    seg = (np.arange(Sg * fanout) // fanout).astype(np.int32)
    f = glx.Features(torch.from_numpy(X).cuda())
    knobs(agg_mfma=1)
    e, c = f.aggregate(op, torch.from_numpy(ids).cuda(), None, Sg, default_attr=0.5)
    e = e.cpu().numpy()
    we, wc = ORC.aggregate(X, op, ids, seg, Sg, 0.5)
    assert np.array_equal(c.cpu().numpy(), wc)
    for t in targets:
        blk = t // 16 * 16
        clean = [s for s in range(blk, blk + 16) if s != t]
        hit = [s for s in clean if np.isnan(e[s]).any()]
        assert not hit, "NaN reached segments %s of the block of segment %d (columns %s)" % (
            hit, t, sorted(set(np.argwhere(np.isnan(e[hit]))[:, 1].tolist())))
        assert np.array_equal(sv.bits(e[clean]), sv.bits(we[clean])), (D, fanout, op, t)
    m = sv.mismatch(e, we, op, wc)
    assert not m, (D, fanout, op, m)
    # an unknown id whose default row is NaN: the same contamination path through the staged default row
    ids2 = ids.copy()
    ids2[target * fanout] = 10 ** 9
    e2, _ = f.aggregate(op, torch.from_numpy(ids2).cuda(), None, Sg, default_attr=float("nan"))
    we2, wc2 = ORC.aggregate(X, op, ids2, seg, Sg, float("nan"))
    m = sv.mismatch(e2.cpu().numpy(), we2, op, wc2)
    assert not m, (D, fanout, op, "NaN default", m)


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("fanout", [1, 4, 10])
def test_mfma_subnormal_and_special_segments(knobs, D, fanout):
    """Subnormal rows, subnormal sums and means, signed zeros, overflow -- through the MFMA ablation (this also measures
    whether f32 MFMA keeps subnormal inputs and results on the device: it must, for bit-identity)."""
    X, ids, seg, Sg, d = sv.build_case(D, 40 + D, 0.25, blocks=1, empty=False)
    reqs = [r for r in _requests(ids, seg, Sg) if r[2] is None]
    sub = np.full((64, D), sv.SUB_MID, np.float32)
    sub[::2] = -sv.SUB
    sub[1::4] = sv.SUB_BIG
    sub[3::8] = sv.TINY
    big = np.full((64, D), sv.FLT_MAX, np.float32)  # sums that overflow inside one 4-row MFMA step
    big[1::3] = -sv.FLT_MAX
    big[2::5] = 3e38
    big[3::7] = 1.0
    f_sub = glx.Features(torch.from_numpy(sub).cuda())
    f_big = glx.Features(torch.from_numpy(big).cuda())
    f = glx.Features(torch.from_numpy(X).cuda())
    knobs(agg_mfma=1)
    rng = np.random.default_rng(fanout)
    sid = rng.integers(0, 64, 48 * fanout).astype(np.int64)
    for op in ("SumAggregator", "MeanAggregator"):
        got = f_sub.aggregate(op, torch.from_numpy(sid).cuda(), None, 48)
        want = ORC.aggregate(sub, op, sid, (np.arange(sid.shape[0]) // fanout).astype(np.int32), 48)
        _check(got, want, op, ("subnormal rows", D, fanout))
        got = f_big.aggregate(op, torch.from_numpy(sid).cuda(), None, 48)
        want = ORC.aggregate(big, op, sid, (np.arange(sid.shape[0]) // fanout).astype(np.int32), 48)
        _check(got, want, op, ("overflowing rows", D, fanout))
        for label, i, _, n in reqs:
            got = f.aggregate(op, torch.from_numpy(i).cuda(), None, n, default_attr=float(d))
            want = ORC.aggregate(X, op, i, (np.arange(i.shape[0]) // (i.shape[0] // n)).astype(np.int32), n, float(d))
            _check(got, want, op, ("special rows", D, label))


# ---- 5. one request big enough for the stripes ----------------------------------------------------------------------
def test_full_size_request_with_special_values(knobs):
    """>= 4 M ids at D = 256 take the XCD stripes by default; special values in the table."""
    rng = np.random.default_rng(12)
    V, f, D = 100_000, 10, 256
    Sg = (4 << 20) // f + 13
    X = rng.standard_normal((V, D)).astype(np.float32)
    pool = np.array(sv.POOL, np.float32)
    mask = rng.random((V, D)) < 0.03
    X[mask] = pool[rng.integers(0, pool.shape[0], int(mask.sum()))]
    ids = rng.integers(-2, V + 2, Sg * f).astype(np.int64)
    feats = glx.Features(torch.from_numpy(X).cuda())
    ti = torch.from_numpy(ids).cuda()
    n = 3000
    tail = ids[-n * f:]
    for op in ("MaxAggregator", "SumAggregator"):
        knobs()
        e, c = feats.aggregate(op, ti, None, Sg, default_attr=sv.NAN[3])
        torch.cuda.synchronize()
        e_tail, c_tail = e[-n:].cpu().numpy(), c[-n:].cpu().numpy()
        head_e, head_c = e[:n].cpu().numpy(), c[:n].cpu().numpy()
        del e, c
        knobs(agg_xcd_stripes=0, agg_xcd_slices=1)
        e0, c0 = feats.aggregate(op, ti, None, Sg, default_attr=sv.NAN[3])
        torch.cuda.synchronize()
        want = ORC.aggregate(X, op, tail, (np.arange(n * f) // f).astype(np.int32), n, sv.NAN[3])
        _check((e_tail, c_tail), want, op, "stripes tail vs oracle")
        _check((e0[-n:], c0[-n:]), want, op, "in order tail vs oracle")
        want = ORC.aggregate(X, op, ids[:n * f], (np.arange(n * f) // f).astype(np.int32), n, sv.NAN[3])
        _check((head_e, head_c), want, op, "stripes head vs oracle")
        del e0, c0
        torch.cuda.empty_cache()


# ---- 6. captured plans ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg", ["SumAggregator", "MaxAggregator", "MeanAggregator"])
def test_plan_with_special_values(agg):
    import synth
    V, D = 3000, 128
    rp, col, eid, w = synth.small_graph(V, 40000, seed=9, weighted=True, hub_degree=1000)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    g = glx.Graph(t(rp), t(col), t(eid), t(w))
    rng = np.random.default_rng(6)
    X = rng.standard_normal((V, D)).astype(np.float32)
    pool = np.array(sv.POOL, np.float32)
    mask = rng.random((V, D)) < 0.05
    X[mask] = pool[rng.integers(0, pool.shape[0], int(mask.sum()))]
    X[0] = -0.0  # the hub row
    X[0, ::7] = sv.NAN[1]
    f = glx.Features(t(X))
    plan = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[f, f], agg=agg, seed=5)
    try:
        for run in range(2):
            seeds = t(rng.integers(0, V, 512).astype(np.int64))
            hops = plan.run(seeds, call_counter=10 * run)
            hops = [{k: v.clone() for k, v in h.items()} for h in hops]
            ref = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, [25, 10], seed=5, call_counter=10 * run)
            torch.cuda.synchronize()
            for h in range(2):
                ids = ref[h][0].view(-1).cpu().numpy()
                n, k = ref[h][0].shape
                want = ORC.aggregate(X, agg, ids, (np.arange(n * k) // k).astype(np.int32), n)
                _check((hops[h]["emb"], hops[h]["cnt"]), want, agg, ("plan", run, h))
    finally:
        plan.close()


# ---- 7. the 3-source distributed reduce and lookup ------------------------------------------------------------------
def test_three_source_distributed_reduce_and_lookup(knobs):
    """Own shard + hot-row replica + halo rows, with NaN / -0.0 / inf in the replicated and the halo rows."""
    import dist as gdist
    import synth
    V, D, P = 4000, 128, 2
    rp, col, eid, w = synth.small_graph(V, 60000, seed=5, weighted=True, hub_degree=2000)
    rng = np.random.default_rng(8)
    X = rng.standard_normal((V, D)).astype(np.float32)
    hot = np.argsort(-np.bincount(col, minlength=V), kind="stable")[:300].astype(np.int64)
    X[hot[::3], ::5] = sv.NAN[4]
    X[hot[1::3]] = -0.0
    X[hot[2::3], 3] = -np.inf
    cold = np.setdiff1d(np.arange(V), hot)[::7]
    X[cold, 1::4] = sv.NAN[5]
    X[cold[::2], 2::4] = -0.0
    X[cold[1::2], 0] = sv.SUB
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    whole = glx.Features(t(X))
    fs = []
    for r in range(P):
        _, _, _, _, sids = gdist.shard_graph(t(rp), t(col), t(eid), t(w), r, P)
        fs.append(glx.Features(t(X[r::P].copy()), ids=sids))
    for i, s in enumerate([dict(agg_xcd_stripes=0), dict(), dict(agg_legacy=1)]):
        knobs(**s)
        errors = [None] * P
        key = 78100 + i

        def main(r):
            try:
                comm = glx.Comm.local(key, 0, r, P)
                with torch.cuda.stream(torch.cuda.Stream(device=0)):
                    st = glx.DistStore(comm, features=fs[r])
                    st.set_cache(hot, default_attr=3.0)
                    rng = np.random.default_rng(60 + r)
                    n, f = 20000 + 30 * r, 10
                    h = np.where(rng.random(n) < 0.6, hot[rng.integers(0, 300, n)], rng.integers(-3, V + 3, n))
                    h = h.astype(np.int64)
                    ids = t(h)
                    for dflt in (sv.NAN[2], -0.0):
                        for name in AGGREGATORS:
                            e, c = st.aggregate(name, ids, None, n // f, default_attr=dflt)
                            want = ORC.aggregate(X, name, h, (np.arange(n) // f).astype(np.int32), n // f, dflt)
                            _check((e, c), want, name, ("dist", r, s, dflt))
                        lk = st.lookup(ids[:4000], default_attr=dflt).cpu().numpy()
                        wl = np.where(((h[:4000] >= 0) & (h[:4000] < V))[:, None], X[np.clip(h[:4000], 0, V - 1)],
                                      np.float32(dflt))
                        assert np.array_equal(sv.bits(lk), sv.bits(wl)), ("dist lookup", r, s, dflt)
                    torch.cuda.current_stream().synchronize()
            except BaseException as ex:  # noqa: BLE001
                errors[r] = ex
        ts = [threading.Thread(target=main, args=(r,)) for r in range(P)]
        for th in ts:
            th.start()
        for th in ts:
            th.join(300)
        assert not any(th.is_alive() for th in ts), "a rank hung"
        for e in errors:
            if e is not None:
                raise e


# ---- 8. the stitch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Sg,D", [(1, 33, 1), (3, 70, 3), (3, 70, 8), (8, 40, 64)])
def test_aggregate_stitch_with_special_values(P, Sg, D):
    rng = np.random.default_rng(P * 1000 + D)
    pool = np.array(sv.POOL, np.float32)
    parts = pool[rng.integers(0, pool.shape[0], (P, Sg, D))]
    cnts = rng.integers(0, 4, (P, Sg)).astype(np.int32)
    cnts[:, 0] = 0
    cnts[0, 1:4] = 0
    parts[cnts == 0] = sv.NAN[0]  # what an empty partial holds must not matter
    dev = torch.device("cuda", 0)
    for dflt in sv.DEFAULTS:
        for name in AGGREGATORS:
            got = glx.aggregate_stitch(name, torch.from_numpy(parts).to(dev), torch.from_numpy(cnts).to(dev), dflt)
            _check(got, ORC.aggregate_stitch(name, parts, cnts, dflt), name, ("stitch", P, D, dflt))


# ---- 9. lookup: a move, so every bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tdt", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 8, 64, 264])
def test_lookup_keeps_every_bit(name, tdt, D):
    rng = np.random.default_rng(D)
    V = 300
    pool = np.concatenate([np.array(sv.POOL, np.float32), sv.f32([0x7F800001, 0xFF800123, 0x80000001])])
    X = pool[rng.integers(0, pool.shape[0], (V, D))]
    want_rows = _upcast(X, tdt)
    raw = rng.permutation(5 * V)[:V].astype(np.int64) * 3 - 100
    for ids_kind in ("dense", "hashed"):
        known = np.arange(V, dtype=np.int64) if ids_kind == "dense" else raw
        q = np.concatenate([known[rng.integers(0, V, 700)], np.array([-1, 10 ** 9, -7], np.int64)])
        row_of = {int(k): i for i, k in enumerate(known)}
        rows = np.array([row_of.get(int(x), -1) for x in q])
        for host in (False, True):
            src = torch.from_numpy(X) if host else torch.from_numpy(X).cuda()
            ids = None if ids_kind == "dense" else (raw if host else torch.from_numpy(raw).cuda())
            f = glx.Features(src, ids=ids, dtype=name)
            for dflt in sv.DEFAULTS:
                got = f.lookup(q if host else torch.from_numpy(q).cuda(), default_attr=dflt)
                want = np.where((rows >= 0)[:, None], want_rows[np.maximum(rows, 0)], np.float32(dflt))
                m = sv.mismatch(_np(got), want, "lookup")
                assert not m, (name, D, ids_kind, host, dflt, m)


# ---- 10. what the device's arithmetic NaNs look like (reported, not asserted) --------------------------------------
def test_report_arithmetic_nan_payloads(capsys):
    X, ids, seg, Sg, d = sv.build_case(64, 3, 0.0)
    f = glx.Features(torch.from_numpy(X).cuda())
    lines = []
    for op in ("SumAggregator", "MeanAggregator", "ProdAggregator"):
        e, c = f.aggregate(op, torch.from_numpy(ids).cuda(), torch.from_numpy(seg).cuda(), Sg, default_attr=float(d))
        we, _ = ORC.aggregate(X, op, ids, seg, Sg, float(d))
        e = e.cpu().numpy()
        nan = np.isnan(we)
        same = int((sv.bits(e)[nan] == sv.bits(we)[nan]).sum())
        lines.append("%s: %d NaN outputs, %d with the oracle's payload; device payloads %s" % (
            op, int(nan.sum()), same, sorted({"%08x" % x for x in sv.bits(e)[nan]})[:6]))
    with capsys.disabled():
        print("\nNaN payloads of arithmetic results:\n  " + "\n  ".join(lines))
