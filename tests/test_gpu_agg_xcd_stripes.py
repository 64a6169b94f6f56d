"""GPU tests of the XCD-stripe mapping of the grouped aggregation kernel (glx_aggregate.hip agg_stripe_block): the
slice-local workgroup index is permuted so the XCDs that share a column slice walk contiguous chunks of segment
blocks.  Every (segment block, slice) pair must still be reduced exactly once and every output element accumulated in
the reference's order: bit-identical to the oracle and to the launch without stripes, for every setting glx_tune can
select and for segment counts that do not fill a chunk, a run of chunks, or a single workgroup."""
import numpy as np
import pytest
import torch

import glx
from oracle_bindings import Oracle

pytestmark = pytest.mark.gpu
AGGS = ["MaxAggregator", "SumAggregator", "MeanAggregator"]
DEFAULTS = dict(agg_xcd_slices=0, agg_xcd_stripes=-1, agg_xcd_chunk=0, agg_segs=0)
OFF = dict(agg_xcd_stripes=0)
SETTINGS = [dict(), dict(agg_xcd_stripes=1)] + [
    dict(agg_xcd_stripes=1, agg_xcd_slices=n, agg_xcd_chunk=c) for n in (1, 2, 4) for c in (1, 3, 64)] + [
    dict(agg_xcd_stripes=1, agg_xcd_slices=n, agg_xcd_chunk=c, agg_segs=3) for n in (1, 2) for c in (1, 3)] + [
    dict(agg_xcd_stripes=1, agg_xcd_slices=8, agg_xcd_chunk=1)]


def beq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture
def knobs():
    def set_knobs(**kw):
        for k, v in DEFAULTS.items():
            glx.tune(k, kw.get(k, v))
    yield set_knobs
    set_knobs()


def _check_all(knobs, feats, X, ids, seg, h_seg, Sg, label):
    """Every setting against the oracle and against stripes switched off (same process); seg may be None (dense
    response), h_seg is what the oracle reads."""
    orc = Oracle()
    h_ids = ids.cpu().numpy()
    for name in AGGS:
        want_e, want_c = orc.aggregate(X, name, h_ids, h_seg, Sg, 1.25)
        knobs(**OFF)
        off_e, off_c = feats.aggregate(name, ids, seg, Sg, default_attr=1.25)
        torch.cuda.synchronize()
        assert beq(off_e.cpu().numpy(), want_e) and np.array_equal(off_c.cpu().numpy(), want_c), (label, name)
        for s in SETTINGS:
            knobs(**s)
            e, c = feats.aggregate(name, ids, seg, Sg, default_attr=1.25)
            torch.cuda.synchronize()
            assert torch.equal(e.view(torch.int32), off_e.view(torch.int32)), (label, name, s)
            assert torch.equal(c, off_c), (label, name, s)


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("Sg", [0, 5, 1037, 4099])
def test_dense_responses_every_setting(knobs, D, Sg):
    """segment_ids = None (a dense sampler response), fanout 10: no segments, fewer than one workgroup, and counts
    that leave a partial run of chunks and a partial workgroup."""
    rng = np.random.default_rng(D + Sg)
    V, f = 3000, 10
    X = (rng.standard_normal((V, D)) * 3).astype(np.float32)
    X[rng.random((V, D)) < 0.02] = -50.0  # below Max's -37 initialiser
    feats = glx.Features(torch.from_numpy(X).cuda(), device=0)
    h = rng.integers(-2, V + 2, Sg * f).astype(np.int64)
    ids = torch.from_numpy(h).cuda()
    h_seg = (np.arange(Sg * f) // f).astype(np.int32)
    seg = torch.from_numpy(h_seg).cuda()
    _check_all(knobs, feats, X, ids, None, h_seg, Sg, "dense")
    _check_all(knobs, feats, X, ids, seg, h_seg, Sg, "explicit dense segment_ids")


@pytest.mark.parametrize("D", [128, 256])
def test_ragged_segment_ids_every_setting(knobs, D):
    """Explicit ragged segment_ids: empty segments, a long one (several id chunks), unknown ids."""
    rng = np.random.default_rng(7 * D)
    V, Sg = 2000, 3001
    X = rng.standard_normal((V, D)).astype(np.float32)
    feats = glx.Features(torch.from_numpy(X).cuda(), device=0)
    sizes = rng.integers(0, 14, Sg)
    sizes[[0, 5, Sg - 1]] = 0
    sizes[9] = 300
    h_seg = np.repeat(np.arange(Sg, dtype=np.int32), sizes)
    seg = torch.from_numpy(h_seg).cuda()
    ids = torch.from_numpy(rng.integers(-3, V + 3, int(sizes.sum())).astype(np.int64)).cuda()
    _check_all(knobs, feats, X, ids, seg, h_seg, Sg, "ragged")


def test_default_big_request_takes_stripes_bit_identical(knobs):
    """A request of >= 4 M ids takes the stripes by default (D = 256: whole rows, n = 1; D = 128: n = 2); same bits as
    stripes off, as the old two-slice default, and -- on a slice -- as the oracle."""
    rng = np.random.default_rng(11)
    V, f = 100_000, 10
    Sg = (4 << 20) // f + 13
    h = rng.integers(-2, V + 2, Sg * f).astype(np.int64)
    ids = torch.from_numpy(h).cuda()
    for D in (128, 256):
        X = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).cuda()
        feats = glx.Features(X, device=0)
        out = {}
        for label, s in (("default", dict()), ("off", OFF), ("old default", dict(agg_xcd_stripes=0, agg_xcd_slices=2)),
                         ("chunk 5", dict(agg_xcd_chunk=5))):
            knobs(**s)
            e, c = feats.aggregate("MaxAggregator", ids, None, Sg)
            torch.cuda.synchronize()
            out[label] = (e.clone(), c.clone())
            del e, c
        for label in ("off", "old default", "chunk 5"):
            assert torch.equal(out["default"][0].view(torch.int32), out[label][0].view(torch.int32)), (D, label)
            assert torch.equal(out["default"][1], out[label][1]), (D, label)
        n = 3000
        oe, oc = Oracle().aggregate(X.cpu().numpy(), "MaxAggregator", h[-n * f:], (np.arange(n * f) // f).astype(np.int32), n)
        assert beq(out["default"][0][-n:].cpu().numpy(), oe) and np.array_equal(out["default"][1][-n:].cpu().numpy(), oc)
        del out, feats, X
        torch.cuda.empty_cache()


def test_three_source_distributed_reduce(knobs):
    """The distributed store's 3-source reduce (own shard + hot-row replica + halo rows): every setting equals the
    unpartitioned operator."""
    import threading
    import dist as gdist
    import synth
    V, D, P = 4000, 128, 2
    rp, col, eid, w = synth.small_graph(V, 60000, seed=5, weighted=True, hub_degree=2000)
    X = np.random.default_rng(8).standard_normal((V, D)).astype(np.float32)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    whole = glx.Features(t(X))
    fs = []
    for r in range(P):
        _, _, _, _, sids = gdist.shard_graph(t(rp), t(col), t(eid), t(w), r, P)
        fs.append(glx.Features(t(X[r::P].copy()), ids=sids))
    hot = np.argsort(-np.bincount(col, minlength=V), kind="stable")[:300].astype(np.int64)
    for i, s in enumerate([OFF] + SETTINGS[:8]):
        knobs(**s)
        errors = [None] * P
        key = 77000 + i  # a fabric of its own per setting

        def main(r):
            try:
                comm = glx.Comm.local(key, 0, r, P)
                with torch.cuda.stream(torch.cuda.Stream(device=0)):
                    st = glx.DistStore(comm, features=fs[r])
                    st.set_cache(hot, default_attr=3.0)
                    rng = np.random.default_rng(60 + r)
                    n, f = 20000 + 30 * r, 10
                    ids = np.where(rng.random(n) < 0.6, hot[rng.integers(0, 300, n)], rng.integers(-3, V + 3, n))
                    ids = t(ids.astype(np.int64))
                    for name in AGGS:
                        e, c = st.aggregate(name, ids, None, n // f, default_attr=0.5)
                        ref_e, ref_c = whole.aggregate(name, ids, None, n // f, default_attr=0.5)
                        assert torch.equal(c, ref_c) and torch.equal(e.view(torch.int32), ref_e.view(torch.int32)), (name, r, s)
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


@pytest.mark.parametrize("agg", ["MaxAggregator", "MeanAggregator"])
def test_plan_replayed_twice_with_stripes(knobs, agg):
    """A glx_plan captures the launch shape once; replayed twice with stripes forced on (chunk 1: the small plan's
    blocks are permuted) it equals the eager sample + aggregate."""
    import synth
    V, D = 3000, 256
    rp, col, eid, w = synth.small_graph(V, 40000, seed=9, weighted=True, hub_degree=1000)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    g = glx.Graph(t(rp), t(col), t(eid), t(w))
    f = glx.Features(t(np.random.default_rng(3).standard_normal((V, D)).astype(np.float32)))
    knobs(agg_xcd_stripes=1, agg_xcd_chunk=1)
    plan = glx.Plan([g, g], "EdgeWeightSampler", [25, 10], 512, features=[f, f], agg=agg, seed=5)
    rng = np.random.default_rng(1)
    for run in range(2):
        seeds = t(rng.integers(0, V, 512).astype(np.int64))
        hops = plan.run(seeds, call_counter=10 * run)
        ref = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, [25, 10], seed=5, call_counter=10 * run)
        torch.cuda.synchronize()
        for h in range(2):
            knobs(**OFF)
            e, c = f.aggregate(agg, ref[h][0].view(-1), None, ref[h][0].shape[0])
            torch.cuda.synchronize()
            assert torch.equal(hops[h]["cnt"], c), (run, h)
            assert torch.equal(hops[h]["emb"].view(torch.int32), e.view(torch.int32)), (run, h)
    plan.close()
