"""Host-pointer staging (GlxHostStage) of every per-request entry point: pageable numpy buffers, numpy buffers pinned
with glx_host_register, and torch device tensors give bit-identical answers, size-dependent responses included; empty
requests work; a request refused after its staging began leaves the thread's workspace lease free for the next one; two
host threads on one device do not disturb each other.

The pinned variant runs in a process of its own (this file as a script), like tests/scripts/pinned_host_check.py: pinned
ranges are whole anonymous mappings, and the process ends right after it unregisters them."""
import ctypes
import itertools
import mmap
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "graph-learn_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import glx  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

V, E, D = 1500, 30000, 24
_FABRIC = itertools.count(0x57A6E000)


def _world():
    rng = np.random.default_rng(5)
    rp, col, eid, w = synth.small_graph(V, E, seed=17, weighted=True, hub_degree=300)
    g = glx.Graph(rp, col, eid, w)
    g.enable_in_degree()
    g.enable_negative()
    f = glx.Features(rng.standard_normal((V, D)).astype(np.float32))
    neg = glx.Negative(np.arange(V, dtype=np.int64), rng.random(V).astype(np.float32) + 0.1)
    keys = rng.integers(0, 4, (1, V)).astype(np.int64)
    cond = glx.CondTable(np.arange(V, dtype=np.int64), rng.random(V).astype(np.float32) + 0.1, keys)
    os.environ["GLX_DIST_NO_SHORTCUT"] = "1"  # world size 1 through the store's generic (collective) paths
    try:
        st = glx.DistStore(glx.Comm.local(next(_FABRIC), 0, 0, 1), graph=g, features=f)
    finally:
        del os.environ["GLX_DIST_NO_SHORTCUT"]
    st.enable_in_degree()
    dneg = st.negative_table()
    return dict(g=g, f=f, neg=neg, cond=cond, st=st, dneg=dneg, rng=rng)


def _requests(n, seed=3):
    rng = np.random.default_rng(seed)
    return dict(
        src=rng.integers(0, V, n).astype(np.int64),
        vals=rng.integers(0, V, n).astype(np.int64),
        rows=rng.permutation(n).astype(np.int64),
        seg=np.sort(rng.integers(0, max(n // 4, 1), n)).astype(np.int32),
        dst=rng.integers(0, V, n).astype(np.int64),
        keys=rng.integers(0, 4, (n, 1)).astype(np.int64),
    )


def _np(x):
    if isinstance(x, (tuple, list)):
        return [_np(y) for y in x]
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run_all(w, req, conv):
    """Every ported entry point on one request; conv turns a numpy input into the pointer kind under test."""
    g, f, st = w["g"], w["f"], w["st"]
    r = {k: conv(v) for k, v in req.items()}
    n = int(req["src"].shape[0])
    nseg = int(req["seg"][-1]) + 1 if n else 0
    out = {}
    out["sample"] = g.sample("EdgeWeightSampler", r["src"], 5, seed=1, call_counter=2)
    out["sample_ex"] = g.sample("RandomSampler", r["src"], 4, seed=1, call_counter=3, rng_rows=r["rows"])
    if n or not glx._is_torch(r["src"]):  # an empty torch tensor has no data pointer, which glx_sample_hops refuses
        out["sample_hops"] = glx.sample_hops([g, g], "RandomSampler", r["src"], [3, 2], seed=4)
    out["sample_filtered"] = g.sample_filtered("TopkSampler", r["src"], 4, glx.FILTER_EQUAL, glx.FILTER_FIELD_ID, r["vals"])
    out["sample_full"] = g.sample_full(r["src"], max_limit=7)
    deg, nbr, eid = out["sample_full"]
    offs = np.concatenate([[0], np.cumsum(_np(deg).astype(np.int64))]).astype(np.int64)
    out["sample_full_filtered"] = g.sample_full_filtered(r["src"], 7, glx.FILTER_EQUAL, glx.FILTER_FIELD_ID, r["vals"])
    out["aggregate"] = f.aggregate("MeanAggregator", r["src"], r["seg"], nseg)
    out["lookup"] = f.lookup(r["src"])
    out["random_walk"] = g.random_walk(r["src"], 4, p=0.5, q=2.0, seed=6)
    out["degrees"] = g.degrees(r["src"])
    out["in_degrees"] = g.in_degrees(r["src"])
    out["negative"] = w["neg"].sample(r["src"], 3, exclude=glx.NEG_EXCLUDE_BATCH, seed=8)
    out["negative_nbrs"] = w["neg"].sample(r["src"], 3, exclude=glx.NEG_EXCLUDE_NEIGHBORS, graph=g, seed=8)
    out["cond_negative"] = w["cond"].sample(g, r["src"], r["dst"], r["keys"], [0.5], 4, seed=9)
    out["subgraph"] = glx.subgraph_induce(r["src"], conv(offs), nbr, eid)
    out["dist_sample"] = st.sample("EdgeWeightSampler", r["src"], 5, seed=1, call_counter=2)
    out["dist_sample_filtered"] = st.sample("TopkSampler", r["src"], 4, filter_type=glx.FILTER_EQUAL,
                                            filter_field=glx.FILTER_FIELD_ID, values=r["vals"])
    out["dist_sample_full"] = st.sample_full(r["src"], max_limit=7)
    out["dist_sample_full_filtered"] = st.sample_full(r["src"], 7, filter_type=glx.FILTER_EQUAL,
                                                      filter_field=glx.FILTER_FIELD_ID, values=r["vals"])
    out["dist_random_walk"] = st.random_walk(r["src"], 3, seed=6)
    out["dist_random_walk_n2v"] = st.random_walk(r["src"], 3, p=0.5, q=2.0, seed=6)
    out["dist_aggregate"] = st.aggregate("SumAggregator", r["src"], r["seg"], nseg)
    out["dist_aggregate_partial"] = st.aggregate("SumAggregator", r["src"], r["seg"], nseg, partial=True)
    out["dist_lookup"] = st.lookup(r["src"])
    out["dist_in_degrees"] = st.in_degrees(r["src"])
    out["dist_negative"] = st.negative_sample(w["dneg"], r["src"], 3, exclude=glx.NEG_EXCLUDE_NEIGHBORS, seed=8)
    return {k: _np(v) for k, v in out.items()}


def _device_conv(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _flat(x):
    return [z for y in x for z in _flat(y)] if isinstance(x, list) else [x]


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        xa, xb = _flat(a[k]), _flat(b[k])
        assert len(xa) == len(xb), (what, k)
        for i, (p, q) in enumerate(zip(xa, xb)):
            p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
            assert p.dtype == q.dtype and p.shape == q.shape, (what, k, i, p.shape, q.shape)
            assert p.tobytes() == q.tobytes(), (what, k, i)


@pytest.fixture(scope="module")
def world():
    return _world()


def test_host_and_device_pointers_agree(world):
    req = _requests(400)
    host = run_all(world, req, lambda a: np.ascontiguousarray(a))
    dev = run_all(world, req, _device_conv)
    _assert_same(host, dev, "pageable vs device")
    # the response really has content (a size-dependent one included)
    assert host["sample_full"][1].size > 0 and host["subgraph"][0].size > 0 and host["dist_sample_full"][1].size > 0


def test_empty_requests(world):
    req = _requests(0)
    host = run_all(world, req, lambda a: np.ascontiguousarray(a))
    dev = run_all(world, req, _device_conv)
    assert len(host.pop("sample_hops")) == 2
    _assert_same(host, dev, "empty")
    assert all(x.size == 0 for v in host.values() for x in _flat(v))


def test_refused_request_then_good_request(world):
    """Requests refused by the argument checks -- before the staging, and after it began (the condition proportions
    are checked once the inputs are on the device) -- leave this thread's slot-0 lease free: the next request answers
    right."""
    req = _requests(300, seed=11)
    want = run_all(world, req, lambda a: np.ascontiguousarray(a))
    g = world["g"]
    for _ in range(2):
        with pytest.raises(glx.GlxError):
            world["cond"].sample(g, req["src"], req["dst"], req["keys"], [1.5], 4, seed=9)
        with pytest.raises(glx.GlxError):
            g.sample("EdgeWeightSampler", req["src"], 5, padding_mode=7)
    got = run_all(world, req, lambda a: np.ascontiguousarray(a))
    _assert_same(want, got, "after refusals")


def test_two_host_threads(world):
    reqs = [_requests(500, seed=s) for s in (21, 22)]
    want = [run_all(world, r, lambda a: np.ascontiguousarray(a)) for r in reqs]
    g, f = world["g"], world["f"]
    errors = []

    def body(r, wnt):
        try:
            for _ in range(20):
                n, e = g.sample("EdgeWeightSampler", r["src"], 5, seed=1, call_counter=2)
                assert np.array_equal(n, wnt["sample"][0]) and np.array_equal(e, wnt["sample"][1])
                emb, cnt = f.aggregate("MeanAggregator", r["src"], r["seg"], int(r["seg"][-1]) + 1)
                assert emb.tobytes() == wnt["aggregate"][0].tobytes() and np.array_equal(cnt, wnt["aggregate"][1])
                deg, nbr, eid = g.sample_full(r["src"], max_limit=7)
                assert np.array_equal(nbr, wnt["sample_full"][1]) and np.array_equal(eid, wnt["sample_full"][2])
        except BaseException as ex:  # noqa: BLE001
            errors.append(ex)
    ts = [threading.Thread(target=body, args=(r, w)) for r, w in zip(reqs, want)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_pinned_buffers_agree():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0 and "PINNED_STAGE_OK" in r.stdout, r.stdout[-3000:]


def _pinned_main():
    """Inputs pinned for every entry point; outputs pinned too for the calls that write them directly."""
    L = glx.lib()
    owners = []

    def pinned(a):
        a = np.ascontiguousarray(a)
        span = max((a.nbytes + 4095) // 4096 * 4096, 4096)
        gran = 2 << 20  # whole pages of an anonymous mapping of their own, never a range of the malloc heap
        mm = mmap.mmap(-1, span + gran, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
        raw = np.frombuffer(mm, np.uint8)
        off = (-raw.ctypes.data) % gran
        b = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        assert L.glx_host_register(ctypes.c_void_p(b.ctypes.data), span) == 0, L.glx_last_error()
        owners.append((mm, raw, b))
        b[...] = a
        return b

    w = _world()
    req = _requests(400)
    want = run_all(w, req, lambda a: np.ascontiguousarray(a))
    _assert_same(want, run_all(w, req, pinned), "pageable vs pinned inputs")
    # outputs written straight into pinned buffers: aggregate (out=), sample / sample_filtered / lookup (raw calls)
    g, f = w["g"], w["f"]
    src = pinned(req["src"])
    nseg = int(req["seg"][-1]) + 1
    emb, cnt = pinned(np.zeros((nseg, D), np.float32)), pinned(np.zeros(nseg, np.int32))
    f.aggregate("MeanAggregator", src, pinned(req["seg"]), nseg, out=(emb, cnt))
    assert emb.tobytes() == want["aggregate"][0].tobytes() and np.array_equal(cnt, want["aggregate"][1])
    n, k = src.shape[0], 5
    nbr, eid = pinned(np.zeros((n, k), np.int64)), pinned(np.zeros((n, k), np.int64))
    vp = ctypes.c_void_p
    assert L.glx_sample(g._h, glx.SAMPLER_IDS["EdgeWeightSampler"], vp(src.ctypes.data), n, k, glx.PAD_CIRCULAR, 0, 1, 2,
                        vp(nbr.ctypes.data), vp(eid.ctypes.data), glx.PTR_HOST, None) == 0, L.glx_last_error()
    assert np.array_equal(nbr, want["sample"][0]) and np.array_equal(eid, want["sample"][1])
    look = pinned(np.zeros((n, D), np.float32))
    assert L.glx_lookup(f._h, vp(src.ctypes.data), n, ctypes.c_float(0.0), vp(look.ctypes.data), glx.PTR_HOST, None) == 0
    assert look.tobytes() == want["lookup"].tobytes()
    for _, _, b in owners:
        assert L.glx_host_unregister(ctypes.c_void_p(b.ctypes.data)) == 0
    print("PINNED_STAGE_OK")


if __name__ == "__main__":
    _pinned_main()
