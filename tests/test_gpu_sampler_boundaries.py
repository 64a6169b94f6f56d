"""The samplers at every launch boundary, bit for bit against the oracle (oracle/glx_oracle.c).

sample_device (csrc/glx_sample.hip) picks its kernel by k, by row length, by edge-id range and by output alignment.
Each case below sits on both sides of one of those choices:
  * RandomWithoutReplacement, circular padding: glx_rwor_small_kernel<W, K> for every k <= 16, glx_rwor_kernel<32>,
    <64>, and glx_rwor_lds_kernel up to k = 8192, whose dynamic LDS (12 bytes per k) passes 64 KiB at k = 5462;
    k = 8193 is refused.  Batches leave the last wave (and, for the small kernel, the last block) partly full.
  * the same kernels over row prefixes of 0, 1, k, 2k + 1 and most of a hub row (timestamp > value filters), and
    FullSampler under that filter;
  * the slot kernel's paired 16-byte store against outputs that are 8- but not 16-byte aligned;
  * EdgeWeight's packed records (every edge id fits an int32) and the unpacked fallback;
  * the alias build's lane-per-row / wave-per-row split at 96 slots, unfiltered and over filtered reserved lists;
  * the id == value filter's fast paths around kMaxHits = 8 and kFastMaxK = 32;
  * rows longer than 2^24, where the float cast of the alias variate decides the slot;
  * the multi-hop driver at the new fanouts.
"""
import ctypes
import mmap
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "graph-learn_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import glx  # noqa: E402
from oracle_bindings import Oracle  # noqa: E402

pytestmark = pytest.mark.gpu

RANDOM, RWOR, EDGE_WEIGHT, TOPK, IN_DEGREE = ("RandomSampler", "RandomWithoutReplacementSampler", "EdgeWeightSampler",
                                              "TopkSampler", "InDegreeSampler")
CIRC, REPL = glx.PAD_CIRCULAR, glx.PAD_REPLICATE
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
KS = list(range(1, 17)) + [17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 4096, 5461, 5462, 8192]
HUB = 40000  # >> the largest k


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert glx.device_count() >= 1, "GPU tests need a HIP device; glx has no CPU fallback"


def same(got, want):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))


def host(x):
    return x.cpu().numpy() if glx._is_torch(x) else x


def cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def csr(degrees, rng, num_cols):
    rp = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    E = int(rp[-1])
    col = rng.integers(0, num_cols, E).astype(np.int64)
    eid = rng.permutation(E).astype(np.int64)
    return rp, col, eid


def rwor_small_rows_per_wave(k):
    """Rows per wavefront of glx_rwor_small_kernel<W, k> (launch_rwor_small)."""
    p2 = 1 if k <= 1 else 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16
    return 64 // (k if 64 // k > 64 // p2 else p2)


def batch_for(k):
    if k <= 16:
        R = rwor_small_rows_per_wave(k)
        # three whole blocks of four waves, then a block of two whole waves and one partly full wave
        return 12 * R + 2 * R + R // 2 + 1
    if k <= 64:
        return 67  # 256 / W rows per block (8 or 4): the last block and its last wave are partly full
    return 37  # one row per block


# ------------------------------------------------------------------ every RWoR kernel and LDS size ---
@pytest.fixture(scope="module")
def kgraph(orc):
    """One weighted graph with, for every k of KS, rows of degree 0, 1, k - 1, k, k + 1 and 2k, and a hub row of
    HUB >> k neighbours (row 0); neighbours are row indices, so hops can chain.  Dense ids and hashed ids."""
    rng = np.random.default_rng(2024)
    degrees, rows = [HUB], {}
    for k in KS:
        for d in (0, 1, k - 1, k, k + 1, 2 * k):
            rows[(k, d)] = len(degrees)
            degrees.append(d)
    V = len(degrees)
    rp, col, eid = csr(degrees, rng, V)
    w = (rng.random(col.shape[0]) * 0.99 + 0.01).astype(np.float32)
    dense = dict(row_ptr=rp, col=col, eid=eid, weight=w, alias=orc.alias_build(rp, w))
    raw = (np.arange(V, dtype=np.int64) * 13 - 900)[rng.permutation(V)]
    hashed = dict(row_ptr=rp, col=raw[col], eid=eid, weight=w, alias=dense["alias"], ids=raw)
    out = dict(rows=rows, V=V, raw=raw,
               dense=(dense, glx.Graph(rp, col, eid, w)),
               hashed=(hashed, glx.Graph(rp, raw[col], eid, w, ids=raw)))
    yield out
    out["dense"][1].close()
    out["hashed"][1].close()


def k_queries(kg, k, which, rng):
    idx = [0] + [kg["rows"][(k, d)] for d in (0, 1, k - 1, k, k + 1, 2 * k)]
    ids = np.arange(kg["V"], dtype=np.int64) if which == "dense" else kg["raw"]
    pattern = np.concatenate([ids[idx], [kg["V"] + 10 if which == "dense" else 10 ** 12]])  # + an unknown id
    B = batch_for(k)
    q = np.tile(pattern, B // pattern.shape[0] + 1)[:B]
    return q[rng.permutation(B)].astype(np.int64)


@pytest.mark.parametrize("k", KS, ids=["k%d" % k for k in KS])
def test_rwor_topk_random_at_every_kernel_boundary(orc, kgraph, k):
    import torch
    rng = np.random.default_rng(k)
    cc = 0
    for which in ("dense", "hashed"):
        og, dev = kgraph[which]
        q = k_queries(kgraph, k, which, rng)
        rr = rng.integers(0, 1 << 30, q.shape[0]).astype(np.int64)  # a shard's streams
        cases = [(RWOR, CIRC, None), (RWOR, CIRC, rr), (RWOR, REPL, None), (TOPK, CIRC, None), (TOPK, REPL, None),
                 (RANDOM, CIRC, None), (RANDOM, REPL, rr)]
        for name, pad, rows in cases:
            cc += 1
            want = orc.sample(og, name, q, k, seed=0x5eed + k, call_counter=cc, padding_mode=pad,
                              default_neighbor_id=-3, rng_rows=rows)
            got = dev.sample(name, q, k, seed=0x5eed + k, call_counter=cc, padding_mode=pad, default_neighbor_id=-3,
                             rng_rows=rows)
            assert same(got, want), (which, name, pad, rows is not None)
            if name == RWOR and pad == CIRC:  # device pointers
                got = dev.sample(name, cuda(q), k, seed=0x5eed + k, call_counter=cc, padding_mode=pad,
                                 default_neighbor_id=-3, rng_rows=cuda(rows))
                torch.cuda.synchronize()
                assert same([host(x) for x in got], want), (which, name, "device pointers", rows is not None)


def test_rwor_beyond_8192_is_refused_and_leaves_the_output_alone(kgraph):
    import torch
    _, dev = kgraph["dense"]
    q = np.array([0, 1, 2], np.int64)
    k = 8193
    nbr, eid = np.full((3, k), -77, np.int64), np.full((3, k), -78, np.int64)
    with pytest.raises(glx.GlxError) as e:
        dev.sample(RWOR, q, k, out=(nbr, eid))
    assert e.value.code == 3 and "8192" in str(e.value)
    assert (nbr == -77).all() and (eid == -78).all()
    tn, te = torch.full((3, k), -77, dtype=torch.int64, device="cuda"), torch.full((3, k), -78, dtype=torch.int64,
                                                                                   device="cuda")
    with pytest.raises(glx.GlxError) as e:
        dev.sample(RWOR, cuda(q), k, out=(tn, te))
    assert e.value.code == 3
    torch.cuda.synchronize()
    assert bool((tn == -77).all()) and bool((te == -78).all())
    # k = 8193 is refused for the without-replacement shuffle only: replicate padding and TopK serve it
    got = dev.sample(RWOR, q, k, padding_mode=REPL)
    assert got[0].shape == (3, k)


# --------------------------------------------------------------------- the multi-hop driver ---
@pytest.mark.parametrize("fanouts", [[65], [5462], [3, 129]], ids=["65", "5462", "3-129"])
@pytest.mark.parametrize("name", [RWOR, RANDOM])
def test_sample_hops_equals_chained_samples(orc, kgraph, fanouts, name):
    import torch
    og, dev = kgraph["dense"]
    rng = np.random.default_rng(sum(fanouts))
    seeds = np.concatenate([[0], rng.integers(0, kgraph["V"], 22)]).astype(np.int64)
    hops = glx.sample_hops([dev] * len(fanouts), name, seeds, fanouts, seed=91, call_counter=40)
    dhops = glx.sample_hops([dev] * len(fanouts), name, cuda(seeds), fanouts, seed=91, call_counter=40)
    torch.cuda.synchronize()
    frontier = seeds
    for h, k in enumerate(fanouts):
        chained = dev.sample(name, frontier, k, seed=91, call_counter=40 + h)
        want = orc.sample(og, name, frontier, k, seed=91, call_counter=40 + h)
        assert same(chained, want), h
        assert same(hops[h], want), h
        assert same([host(x) for x in dhops[h]], want), h
        frontier = want[0].reshape(-1)


# ------------------------------------------------------------------ the prefix path at the same k ---
# `timestamp > value` reads ONE value for the whole request, values[0] (Filter::FindkthLargest with batch_share_idx = 0;
# ts_prefix_of in csrc/glx_filter.hip): the reserved prefix of a row is the run of its timestamps below that value.  So
# every k has rows of its own whose timestamps straddle one threshold T(k) at a different position each.
PREFIX_HUB = 20000


def prefix_targets(k):
    """(row length, prefix length) of k's rows: 0, 1, k and all 2k + 1 slots of a short row; 1, k and all but 7 slots
    of a hub row."""
    return list(dict.fromkeys([(2 * k + 1, 0), (2 * k + 1, 1), (2 * k + 1, k), (2 * k + 1, 2 * k + 1),
                               (PREFIX_HUB, 1), (PREFIX_HUB, k), (PREFIX_HUB, PREFIX_HUB - 7)]))  # k = 1: 1 == k


def prefix_threshold(k):
    return (KS.index(k) + 1) * 10 ** 7


@pytest.fixture(scope="module")
def tsgraph(orc):
    """Timestamped graph (rows in timestamp-ascending order) holding prefix_targets(k) for every k of KS: a row whose
    prefix is c has c timestamps below prefix_threshold(k) and the others above it."""
    rng = np.random.default_rng(77)
    src, ts, rows = [], [], {}
    for k in KS:
        T = prefix_threshold(k)
        for n, c in prefix_targets(k):
            v = len(rows) * 7 + 3
            rows[(k, n, c)] = v
            src.append(np.full(n, v, np.int64))
            ts.append(np.concatenate([T - c + np.arange(c), T + 1 + np.arange(n - c)]).astype(np.int64))
    src, ts = np.concatenate(src), np.concatenate(ts)
    perm = rng.permutation(src.shape[0])  # insertion order: shuffled; the build sorts every row by timestamp
    src, ts = src[perm], ts[perm]
    dst = rng.integers(0, 5000, src.shape[0]).astype(np.int64)
    w = (rng.random(src.shape[0]) + 0.01).astype(np.float32)
    dev = glx.Graph.from_edges(src, dst, w, timestamp=ts)
    ids = np.array(list(rows.values()), np.int64)
    deg, col, eid = dev.sample_full(ids, 0)
    assert np.array_equal(deg, [n for (_, n, _) in rows])
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w[eid], ids=ids, ts_slot=ts[eid])
    yield og, dev, rows
    dev.close()


@pytest.mark.parametrize("k", KS, ids=["k%d" % k for k in KS])
def test_timestamp_prefix_samplers_at_every_kernel_boundary(orc, tsgraph, k):
    og, dev, rows = tsgraph
    rng = np.random.default_rng(500 + k)
    targets = prefix_targets(k)
    pattern = np.array([rows[(k, n, c)] for n, c in targets] + [999999], np.int64)  # + an unknown id
    B = batch_for(k)
    pick = np.tile(np.arange(pattern.shape[0]), B // pattern.shape[0] + 1)[:B][rng.permutation(B)]
    ids = pattern[pick]
    want_prefix = np.array([c for _, c in targets] + [0])[pick]
    vals = np.full(B, prefix_threshold(k), np.int64)
    ft, ff = glx.FILTER_LARGER_THAN, glx.FILTER_FIELD_TIMESTAMP
    flt = dict(type=ft, field=ff, values=vals)
    # the prefixes the device realises: FullSampler with replicate padding answers a row's prefix, then default slots
    deg, _, eid = dev.sample_full_filtered(ids, 0, ft, ff, vals, padding_mode=REPL, default_neighbor_id=-9)
    assert same((deg, eid), orc.sample_full_filtered(og, ids, 0, flt, padding_mode=REPL, default_neighbor_id=-9)[::2])
    seg = np.repeat(np.arange(B), deg)
    got_prefix = np.bincount(seg[eid != -1], minlength=B)
    assert np.array_equal(got_prefix, want_prefix)
    rr = rng.integers(0, 1 << 30, B).astype(np.int64)
    for name in (TOPK, RWOR):
        for pad in (CIRC, REPL):
            for retry in (0, 3):
                rows_ = rr if retry else None
                flt["retry_times"] = retry
                want = orc.sample_filtered(og, name, ids, k, flt, seed=13, call_counter=k, padding_mode=pad,
                                           default_neighbor_id=-9, rng_rows=rows_)
                got = dev.sample_filtered(name, ids, k, ft, ff, vals, seed=13, call_counter=k, padding_mode=pad,
                                          default_neighbor_id=-9, retry_times=retry, rng_rows=rows_)
                assert same(got, want), (name, pad, retry)
    for pad in (CIRC, REPL):
        want = orc.sample_full_filtered(og, ids, k, flt, padding_mode=pad, default_neighbor_id=-9)
        got = dev.sample_full_filtered(ids, k, ft, ff, vals, padding_mode=pad, default_neighbor_id=-9)
        assert same(got, want), ("FullSampler", pad)


# ------------------------------------------------- small weighted graphs: alignment, packing, alias ---
def weighted_rows(rng, degrees):
    """Weights with ties and zeros: every row mixes a few distinct values, some of them 0."""
    return rng.choice(np.array([0.0, 0.25, 0.5, 0.5, 1.0, 3.0, 0.125], np.float32), int(np.sum(degrees)))


def make_graph(orc, degrees, seed):
    rng = np.random.default_rng(seed)
    rp, col, eid = csr(degrees, rng, len(degrees))
    w = weighted_rows(rng, degrees)
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w, alias=orc.alias_build(rp, w))
    og["indeg_alias"] = orc.in_degree_alias(og)[0]
    return og


def device_graph(og):
    g = glx.Graph(og["row_ptr"], og["col"], og["eid"], og["weight"])
    g.enable_in_degree()
    return g


def _offset_outputs_check(backend):
    """Every slot-kernel sampler at even and odd k into outputs that start 8 bytes past a 16-byte boundary, against the
    oracle and the same call into fresh outputs; the elements on either side of the outputs stay untouched.
    backend: "torch" (device pointers: the kernel writes at the offset), "pinned" (numpy buffers in a range registered
    with glx_host_register: the kernel writes straight into them, at the offset), "numpy" (pageable: staged through an
    aligned device workspace; only the host copy lands at the offset)."""
    import torch
    orc = Oracle()
    og = make_graph(orc, [0, 1, 2, 3, 5, 8, 17, 40, 97, 300], seed=5)
    dev = device_graph(og)
    L, owners = glx.lib(), []

    def buffer(n):
        if backend == "torch":
            buf = torch.full((n + 4,), -111, dtype=torch.int64, device="cuda")
            return buf, (1 if buf.data_ptr() % 16 == 0 else 2)
        if backend == "numpy":
            buf = np.full(n + 4, -111, np.int64)
        else:  # whole pages of an anonymous mapping of its own, never a range of the malloc heap (include/glx.h)
            span = ((n + 4) * 8 + 4095) // 4096 * 4096
            gran = 2 << 20
            mm = mmap.mmap(-1, span + gran, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
            raw = np.frombuffer(mm, np.uint8)
            o = (-raw.ctypes.data) % gran
            buf = raw[o:o + (n + 4) * 8].view(np.int64)
            assert L.glx_host_register(ctypes.c_void_p(buf.ctypes.data), span) == 0, L.glx_last_error()
            owners.append((mm, raw, buf))
            buf[...] = -111
        return buf, (1 if buf.ctypes.data % 16 == 0 else 2)

    q = np.concatenate([np.arange(10), [10, -1], np.arange(10)[::-1]]).astype(np.int64)
    B = q.shape[0]
    src = cuda(q) if backend == "torch" else q
    for name, pad in ((RANDOM, CIRC), (EDGE_WEIGHT, CIRC), (IN_DEGREE, CIRC), (TOPK, CIRC), (RWOR, REPL),
                      (EDGE_WEIGHT, REPL)):
        for k in (1, 2, 7, 8, 33, 64):
            want = orc.sample(og, name, q, k, seed=3, call_counter=k, padding_mode=pad, default_neighbor_id=-5)
            n = B * k
            (bn, on), (be, oe) = buffer(n), buffer(n)
            views = (bn[on:on + n].reshape(B, k), be[oe:oe + n].reshape(B, k))
            for v in views:
                assert (v.data_ptr() if backend == "torch" else v.ctypes.data) % 16 == 8
            aligned = dev.sample(name, src, k, seed=3, call_counter=k, padding_mode=pad, default_neighbor_id=-5)
            got = dev.sample(name, src, k, seed=3, call_counter=k, padding_mode=pad, default_neighbor_id=-5, out=views)
            if backend == "torch":
                torch.cuda.synchronize()
            assert same([host(x) for x in got], want), (name, pad, k)
            assert same([host(x) for x in aligned], want), (name, pad, k)
            for buf, off in ((host(bn), on), (host(be), oe)):
                assert (buf[:off] == -111).all() and (buf[off + n:] == -111).all(), (name, pad, k)
    dev.close()
    for _, _, b in owners:
        assert L.glx_host_unregister(ctypes.c_void_p(b.ctypes.data)) == 0
    print("OFFSET_OUTPUTS_OK")


@pytest.mark.parametrize("backend", ["numpy", "pinned", "torch"])
def test_slot_samplers_into_outputs_offset_by_one_element(backend):
    """The pair store of glx_sample_slots_kernel is one 16-byte store when the pair's address is 16-byte aligned and two
    8-byte stores otherwise: outputs that start 8 bytes past a 16-byte boundary take the second form for every pair
    (device pointers and pinned host buffers; pageable host buffers are staged).  Pinned buffers are registered in a
    process of their own (this file as a script), like tests/test_gpu_host_stage.py's."""
    if backend != "pinned":
        _offset_outputs_check(backend)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "pinned"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "OFFSET_OUTPUTS_OK" in r.stdout, r.stdout[-3000:]


PACK_CASES = {
    # edge ids of slots 0 and 1 of the 3rd row; the rest are small
    "int32_max_min": (INT32_MAX, INT32_MIN),
    "int32_max_plus_1": (INT32_MAX + 1, 5),
    "int32_min_minus_1": (5, INT32_MIN - 1),
}


def _pack_graph(orc, case):
    degrees = [4, 1, 30, 0, 130, 7]
    rng = np.random.default_rng(11)
    rp, col, _ = csr(degrees, rng, len(degrees))
    eid = np.arange(rp[-1], dtype=np.int64) * 3 + 1000
    w = weighted_rows(rng, degrees)
    w[rp[2]:rp[2] + 2] = 3.0  # the slots that carry the edge-id bounds are drawn often
    if case == "partner_only":
        # row 4: the only edge id beyond int32 sits on the heavy slot that every light slot of the row names as its
        # alias partner, so most draws that return it come through a partner field.  That slot's own record holds the
        # id too (every partner is some slot's own record): this case cannot tell the two range checks apart.
        s, e = rp[4], rp[5]
        w[s:e] = 0.5
        w[s + 77] = 40.0
        eid[s + 77] = INT32_MAX + 12
    elif case != "no_pack_env":
        eid[rp[2]], eid[rp[2] + 1] = PACK_CASES[case]
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w, alias=orc.alias_build(rp, w))
    og["indeg_alias"] = orc.in_degree_alias(og)[0]
    if case == "partner_only":
        partners, light = og["alias"][1][s:e], og["alias"][0][s:e] < 1.0
        assert light.sum() > 50 and (partners[light] == 77).all()
    return og


@pytest.mark.parametrize("case", list(PACK_CASES) + ["partner_only", "no_pack_env"])
def test_edge_weight_records_packed_and_unpacked(orc, case, monkeypatch):
    """Packed {prob, own (nbr, eid), partner (nbr, eid)} records need every edge id in int32 range
    (glx_pack_ew_kernel); beyond it, or with GLX_EW_PACKED=0 at creation, the alias-table kernel serves EdgeWeight.
    Either way the draws are the oracle's, and so are InDegree's (which never packs)."""
    og = _pack_graph(orc, case)
    if case == "no_pack_env":
        monkeypatch.setenv("GLX_EW_PACKED", "0")
    dev = device_graph(og)
    monkeypatch.delenv("GLX_EW_PACKED", raising=False)
    assert dev.edge_weight_packed() == (case == "int32_max_min"), case  # the kernel that serves EdgeWeight
    prob, alias = dev.export_alias()
    assert np.array_equal(prob.view(np.uint32), og["alias"][0].view(np.uint32))
    assert np.array_equal(alias, og["alias"][1])
    q = np.tile(np.arange(7, dtype=np.int64), 40)
    for name in (EDGE_WEIGHT, IN_DEGREE):
        for k in (1, 6, 31):
            for pad in (CIRC, REPL):
                want = orc.sample(og, name, q, k, seed=8, call_counter=k, padding_mode=pad, default_neighbor_id=-2)
                got = dev.sample(name, q, k, seed=8, call_counter=k, padding_mode=pad, default_neighbor_id=-2)
                assert same(got, want), (name, k, pad)
    if case != "no_pack_env":  # the ids beyond int32 are in the answers
        big = og["eid"][(og["eid"] > INT32_MAX - 1) | (og["eid"] < INT32_MIN + 1)]
        got = dev.sample(EDGE_WEIGHT, np.full(400, 2 if case != "partner_only" else 4, np.int64), 16, seed=1)[1]
        assert np.isin(big, got).all()
    dev.close()


ALIAS_DEGREES = [95, 96, 97, 192, 193, 1, 0, 64]


def test_alias_build_around_the_lane_per_row_limit(orc):
    """kAliasLaneRowMax = 96: rows of up to 96 slots are built by one lane, longer ones by a wave.  Zero weights and
    ties in every row; one row of 97 all-zero weights (NaN probabilities, compared bit for bit)."""
    degrees = ALIAS_DEGREES + [97]
    rng = np.random.default_rng(12)
    rp, col, eid = csr(degrees, rng, len(degrees))
    w = weighted_rows(rng, degrees)
    w[rp[-2]:] = 0.0
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w, alias=orc.alias_build(rp, w))
    og["indeg_alias"] = orc.in_degree_alias(og)[0]
    dev = device_graph(og)
    prob, alias = dev.export_alias()
    assert np.array_equal(prob.view(np.uint32), og["alias"][0].view(np.uint32))
    assert np.array_equal(alias, og["alias"][1])
    q = np.tile(np.arange(len(degrees) + 1, dtype=np.int64), 60)
    for name in (EDGE_WEIGHT, IN_DEGREE):
        for k in (3, 40):
            want = orc.sample(og, name, q, k, seed=4, call_counter=k, default_neighbor_id=-2)
            got = dev.sample(name, q, k, seed=4, call_counter=k, default_neighbor_id=-2)
            assert same(got, want), (name, k)
    dev.close()


def filter_graph(orc, rows, seed):
    """rows: list of (others, hits) -- `hits` parallel edges to id 7 and `others` distinct other neighbours (some
    of them repeated across rows, so in-degrees tie).  Timestamped and weighted with zeros and ties."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for v, (others, hits) in enumerate(rows):
        d = np.concatenate([np.full(hits, 7, np.int64), rng.integers(100, 100 + 3 * others + 5, others)])
        src.append(np.full(d.shape[0], v * 5 + 1, np.int64))
        dst.append(d)
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(src.shape[0])
    src, dst = src[perm], dst[perm]
    w = weighted_rows(rng, [src.shape[0]])
    ts = rng.permutation(src.shape[0]).astype(np.int64)
    dev = glx.Graph.from_edges(src, dst, w, timestamp=ts)
    dev.enable_in_degree()
    ids = np.arange(len(rows), dtype=np.int64) * 5 + 1
    deg, col, eid = dev.sample_full(ids, 0)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w[eid], ids=ids, ts_slot=ts[eid])
    og["indeg_weight"] = orc.in_degree_alias(og)[1]
    return og, dev, ids


@pytest.mark.parametrize("dedup", [0, 1], ids=["per_row", "shared"])
def test_filtered_alias_build_around_the_lane_per_row_limit(orc, dedup):
    """id == value filters: EdgeWeight / InDegree rebuild the alias table over the reserved list (the survivors) of
    every row with a hit -- one lane per list of up to 96 entries, one wave above.  Survivor counts 95, 96, 97, 192,
    193 with 1 and 3 hits; filter_dedup_min_rows on (1: rows of one (vertex, value) pair share a table) and off."""
    rows = [(m, h) for m in (95, 96, 97, 192, 193) for h in (1, 3)] + [(40, 0), (0, 2)]
    og, dev, ids = filter_graph(orc, rows, 31)
    q = np.tile(ids, 6)
    vals = np.full(q.shape[0], 7, np.int64)
    flt = dict(type=glx.FILTER_EQUAL, field=glx.FILTER_FIELD_ID, values=vals)
    try:
        glx.tune("filter_dedup_min_rows", dedup)
        for name in (EDGE_WEIGHT, IN_DEGREE):
            for k in (2, 33):
                want = orc.sample_filtered(og, name, q, k, flt, seed=6, call_counter=k, default_neighbor_id=-4)
                got = dev.sample_filtered(name, q, k, glx.FILTER_EQUAL, glx.FILTER_FIELD_ID, vals, seed=6,
                                          call_counter=k, default_neighbor_id=-4)
                assert same(got, want), (name, k)
    finally:
        glx.tune("filter_dedup_min_rows", -1)
        dev.close()


# ---------------------------------------------------------------- filtered fast-path edges ---
@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "id_index"])
def test_id_equal_fast_paths_around_max_hits_and_max_k(orc, indexed):
    """kMaxHits = 8 hit positions are listed by one ballot scan when there is no id index (more go the general path);
    RWoR's fast path holds k <= kFastMaxK = 32.  Rows with 7, 8 and 9 parallel hits among 0, 1, 30 and 60 others."""
    rows = [(o, h) for h in (7, 8, 9) for o in (0, 1, 30, 60)] + [(45, 1), (33, 0)]
    og, dev, ids = filter_graph(orc, rows, 41 + indexed)
    if indexed:
        dev.enable_id_index()
    rng = np.random.default_rng(3)
    q = np.concatenate([np.tile(ids, 5), [999999]]).astype(np.int64)
    vals = np.full(q.shape[0], 7, np.int64)
    vals[::7] = og["col"][og["row_ptr"][1]]  # some rows filter another id
    rr = rng.permutation(q.shape[0]).astype(np.int64)
    flt = dict(type=glx.FILTER_EQUAL, field=glx.FILTER_FIELD_ID, values=vals)
    for name in (RWOR, TOPK):
        for k in (31, 32, 33):
            for pad in (CIRC, REPL):
                for rows_ in (None, rr):
                    want = orc.sample_filtered(og, name, q, k, flt, seed=2, call_counter=k, padding_mode=pad,
                                               default_neighbor_id=-4, rng_rows=rows_)
                    got = dev.sample_filtered(name, q, k, glx.FILTER_EQUAL, glx.FILTER_FIELD_ID, vals, seed=2,
                                              call_counter=k, padding_mode=pad, default_neighbor_id=-4, rng_rows=rows_)
                    assert same(got, want), (name, k, pad, rows_ is not None)
    dev.close()


# ---------------------------------------------------------------------- rows beyond 2^24 ---
HUGE = (1 << 24) + 5       # deg - 1 = 2^24 + 4: floats are 2 apart there, so the cast picks even slots only
NEAR = (1 << 24) - 3
# Between 2^24 and 2^25 the cast of a variate below deg - 1 cannot round past deg - 1, and deg - 1 is reached exactly
# here.  These cases say nothing about rows longer than 2^25: there, when deg - 1 is 3 mod 4, the cast can round up to
# deg, one slot past the row (glx_alias_pick, the packed pick in glx_sample_slots_kernel, and the oracle alike).
# Contract streams (seed 1, call counter 1) whose draw 1 on the HUGE row casts to exactly deg - 1 = 2^24 + 4 (the
# last slot) and whose RWoR step 1 swaps with the last slot: r_1 = 1 + bounded(u_1, deg - 1) = deg - 1.
EDGE_ROWS = (8266838, 12589417)


@pytest.fixture(scope="module")
def huge(orc, monkeypatch_module):
    """Rows of 2^24 + 5 and 2^24 - 3 weighted slots and one of 3; packed EdgeWeight records and, built with
    GLX_EW_PACKED=0, the alias-table kernel.  Weights are multiples of 2^-6 below 16 (so the device sums a long row in
    parallel, exactly), the last slot of each long row weighs 0."""
    rng = np.random.default_rng(2 ** 24)
    degrees = [HUGE, NEAR, 3]
    rp = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    E = int(rp[-1])
    col = rng.integers(0, 1000, E).astype(np.int64)
    eid = np.arange(E, dtype=np.int64)
    w = (rng.integers(0, 1000, E) / 64.0).astype(np.float32)
    w[rp[1] - 1] = 0.0
    w[rp[2] - 1] = 0.0
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w, alias=orc.alias_build(rp, w))
    packed = glx.Graph(rp, col, eid, w)
    monkeypatch_module.setenv("GLX_EW_PACKED", "0")
    plain = glx.Graph(rp, col, eid, w)
    monkeypatch_module.delenv("GLX_EW_PACKED")
    yield og, packed, plain
    packed.close()
    plain.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def test_huge_rows_alias_tables(huge):
    og, packed, plain = huge
    assert packed.edge_weight_packed() and not plain.edge_weight_packed()
    for dev in (packed, plain):
        prob, alias = dev.export_alias()
        assert np.array_equal(prob.view(np.uint32), og["alias"][0].view(np.uint32))
        assert np.array_equal(alias, og["alias"][1])


def test_huge_rows_edge_weight_draws_reach_the_last_slot(orc, huge):
    og, packed, plain = huge
    # the planted streams do cast to the last slot (and that slot's probability is 0: the draw takes its alias)
    for r in EDGE_ROWS:
        u = orc.draw64(1, 1, r, 1)
        rnd = np.float32(((u >> 11) * 2.0 ** -53) * float(HUGE - 1))
        assert int(rnd) == HUGE - 1
    assert og["alias"][0][HUGE - 1] == 0.0
    rng = np.random.default_rng(5)
    q = np.concatenate([np.zeros(1024, np.int64), np.ones(256, np.int64), [2, 3]])
    rr = rng.integers(0, 1 << 31, q.shape[0]).astype(np.int64)
    rr[[7, 500]] = EDGE_ROWS
    for k in (64, 3):
        want = orc.sample(og, EDGE_WEIGHT, q, k, seed=1, call_counter=1, rng_rows=rr)
        last = og["alias"][1][HUGE - 1]
        assert want[1][7, 1] == og["eid"][last] and want[1][500, 1] == og["eid"][last]
        for dev in (packed, plain):
            got = dev.sample(EDGE_WEIGHT, q, k, seed=1, call_counter=1, rng_rows=rr)
            assert same(got, want), k


def test_huge_rows_random_topk_rwor(orc, huge):
    og, packed, _ = huge
    rng = np.random.default_rng(6)
    q = np.concatenate([np.zeros(512, np.int64), np.ones(512, np.int64)])
    rr = rng.integers(0, 1 << 31, q.shape[0]).astype(np.int64)
    rr[[3, 100]] = EDGE_ROWS
    want = orc.sample(og, RANDOM, q, 64, seed=1, call_counter=1, rng_rows=rr)
    assert same(packed.sample(RANDOM, q, 64, seed=1, call_counter=1, rng_rows=rr), want)
    few = np.ascontiguousarray(q[::64])
    for pad in (CIRC, REPL):
        want = orc.sample(og, TOPK, few, 70, padding_mode=pad)
        assert same(packed.sample(TOPK, few, 70, padding_mode=pad), want)
    # RWoR: the planted streams swap the last slot in at step 1; the LDS kernel past 64 KiB at k = 5462
    q = np.array([0, 1, 0, 0, 1, 2, 0, 1], np.int64)
    rr = np.array([EDGE_ROWS[0], 4, EDGE_ROWS[1], 9, EDGE_ROWS[0], 1, 77, 123456], np.int64)
    for k in (25, 5462):
        want = orc.sample(og, RWOR, q, k, seed=1, call_counter=1, rng_rows=rr)
        assert want[1][0, 1] == og["eid"][HUGE - 1] and want[1][2, 1] == og["eid"][HUGE - 1]
        got = packed.sample(RWOR, q, k, seed=1, call_counter=1, rng_rows=rr)
        assert same(got, want), k


if __name__ == "__main__":
    _offset_outputs_check(sys.argv[1])
