"""glx.unique (glx_unique, csrc/glx_unique.hip): the distinct ids of a multi-part stream in first-occurrence order,
every element's position among them and the distinct count after each part -- exact equality against numpy on the
host throughout:

    u, first = np.unique(x, return_index=True)
    order = np.argsort(first, kind="stable")
    nodes = u[order]
    inverse = rank[np.searchsorted(u, x)]          # rank[order] = arange
    part_end[p] = np.count_nonzero(first < prefix_len[p + 1])
"""
import numpy as np
import pytest

import glx
import synth

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def reference(parts):
    x = np.concatenate([np.asarray(p, np.int64).reshape(-1) for p in parts]) if parts else np.empty(0, np.int64)
    u, first = np.unique(x, return_index=True)
    order = np.argsort(first, kind="stable")
    nodes = u[order]
    rank = np.empty(u.shape[0], np.int64)
    rank[order] = np.arange(u.shape[0])
    inverse = rank[np.searchsorted(u, x)]
    prefix = np.concatenate([[0], np.cumsum([np.asarray(p).size for p in parts])])
    part_end = np.array([np.count_nonzero(first < prefix[p + 1]) for p in range(len(parts))], np.int64)
    return nodes, inverse, part_end


def run(parts, where, stream=None, return_inverse=True):
    """-> (nodes, inverse over the whole stream or None, part_end) as numpy arrays."""
    import torch
    if where == "host":
        nodes, inv, part_end = glx.unique([np.ascontiguousarray(p, np.int64) for p in parts], return_inverse)
    else:
        dev = [torch.from_numpy(np.ascontiguousarray(p, np.int64)).cuda() for p in parts]
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                nodes, inv, part_end = glx.unique(dev, return_inverse)
            stream.synchronize()
        else:
            nodes, inv, part_end = glx.unique(dev, return_inverse)
        assert nodes.is_cuda and part_end.is_cuda
        nodes, part_end = nodes.cpu().numpy(), part_end.cpu().numpy()
        inv = [v.cpu().numpy() for v in inv] if inv is not None else None
    if inv is not None:
        for v, p in zip(inv, parts):
            assert v.shape == np.asarray(p).shape
        inv = np.concatenate([v.reshape(-1) for v in inv]) if inv else np.empty(0, np.int64)
    return nodes, inv, part_end


def check(parts, where, stream=None):
    nodes, inv, part_end = run(parts, where, stream)
    want_nodes, want_inv, want_end = reference(parts)
    assert nodes.dtype == np.int64 and inv.dtype == np.int64 and part_end.dtype == np.int64
    np.testing.assert_array_equal(part_end, want_end)
    np.testing.assert_array_equal(nodes, want_nodes)
    np.testing.assert_array_equal(inv, want_inv)


def zipf_ids(rng, n, span=1 << 50):
    """a few ids make up most of the stream"""
    return (rng.zipf(1.5, n).astype(np.uint64) % np.uint64(span)).astype(np.int64)


def splits(n):
    """part lengths for one stream of n ids: 1 to 4 parts, with empty first, middle and last parts"""
    a, b, c = n // 3, n // 2, (3 * n) // 4
    return [[n], [0, n], [n, 0], [a, n - a], [a, 0, n - a], [0, a, n - a, 0], [a, b - a, c - b, n - c], [0, 0, n]]


def cut(x, lens):
    at = np.concatenate([[0], np.cumsum(lens)])
    return [x[at[i]:at[i + 1]] for i in range(len(lens))]


SHAPE_NS = [0, 1, 63, 64, 65, 255, 256, 257, 65537, (1 << 20) + 3]


@pytest.mark.parametrize("where", ["host", "device", "stream"])
@pytest.mark.parametrize("n", SHAPE_NS)
def test_shapes(n, where):
    import torch
    rng = np.random.default_rng(n + 11)
    x = zipf_ids(rng, n)
    if n > 2:
        x[rng.integers(0, n, max(n // 4, 1))] = rng.integers(-(1 << 62), 1 << 62, max(n // 4, 1))
    stream = torch.cuda.Stream() if where == "stream" else None
    # the largest stream: three of the splits (every pointer kind still sees one, several and empty parts)
    for lens in (splits(n) if n < (1 << 20) else [splits(n)[0], splits(n)[5], splits(n)[6]]):
        check(cut(x, lens), "host" if where == "host" else "device", stream)


def test_multi_dimensional_parts_and_no_inverse():
    rng = np.random.default_rng(5)
    parts = [rng.integers(0, 500, 64), rng.integers(0, 500, (64, 5)), rng.integers(0, 500, (320, 3))]
    for where in ("host", "device"):
        check(parts, where)
        nodes, inv, part_end = run(parts, where, return_inverse=False)
        want = reference(parts)
        assert inv is None
        np.testing.assert_array_equal(nodes, want[0])
        np.testing.assert_array_equal(part_end, want[2])


def value_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    for n in (5000, 70001):
        cases["all_equal_%d" % n] = np.full(n, 42, np.int64)
        cases["all_equal_min_%d" % n] = np.full(n, I64_MIN, np.int64)
        cases["all_distinct_%d" % n] = rng.permutation(n).astype(np.int64) * 7919 - 3 * n
        cases["zipf_%d" % n] = zipf_ids(rng, n, 1 << 20)
        cases["negative_%d" % n] = -zipf_ids(rng, n, 1 << 45) - 1
        cases["mixed_sign_%d" % n] = rng.integers(-50, 50, n)
        cases["above_2_40_%d" % n] = (1 << 40) + rng.integers(0, 1 << 22, n) * (1 << 18)
        base = rng.integers(-(1 << 62), 1 << 62, n)
        base[rng.integers(0, n, n // 2)] = base[rng.integers(0, n, n // 2)]  # some repeats
        cases["extremes_absent_%d" % n] = base
        for name, value in (("min", I64_MIN), ("max", I64_MAX)):
            for place in ("first", "last", "middle", "many"):
                y = base.copy()
                if place == "first":
                    y[0] = value
                elif place == "last":
                    y[-1] = value
                elif place == "middle":
                    y[n // 2] = value
                else:
                    y[rng.integers(0, n, n // 10)] = value
                cases["%s_%s_%d" % (name, place, n)] = y
        both = base.copy()
        both[0], both[-1] = I64_MAX, I64_MIN
        both[rng.integers(1, n - 1, 100)] = I64_MIN
        both[rng.integers(1, n - 1, 100)] = I64_MAX
        both[rng.integers(1, n - 1, 100)] = I64_MIN + 1
        cases["min_and_max_%d" % n] = both
    # distinct counts just below and just above a power of two (and of the table's size steps)
    for m in (4095, 4096, 4097, 65535, 65537):
        ids = rng.permutation(1 << 20)[:m].astype(np.int64) - (1 << 19)
        cases["distinct_%d_thrice" % m] = np.concatenate([ids, rng.permutation(ids), ids[::-1]])
        cases["distinct_%d_once" % m] = ids
    return cases


VALUE_CASES = value_cases()


@pytest.mark.parametrize("name", sorted(VALUE_CASES))
def test_values(name):
    x = VALUE_CASES[name]
    n = x.shape[0]
    check([x], "device")
    check(cut(x, [n // 5, 0, n - n // 5]), "device")
    check(cut(x, [n // 2, n - n // 2]), "host")


def test_deterministic_across_runs_and_streams():
    """4.2 M ids over 150 K distinct ones, hub-heavy: inserts of one id race from many waves at once."""
    import torch
    rng = np.random.default_rng(77)
    n = (1 << 22) + 12345
    pool = rng.permutation(1 << 24)[:150000].astype(np.int64) * 1000003 - (1 << 40)
    x = pool[np.minimum(rng.zipf(1.3, n) - 1, rng.integers(0, pool.shape[0], n))]
    lens = [4096, 40960, n - 4096 - 40960]
    parts = [torch.from_numpy(p.copy()).cuda() for p in cut(x, lens)]
    runs = []
    for _ in range(5):
        nodes, inv, part_end = glx.unique(parts)
        runs.append((nodes.clone(), torch.cat([v.reshape(-1) for v in inv]).clone(), part_end.clone()))
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        nodes, inv, part_end = glx.unique(parts)
        runs.append((nodes.clone(), torch.cat([v.reshape(-1) for v in inv]).clone(), part_end.clone()))
    s2.synchronize()
    torch.cuda.synchronize()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    want = reference(cut(x, lens))
    for got, w in zip(runs[0], want):
        np.testing.assert_array_equal(got.cpu().numpy(), w)


def test_prefix_property():
    rng = np.random.default_rng(31)
    B = 1024
    seeds = rng.permutation(100000)[:B].astype(np.int64)  # distinct
    hop1 = rng.integers(0, 100000, (B, 10))
    hop1[:, 0] = seeds  # overlap with the seeds
    hop2 = zipf_ids(rng, B * 50, 100000).reshape(B * 10, 5)
    parts = [seeds, hop1, hop2]
    for where in ("host", "device"):
        nodes, inv, part_end = run(parts, where)
        np.testing.assert_array_equal(nodes[:B], seeds)
        assert part_end[0] == B and part_end[-1] == nodes.shape[0]
        for p in range(3):
            upto = reference(parts[:p + 1])[0]
            np.testing.assert_array_equal(nodes[:part_end[p]], upto)
        np.testing.assert_array_equal(nodes[inv], np.concatenate([q.reshape(-1) for q in parts]))


@pytest.fixture(scope="module")
def sampled_step():
    """RMAT graph (synth.py), a two-hop EdgeWeight sample of it and float32 features."""
    import torch
    V, E, D = 20000, 300000, 64
    row_ptr, col, eid, w = synth.rmat_graph_torch(V, E, 3, "cuda")
    g = glx.Graph(row_ptr, col, eid, w)
    X = synth.features_torch(V, D, 4, "cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    seeds = torch.randperm(V, generator=gen, device="cuda")[:512].contiguous()
    hops = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, [6, 4], seed=13, call_counter=2)
    frontiers = [seeds, hops[0][0], hops[1][0]]
    nodes, local, part_end = glx.unique(frontiers)
    return dict(X=X, frontiers=frontiers, nodes=nodes, local=local, part_end=part_end)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_real_step_lookup_through_the_node_set(sampled_step, dtype):
    import torch
    s = sampled_step
    f = glx.Features(s["X"], dtype=None if dtype == "float32" else dtype)
    assert f.dtype == dtype
    want = reference([t.cpu().numpy() for t in s["frontiers"]])
    np.testing.assert_array_equal(s["nodes"].cpu().numpy(), want[0])
    assert torch.equal(s["nodes"][:512], s["frontiers"][0])  # distinct seeds come first
    x_nodes = f.lookup(s["nodes"])
    for h, frontier in enumerate(s["frontiers"]):
        per_slot = f.lookup(frontier.reshape(-1))
        assert tuple(s["local"][h].shape) == tuple(frontier.shape)
        got = x_nodes[s["local"][h].reshape(-1)]
        assert torch.equal(got.view(torch.int32), per_slot.view(torch.int32)), h


@pytest.mark.parametrize("op", ["SumAggregator", "MeanAggregator", "MaxAggregator"])
def test_compact_batch_feeds_the_existing_reduce(sampled_step, op):
    """Features view over x_nodes (dense ids = node-set positions) + the local ids of frontier h + 1 == the reduce over
    the full table with the global ids, bit for bit: the compact batch needs no reduce code of its own."""
    import torch
    s = sampled_step
    f = glx.Features(s["X"])
    x_nodes = f.lookup(s["nodes"])
    compact = glx.Features(x_nodes, view=True)
    for h in range(2):
        rows = int(s["frontiers"][h].numel())
        emb_c, cnt_c = compact.aggregate(op, s["local"][h + 1].reshape(-1).contiguous(), None, rows)
        emb_g, cnt_g = f.aggregate(op, s["frontiers"][h + 1].reshape(-1).contiguous(), None, rows)
        assert torch.equal(cnt_c, cnt_g)
        assert torch.equal(emb_c.view(torch.int32), emb_g.view(torch.int32)), (op, h)


def test_small_call_after_a_large_one_reuses_the_arena():
    """The table lives in a grow-only workspace: a stale slot of the large call must not leak into the small one."""
    import torch
    rng = np.random.default_rng(8)
    big = torch.from_numpy(rng.integers(0, 3000, 1 << 20)).cuda()
    glx.unique([big])
    for n in (1, 100, 5000, 300000):
        x = rng.integers(0, 3000, n)  # the same id range as the large call
        check(cut(x, [n // 2, n - n // 2]), "device")
        glx.unique([big])
    host_big = rng.integers(-5, 5, 1 << 18)
    glx.unique([host_big])
    check([rng.integers(-5, 5, 77)], "host")
