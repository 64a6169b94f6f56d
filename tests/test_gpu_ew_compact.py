"""EdgeWeightSampler over the compact 20-byte records (csrc/glx_common.h GlxEwRec20, three to a 64-byte sector),
bit for bit against the same graph's 32-byte records (GLX_EW_PACKED=32), its alias tables (GLX_EW_PACKED=0) and the
oracle.

One small weighted graph whose row starts fall on every residue mod 3, with rows of 0, 1, 2 and 3 slots and rows of 96
and 97 slots (either side of the alias build's lane-per-row / wave-per-row limit).  It has 375 edges; two copies with
one and two more edges on the last row show the other two tail residues of the table.  Neighbour ids include negative
values, INT32_MAX and INT32_MIN; edge ids include INT32_MAX and INT32_MIN."""
import os
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

EDGE_WEIGHT, TOPK, IN_DEGREE = "EdgeWeightSampler", "TopkSampler", "InDegreeSampler"
CIRC, REPL = glx.PAD_CIRCULAR, glx.PAD_REPLICATE
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
DEGREES = [4, 1, 30, 0, 2, 130, 7, 3, 97, 96, 5]
KS = (1, 2, 5, 10, 25, 31)
EXTRA = (0, 1, 2)  # edges added to the last row: E = 375, 376, 377


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert glx.device_count() >= 1, "GPU tests need a HIP device; glx has no CPU fallback"


def same(got, want):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))


def host(pair):
    return tuple(x.cpu().numpy() if glx._is_torch(x) else x for x in pair)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_graph(orc, extra):
    degrees = DEGREES[:-1] + [DEGREES[-1] + extra]
    rng = np.random.default_rng(17)
    rp = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    E = int(rp[-1])
    assert E == 375 + extra and {int(s) % 3 for s in rp[:-1]} == {0, 1, 2}
    col = rng.integers(0, len(degrees), E).astype(np.int64)  # row indices, so hops chain
    eid = rng.permutation(E).astype(np.int64)
    # ids at the limits: on short rows, on the lane-built row of 96, on the wave-built rows of 97 and 130, and on the
    # last slots of the table
    col[rp[0]], col[rp[0] + 1], col[rp[0] + 2] = -1, INT32_MAX, INT32_MIN
    col[rp[1]] = INT32_MIN
    col[rp[5] + 129], col[rp[8] + 50], col[rp[9] + 95] = INT32_MAX, -7, INT32_MIN
    col[E - 1], col[E - 2] = INT32_MAX, -(2 ** 20)
    eid[rp[2]], eid[rp[2] + 1] = INT32_MAX, INT32_MIN
    eid[E - 1], eid[rp[7] + 2] = INT32_MAX - 1, INT32_MIN + 1
    w = rng.choice(np.array([0.0, 0.25, 0.5, 0.5, 1.0, 3.0, 0.125], np.float32), E)
    w[rp[0]:rp[0] + 3] = (1.0, 3.0, 0.5)  # the limit ids of rows 0 and 2 can be drawn
    w[rp[2]:rp[2] + 2] = (3.0, 3.0)
    og = dict(row_ptr=rp, col=col, eid=eid, weight=w, alias=orc.alias_build(rp, w))
    og["indeg_alias"] = orc.in_degree_alias(og)[0]
    return og


def device_graph(og, env, mp, in_degree=False):
    if env is None:
        mp.delenv("GLX_EW_PACKED", raising=False)
    else:
        mp.setenv("GLX_EW_PACKED", env)
    try:
        g = glx.Graph(og["row_ptr"], og["col"], og["eid"], og["weight"])
    finally:
        mp.delenv("GLX_EW_PACKED", raising=False)
    if in_degree:
        g.enable_in_degree()
    return g


@pytest.fixture(scope="module")
def graphs(orc):
    """extra -> (oracle graph, compact graph, 32-byte graph, alias-table graph)"""
    mp = pytest.MonkeyPatch()
    out = {}
    for extra in EXTRA:
        og = host_graph(orc, extra)
        out[extra] = (og, device_graph(og, None, mp, True), device_graph(og, "32", mp, True), device_graph(og, "0", mp))
    yield out
    mp.undo()
    for _, a, b, c in out.values():
        for g in (a, b, c):
            g.close()


def request():
    """280 rows: every row of the graph and one unknown id, over and over"""
    return np.resize(np.concatenate([np.arange(len(DEGREES)), [99]]).astype(np.int64), 280)


def test_env_values_pick_the_record(graphs):
    for extra in EXTRA:
        _, compact, rec32, plain = graphs[extra]
        assert compact.edge_weight_record_bytes() == 20 and compact.edge_weight_packed()
        assert rec32.edge_weight_record_bytes() == 32 and rec32.edge_weight_packed()
        assert plain.edge_weight_record_bytes() == 0 and not plain.edge_weight_packed()


@pytest.mark.parametrize("extra", EXTRA)
def test_draws_equal_the_32_byte_records_the_alias_tables_and_the_oracle(orc, graphs, extra):
    og, compact, rec32, plain = graphs[extra]
    q = request()
    dq = cuda(q)
    seen = []
    for k in KS:
        for pad in (CIRC, REPL):
            kw = dict(seed=11, call_counter=k, padding_mode=pad, default_neighbor_id=-2)
            want = orc.sample(og, EDGE_WEIGHT, q, k, **kw)
            for name, g in (("compact", compact), ("32", rec32), ("0", plain)):
                assert same(g.sample(EDGE_WEIGHT, q, k, **kw), want), (name, "host", k, pad)
                assert same(host(g.sample(EDGE_WEIGHT, dq, k, **kw)), want), (name, "device", k, pad)
            if pad == CIRC:
                seen.append(want)
    # the ids at the limits are in the answers, widened with their signs
    nbrs = np.concatenate([w[0].ravel() for w in seen])
    eids = np.concatenate([w[1].ravel() for w in seen])
    assert np.isin([-1, INT32_MAX, INT32_MIN], nbrs).all()
    assert np.isin([INT32_MAX, INT32_MIN], eids).all()


def test_ids_beyond_int32_fall_back(orc, graphs):
    """One neighbour id of 2^31 leaves the 32-byte records; one edge id beyond int32 leaves the alias tables."""
    mp = pytest.MonkeyPatch()
    q = request()
    try:
        for field, value, want_bytes in (("col", 2 ** 31, 32), ("col", INT32_MIN - 1, 32), ("eid", 2 ** 31, 0),
                                         ("eid", INT32_MIN - 1, 0)):
            og = dict(graphs[0][0])
            og[field] = og[field].copy()
            og[field][og["row_ptr"][5] + 64] = value  # the second lane pass of the wave that packs row 5
            g = device_graph(og, None, mp)
            try:
                assert g.edge_weight_record_bytes() == want_bytes, (field, value)
                assert g.edge_weight_packed() == (want_bytes != 0)
                for k in (2, 25):
                    kw = dict(seed=3, call_counter=k, default_neighbor_id=-2)
                    assert same(g.sample(EDGE_WEIGHT, q, k, **kw), orc.sample(og, EDGE_WEIGHT, q, k, **kw)), (field, k)
            finally:
                g.close()
    finally:
        mp.undo()


def test_in_degree_and_topk_never_read_the_records(orc, graphs):
    og, compact, rec32, _ = graphs[1]
    q = request()
    for name in (IN_DEGREE, TOPK):
        for k in (2, 10, 31):
            for pad in (CIRC, REPL):
                kw = dict(seed=5, call_counter=k, padding_mode=pad, default_neighbor_id=-2)
                got = compact.sample(name, q, k, **kw)
                assert same(got, rec32.sample(name, q, k, **kw)), (name, k, pad)
                assert same(got, orc.sample(og, name, q, k, **kw)), (name, k, pad)


def test_captured_plan_equals_the_direct_calls(graphs):
    import torch
    _, compact, rec32, _ = graphs[2]
    seeds = cuda(request())
    plan = glx.Plan([compact, compact], EDGE_WEIGHT, [5, 4], seeds.shape[0], seed=9, default_neighbor_id=-2)
    try:
        for run in range(2):
            hops = plan.run(seeds, call_counter=10 * run)
            hops = [{k: v.clone() for k, v in h.items()} for h in hops]
            torch.cuda.synchronize()
            for g in (compact, rec32):
                ref = glx.sample_hops([g, g], EDGE_WEIGHT, seeds, [5, 4], seed=9, call_counter=10 * run,
                                      default_neighbor_id=-2)
                torch.cuda.synchronize()
                for h in range(2):
                    assert torch.equal(hops[h]["nbr"], ref[h][0].view_as(hops[h]["nbr"])), (run, h)
                    assert torch.equal(hops[h]["eid"], ref[h][1].view_as(hops[h]["eid"])), (run, h)
            # the direct calls: hop h draws with call counter + h from the hop before's neighbours
            n1, e1 = compact.sample(EDGE_WEIGHT, seeds, 5, seed=9, call_counter=10 * run, default_neighbor_id=-2)
            n2, e2 = compact.sample(EDGE_WEIGHT, n1.view(-1), 4, seed=9, call_counter=10 * run + 1, default_neighbor_id=-2)
            torch.cuda.synchronize()
            for got, want in ((hops[0]["nbr"], n1), (hops[0]["eid"], e1), (hops[1]["nbr"], n2), (hops[1]["eid"], e2)):
                assert torch.equal(got, want.view_as(got)), run
    finally:
        plan.close()


def test_second_stream_gives_the_same_answers(orc, graphs):
    import torch
    og, compact, _, _ = graphs[0]
    q = request()
    dq = cuda(q)
    kw = dict(seed=21, call_counter=4, default_neighbor_id=-2)
    want = orc.sample(og, EDGE_WEIGHT, q, 10, **kw)
    first = compact.sample(EDGE_WEIGHT, dq, 10, **kw)
    side = torch.cuda.Stream(device=0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = compact.sample(EDGE_WEIGHT, dq, 10, **kw)
        side.synchronize()
    torch.cuda.synchronize()
    assert same(host(first), want) and same(host(other), want)
