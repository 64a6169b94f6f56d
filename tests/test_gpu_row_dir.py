"""The samplers' row directory (csrc/glx_common.h GlxRowDir: id -> (start, deg) in one load) against the lookup it
replaces (id map + row_ptr), bit for bit.  Every store is built twice from the same edges, once with GLX_ROW_DIR=0 and
once with the form under test; the answers are compared with torch.equal on canary-filled buffers.

The issue's first graph, source ids {0, 3, 4, 9, 64, 65, 1000}, is hashed16 by the rule it states (7 rows give the id
map 64 slots, i.e. 1,024 bytes, and 1,001 direct entries are 8,008): it runs as stated, under the name "gaps_1000", and
"gaps_direct" is the same graph with 100 in place of 1000, which is direct and has gaps."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "graph-learn_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import glx  # noqa: E402
import row_dir_layout as lay  # noqa: E402

pytestmark = pytest.mark.gpu

RANDOM, RWOR, EDGE_WEIGHT, TOPK = ("RandomSampler", "RandomWithoutReplacementSampler", "EdgeWeightSampler",
                                   "TopkSampler")
CIRC, REPL = glx.PAD_CIRCULAR, glx.PAD_REPLICATE
I64MAX, I64MIN = 2 ** 63 - 1, -2 ** 63
DEGREES = [4, 1, 30, 2, 130, 7, 3]
KS = (1, 2, 5, 10, 25)
KS_RWOR = KS + (16, 17, 32, 33, 64, 70)  # glx_rwor_small_kernel, glx_rwor_kernel<32>, <64>, and glx_rwor_lds_kernel
BATCHES = (1, 63, 64, 65, 257)
CANARY = -7777
CAP = 64  # the id map of a graph of up to 32 rows
WRAP = lay.colliding_ids(CAP, CAP - 1, 4, first=2 * CAP)  # three rows and one unknown id, all at home in slot cap - 1

# name -> (source ids, degrees, GLX_ROW_DIR of the build under test ("1": the rule), the form it must have)
GRAPHS = {
    "gaps_direct": ([0, 3, 4, 9, 64, 65, 100], DEGREES, "1", "direct"),
    "gaps_1000": ([0, 3, 4, 9, 64, 65, 1000], DEGREES, "1", "hashed16"),
    "gaps_direct_forced_hash": ([0, 3, 4, 9, 64, 65, 100], DEGREES, "hash", "hashed16"),
    "gaps_1000_forced_hash": ([0, 3, 4, 9, 64, 65, 1000], DEGREES, "hash", "hashed16"),
    "wide_ids": ([-5, 7, 2 ** 40, I64MAX - 1], [4, 30, 1, 70], "1", "hashed16"),
    "wrap": (WRAP[:3] + [5, 6], [3, 70, 5, 2, 9], "1", "hashed16"),
    "one_row": ([11], [5], "1", "direct"),
    "one_row_hash": ([11], [5], "hash", "hashed16"),
    "last_direct": ([0, 1, 2 * CAP - 1], [3, 1, 20], "1", "direct"),    # (max_id + 1) * 8 == cap * 16
    "first_hashed": ([0, 1, 2 * CAP], [3, 1, 20], "1", "hashed16"),      # one more
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert glx.device_count() >= 1, "GPU tests need a HIP device; glx has no CPU fallback"


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def edges_of(ids, degrees, seed=3):
    """(src, dst, weight) in insertion order: neighbours are source ids (so hops chain) and a few ids that are no row."""
    rng = np.random.default_rng(seed)
    src = np.repeat(np.asarray(ids, np.int64), degrees)
    pool = np.asarray(list(ids) + [ids[0] + 1, -9], np.int64)
    dst = pool[rng.integers(0, pool.shape[0], src.shape[0])]
    w = rng.choice(np.array([0.25, 0.5, 0.5, 1.0, 3.0, 0.125], np.float32), src.shape[0])
    return src, dst, w


def build(make, row_dir, ew=None):
    """make() under GLX_ROW_DIR=row_dir (None: unset) and GLX_EW_PACKED=ew; the knobs are read once per build."""
    mp = pytest.MonkeyPatch()
    try:
        for name, value in (("GLX_ROW_DIR", row_dir), ("GLX_EW_PACKED", ew)):
            if value is None:
                mp.delenv(name, raising=False)
            else:
                mp.setenv(name, value)
        return make()
    finally:
        mp.undo()


def pair_of(make, row_dir, form, ew=None):
    """-> (the store without a directory, the store with the form under test)"""
    plain, under_test = build(make, "0", ew), build(make, row_dir, ew)
    assert plain.row_dir() == (None, 0)
    assert under_test.row_dir()[0] == form
    return plain, under_test


def request_pool(ids):
    """Known ids, gaps inside [0, max_id], max_id and max_id + 1, negative ids, INT64_MIN, duplicates."""
    top = max(ids)
    pool = list(ids) + [top, min(top + 1, I64MAX), 1, 2, 5, 63, -1, -5, -6, I64MIN, I64MIN + 1, I64MAX, WRAP[3]]
    return np.asarray(pool + list(ids)[:2], np.int64)


def sample_into(g, sampler, q, k, **kw):
    import torch
    out = (torch.full((q.shape[0], k), CANARY, dtype=torch.int64, device="cuda"),
           torch.full((q.shape[0], k), CANARY, dtype=torch.int64, device="cuda"))
    g.sample(sampler, q, k, out=out, **kw)
    return out


def assert_same_answers(plain, under_test, ids, samplers, tag):
    import torch
    pool = request_pool(ids)
    for batch in BATCHES:
        q = cuda(np.resize(pool, batch))
        for sampler in samplers:
            for k in (KS_RWOR if sampler == RWOR else KS):
                for pad in (CIRC, REPL):
                    kw = dict(seed=13, call_counter=k, padding_mode=pad, default_neighbor_id=-2)
                    want = sample_into(plain, sampler, q, k, **kw)
                    got = sample_into(under_test, sampler, q, k, **kw)
                    torch.cuda.synchronize()
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (tag, batch, sampler, k, pad)
                    assert not (want[0] == CANARY).any() and not (want[1] == CANARY).any(), (tag, batch, sampler, k, pad)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_every_sampler_answers_as_without_a_directory(name):
    ids, degrees, env, form = GRAPHS[name]
    src, dst, w = edges_of(ids, degrees)
    cap = lay.capacity(len(ids))
    assert cap == CAP
    assert lay.FORM_NAMES[lay.form(len(ids), src.shape[0], min(ids), max(ids), cap, env)] == form  # the rule, restated
    plain, under_test = pair_of(lambda: glx.Graph.from_edges(src, dst, w), env, form)
    try:
        assert under_test.row_dir()[1] == lay.table_bytes(lay.form(len(ids), src.shape[0], min(ids), max(ids), cap, env),
                                                          max(ids), cap)
        assert_same_answers(plain, under_test, ids, (RANDOM, RWOR, EDGE_WEIGHT, TOPK), name)
        # the answers are not trivially equal: known rows answer with their neighbours, unknown ids with the default
        nbr, _ = sample_into(under_test, TOPK, cuda(np.asarray([ids[0], I64MIN, max(ids)], np.int64)), 2,
                             default_neighbor_id=-2)
        nbr = nbr.cpu().numpy()
        assert (nbr[1] == -2).all() and nbr[0, 0] in dst[src == ids[0]] and nbr[2, 0] in dst[src == max(ids)]
    finally:
        plain.close()
        under_test.close()


def test_wrap_graph_probes_round_the_end_of_the_table():
    """The premise of "wrap": its first three ids and the unknown request id are at home in the last slot."""
    assert [lay.home_slot(x, CAP) for x in WRAP] == [CAP - 1] * 4
    assert all(x >= 2 * CAP for x in WRAP)  # hashed16 by rule
    ids = GRAPHS["wrap"][0]
    t = lay.build_hashed16(ids, range(len(ids)), [1] * len(ids), CAP)
    assert sorted(lay.lookup(t, lay.HASHED16, x)[3] for x in WRAP[:3]) == [1, 2, 3]  # one of them sits in slot 1
    assert lay.lookup(t, lay.HASHED16, WRAP[3])[3] >= 4  # the unknown one walks past all three


@pytest.mark.parametrize("ew,record_bytes", [(None, 20), ("32", 32), ("0", 0)])
@pytest.mark.parametrize("row_dir,form,ids", [("1", "direct", GRAPHS["gaps_direct"][0]),
                                              ("hash", "hashed16", GRAPHS["gaps_direct"][0]),
                                              ("1", "hashed16", GRAPHS["wide_ids"][0])])
def test_edge_weight_records_of_every_size(ew, record_bytes, row_dir, form, ids):
    degrees = DEGREES[:len(ids)]
    src, dst, w = edges_of(ids, degrees, seed=9)
    dst = np.clip(dst, -2 ** 31, 2 ** 31 - 1)  # neighbour ids within int32, so the 20-byte records are built
    plain, under_test = pair_of(lambda: glx.Graph.from_edges(src, dst, w), row_dir, form, ew)
    try:
        assert plain.edge_weight_record_bytes() == under_test.edge_weight_record_bytes() == record_bytes
        assert_same_answers(plain, under_test, ids, (EDGE_WEIGHT,), (ew, form))
    finally:
        plain.close()
        under_test.close()


def csr_with_an_empty_row():
    """CSR-built: row ids in no order, one of them twice (the first row wins), and a KNOWN row without a slot."""
    ids = np.asarray([40, 7, 22, 7, 90], np.int64)
    degrees = [5, 0, 12, 3, 70]  # id 7 is row 1 (empty); row 3 is shadowed
    rp = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    E = int(rp[-1])
    rng = np.random.default_rng(2)
    col = ids[rng.integers(0, ids.shape[0], E)]
    eid = rng.permutation(E).astype(np.int64)
    w = rng.choice(np.array([0.5, 1.0, 3.0], np.float32), E)
    ts = np.concatenate([np.arange(d, dtype=np.int64) for d in degrees])  # ascending inside every row
    return ids, rp, col, eid, w, ts


@pytest.mark.parametrize("row_dir,form", [("1", "direct"), ("hash", "hashed16")])
def test_csr_graph_with_an_empty_known_row_and_a_prefix_call(row_dir, form):
    import torch
    ids, rp, col, eid, w, ts = csr_with_an_empty_row()

    def make():
        g = glx.Graph(rp, col, eid, w, ids=ids)
        g.set_timestamps(ts)
        return g

    plain, under_test = pair_of(make, row_dir, form)
    try:
        assert torch.equal(under_test.degrees(cuda(ids)), plain.degrees(cuda(ids)))
        assert plain.degrees(ids).tolist() == [5, 0, 12, 0, 70]
        assert_same_answers(plain, under_test, [int(x) for x in ids], (RANDOM, RWOR, EDGE_WEIGHT, TOPK), ("csr", form))
        # glx_sample_prefix_device (timestamp > value keeps a row prefix): Topk and RandomWithoutReplacement run the
        # plain kernels with a per-row prefix, which overrides the degree of KNOWN rows only
        pool = request_pool([int(x) for x in ids])
        for batch in (1, 65, 257):
            q = np.resize(pool, batch)
            values = np.resize(np.asarray([-1, 0, 2, 5, 100], np.int64), batch)
            dq, dv = cuda(q), cuda(values)
            for sampler in (TOPK, RWOR):
                for k in (1, 5, 17, 40, 70):
                    for pad in (CIRC, REPL):
                        kw = dict(seed=5, call_counter=k, padding_mode=pad, default_neighbor_id=-2)
                        want = plain.sample_filtered(sampler, dq, k, glx.FILTER_LARGER_THAN, glx.FILTER_FIELD_TIMESTAMP,
                                                     dv, **kw)
                        got = under_test.sample_filtered(sampler, dq, k, glx.FILTER_LARGER_THAN,
                                                         glx.FILTER_FIELD_TIMESTAMP, dv, **kw)
                        torch.cuda.synchronize()
                        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (form, batch, sampler, k, pad)
    finally:
        plain.close()
        under_test.close()


def test_unset_knob_is_the_default():
    """GLX_ROW_DIR unset is kRowDirDefaultOn (csrc/glx_common.h; tests/row_dir_layout.py DEFAULT_ON restates it)."""
    ids, degrees = GRAPHS["gaps_direct"][:2]
    src, dst, w = edges_of(ids, degrees)
    g = build(lambda: glx.Graph.from_edges(src, dst, w), None)
    try:
        assert g.row_dir() == (("direct", (max(ids) + 1) * 8) if lay.DEFAULT_ON else (None, 0))
    finally:
        g.close()


def test_dense_graph_keeps_no_directory():
    """No ids, no id map: raw id v is row v and row_ptr answers in one step already."""
    _, rp, col, eid, w, _ = csr_with_an_empty_row()
    g = glx.Graph(rp, col, eid, w)
    try:
        assert g.row_dir() == (None, 0)
    finally:
        g.close()


@pytest.mark.parametrize("row_dir,form", [("1", "direct"), ("hash", "hashed16")])
def test_captured_plan_equals_the_eager_calls(row_dir, form):
    import torch
    ids, degrees = GRAPHS["gaps_direct"][:2]
    src, dst, w = edges_of(ids, degrees)
    plain, under_test = pair_of(lambda: glx.Graph.from_edges(src, dst, w), row_dir, form)
    seeds = cuda(np.resize(request_pool(ids), 257))
    plan = glx.Plan([under_test, under_test], EDGE_WEIGHT, [5, 4], seeds.shape[0], seed=9, default_neighbor_id=-2)
    try:
        for run in range(2):
            hops = plan.run(seeds, call_counter=10 * run)
            hops = [{k: v.clone() for k, v in h.items()} for h in hops]
            torch.cuda.synchronize()
            for g in (under_test, plain):
                n1, e1 = g.sample(EDGE_WEIGHT, seeds, 5, seed=9, call_counter=10 * run, default_neighbor_id=-2)
                n2, e2 = g.sample(EDGE_WEIGHT, n1.view(-1), 4, seed=9, call_counter=10 * run + 1, default_neighbor_id=-2)
                torch.cuda.synchronize()
                for got, want in ((hops[0]["nbr"], n1), (hops[0]["eid"], e1), (hops[1]["nbr"], n2), (hops[1]["eid"], e2)):
                    assert torch.equal(got, want.view_as(got)), (form, run)
    finally:
        plan.close()
        plain.close()
        under_test.close()
