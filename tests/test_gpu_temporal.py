"""glx_sample_temporal / glx_sample_temporal_hops against the numpy restatement of their contract
(tests/temporal_ref.py), every (row, slot) of every output for equality.

One graph holds one row of every degree at which the search changes shape: the short rows the last round serves alone,
the (W + 1)^2 edges of every group width W in {8, 16, 32, 64} (81, 289, 1089, 4225 and their neighbours) and a
70,000-slot hub.  Timestamps are negative and positive with runs of ties of 1 .. 130 slots, so runs straddle probe
positions.  The graph is built in the three id forms the samplers look ids up in: the direct row directory, the hashed
one (GLX_ROW_DIR=hash at the build -- the knob is read once per build, so no child process is needed) and none (a
dense-id CSR handle)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "graph-learn_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import glx  # noqa: E402
import temporal_ref as tr  # noqa: E402
from oracle_bindings import Oracle  # noqa: E402

pytestmark = pytest.mark.gpu

DEGREES = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65,
           80, 81, 82, 288, 289, 290, 1088, 1089, 1090, 4224, 4225, 4226,
           70000]
IDS = [2 * r + 3 for r in range(len(DEGREES))]  # raw ids with gaps: 1, 4, 6, ... are no row
KS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 130)     # every group width, and the j += W loop
BATCHES = (0, 1, 63, 64, 65, 257)
FORMS = ("direct", "hashed16", "none")
SEED, CC = 0x5EED0123456789, (1 << 33) + 5
DEFAULT_ID, DEFAULT_TS = -3, -(1 << 50)
CANARY = -7777
UNKNOWN = {"ids": [-1, 1, 4, 2 * len(DEGREES) + 3, tr.I64_MIN, tr.I64_MAX],
           "dense": [-1, len(DEGREES), len(DEGREES) + 7, -2, tr.I64_MIN, tr.I64_MAX]}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert glx.device_count() >= 1, "GPU tests need a HIP device; glx has no CPU fallback"


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _requests(g):
    """(row index or -1 - u for unknown id number u, cutoff) of every request row, shuffled: for rows of at most 300
    slots every slot's timestamp and that +- 1; for longer rows the ends, 200 random positions and every tie-run
    boundary (every distinct value: strict cutoffs land on a run's start, inclusive ones on its end); INT64_MIN and
    INT64_MAX for every row; unknown ids.  A row appears many times with different cutoffs."""
    rng = np.random.default_rng(17)
    rows, cuts = [], []
    for r, d in enumerate(DEGREES):
        ts = g["ts"][g["row_ptr"][r]:g["row_ptr"][r + 1]]
        want = [np.array([tr.I64_MIN, tr.I64_MAX, 0], np.int64)]
        if 0 < d <= 300:
            want += [ts - 1, ts, ts + 1]
        elif d > 300:
            at = ts[rng.integers(0, d, 200)]
            want += [np.array([ts[0] - 1, ts[0], ts[0] + 1, ts[-1] - 1, ts[-1], ts[-1] + 1], np.int64), at - 1, at, at + 1,
                     np.unique(ts)]
        want = np.unique(np.concatenate(want))
        rows.append(np.full(want.shape[0], r, np.int64))
        cuts.append(want)
    some = np.concatenate(cuts)
    for u in range(len(UNKNOWN["ids"])):
        rows.append(np.full(3, -1 - u, np.int64))
        cuts.append(np.array([tr.I64_MAX, tr.I64_MIN, some[rng.integers(0, some.shape[0])]], np.int64))
    rows, cuts = np.concatenate(rows), np.concatenate(cuts)
    order = rng.permutation(rows.shape[0])
    return rows[order], cuts[order]


class World(object):
    """the numpy graph, its request rows, and the restatement's answers, computed once per (k, inclusive, strategy)"""

    def __init__(self):
        self.orc = Oracle()
        self.g = tr.build_graph(DEGREES, seed=1, ids=IDS)
        self.rows, self.cut = _requests(self.g)
        ids = np.asarray(IDS, np.int64)
        known = self.rows >= 0
        self.src = {
            "ids": np.where(known, ids[np.maximum(self.rows, 0)], np.asarray(UNKNOWN["ids"], np.int64)[np.maximum(-1 - self.rows, 0)]),
            "dense": np.where(known, self.rows, np.asarray(UNKNOWN["dense"], np.int64)[np.maximum(-1 - self.rows, 0)]),
        }
        self._want = {}
        self._graphs = {}

    def want(self, k, inclusive, strategy):
        key = (k, bool(inclusive), strategy)
        if key not in self._want:
            out = tr.sample_temporal(self.g, self.src["ids"], self.cut, k, strategy, inclusive, SEED, CC, DEFAULT_ID,
                                     DEFAULT_TS, orc=self.orc)
            for a in out:
                a.setflags(write=False)
            self._want[key] = out
        return self._want[key]

    def graph(self, form):
        if form not in self._graphs:
            g = self.g
            mp = pytest.MonkeyPatch()
            try:
                mp.delenv("GLX_ROW_DIR", raising=False)
                if form == "hashed16":
                    mp.setenv("GLX_ROW_DIR", "hash")
                dev = glx.Graph(g["row_ptr"], g["col"], g["eid"], ids=None if form == "none" else g["ids"])
            finally:
                mp.undo()
            assert dev.row_dir()[0] == (None if form == "none" else form)
            assert not dev.has_timestamps
            dev.set_timestamps(g["ts"])
            assert dev.has_timestamps
            self._graphs[form] = dev
        return self._graphs[form]

    def request(self, form):
        return self.src["dense" if form == "none" else "ids"], self.cut


@pytest.fixture(scope="module")
def world():
    return World()


def assert_equal(got, want, tag):
    for name, a, b in zip(("nbr", "eid", "ts", "cnt"), got, want):
        a = a.cpu().numpy() if glx._is_torch(a) else a  # pylint: disable=protected-access
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, name, a.dtype, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.shape[0] == 0, (tag, name, "first mismatch at", bad[0].tolist(), "of", bad.shape[0])


def test_request_rows_cover_what_they_claim(world):
    assert world.g["ts"].min() < 0 < world.g["ts"].max()
    long_ts = world.g["ts"][world.g["row_ptr"][-2]:]
    runs = np.diff(np.flatnonzero(np.concatenate([[True], long_ts[1:] != long_ts[:-1], [True]])))
    assert runs.min() == 1 and runs.max() >= 120 and long_ts.shape[0] == 70000
    assert (np.diff(world.g["ts"])[np.diff(np.repeat(np.arange(len(DEGREES)), DEGREES)) == 0] >= 0).all()
    start, c = tr.prefix_lengths(world.g, world.src["ids"], world.cut, False)
    hub = world.rows == len(DEGREES) - 1
    assert {0, 70000} <= set(c[hub].tolist()) and np.unique(c[hub]).shape[0] > 1000
    assert (world.rows < 0).sum() == 3 * len(UNKNOWN["ids"])
    assert world.rows.shape[0] < 20000


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("form", FORMS)
def test_every_row_and_slot(world, form, k):
    g = world.graph(form)
    src, cut = (cuda(a) for a in world.request(form))
    for strategy, name in ((tr.RECENT, "recent"), (tr.UNIFORM, "uniform")):
        for inclusive in (False, True):
            got = g.sample_temporal(src, cut, k, strategy=name, inclusive=inclusive, seed=SEED, call_counter=CC,
                                    default_neighbor_id=DEFAULT_ID, default_timestamp=DEFAULT_TS)
            assert_equal(got, world.want(k, inclusive, strategy), (form, k, name, inclusive))


@pytest.mark.parametrize("k", (1, 16, 32, 65))
def test_batch_sizes(world, k):
    """a whole number of groups per block, a block's last group, one group past it, several blocks"""
    g = world.graph("direct")
    src, cut = world.request("direct")
    for batch in BATCHES:
        for strategy, name in ((tr.RECENT, "recent"), (tr.UNIFORM, "uniform")):
            got = g.sample_temporal(cuda(src[:batch]), cuda(cut[:batch]), k, strategy=name, seed=SEED, call_counter=CC,
                                    default_neighbor_id=DEFAULT_ID, default_timestamp=DEFAULT_TS)
            want = tuple(a[:batch] for a in world.want(k, False, strategy))
            assert_equal(got, want, (batch, k, name))


def _raw_call(g, strategy, src, cut, k, nbr, eid, ts, cnt, kind):
    p = lambda a: None if a is None else glx._ptr(a)[0]  # noqa: E731  pylint: disable=protected-access
    glx._check(glx.lib().glx_sample_temporal(  # pylint: disable=protected-access
        g._h, strategy, p(src), p(cut), None, int(src.shape[0]), k, 0, DEFAULT_ID, DEFAULT_TS, SEED, CC, p(nbr), p(eid),
        p(ts), p(cnt), kind, glx._stream(kind, g.device)))  # pylint: disable=protected-access


@pytest.mark.parametrize("strategy", (tr.RECENT, tr.UNIFORM))
def test_optional_outputs_may_be_null_and_every_element_is_written(world, strategy):
    import torch
    g = world.graph("hashed16")
    src, cut = (a[:400] for a in world.request("hashed16"))
    k = 9
    want = tuple(a[:400] for a in world.want(k, False, strategy))
    for present in ((1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        # device pointers
        outs = [torch.full((400, k), CANARY, dtype=torch.int64, device="cuda") for _ in range(3)]
        outs.append(torch.full((400,), CANARY, dtype=torch.int32, device="cuda"))
        args = [outs[0]] + [o if keep else None for o, keep in zip(outs[1:], present)]
        _raw_call(g, strategy, cuda(src), cuda(cut), k, *args, kind=glx.PTR_DEVICE)
        torch.cuda.synchronize()
        for i, (o, keep) in enumerate(zip(outs, (1,) + present)):
            if keep:
                assert np.array_equal(o.cpu().numpy(), want[i]), (present, i)
            else:
                assert bool((o == CANARY).all()), (present, i)
        # host pointers
        houts = [np.full((400, k), CANARY, np.int64) for _ in range(3)] + [np.full(400, CANARY, np.int32)]
        args = [houts[0]] + [o if keep else None for o, keep in zip(houts[1:], present)]
        _raw_call(g, strategy, src.copy(), cut.copy(), k, *args, kind=glx.PTR_HOST)
        for i, (o, keep) in enumerate(zip(houts, (1,) + present)):
            assert np.array_equal(o, want[i]) if keep else (o == CANARY).all(), (present, i)


@pytest.mark.parametrize("form", FORMS)
def test_host_pointers_answer_what_device_tensors_answer(world, form):
    g = world.graph(form)
    src, cut = world.request(form)
    for strategy, name in ((tr.RECENT, "recent"), (tr.UNIFORM, "uniform")):
        got = g.sample_temporal(src.copy(), cut.copy(), 17, strategy=name, inclusive=True, seed=SEED, call_counter=CC,
                                default_neighbor_id=DEFAULT_ID, default_timestamp=DEFAULT_TS)
        assert all(isinstance(a, np.ndarray) for a in got)
        assert_equal(got, world.want(17, True, strategy), (form, name))


def test_two_calls_give_the_same_bits(world):
    import torch
    g = world.graph("direct")
    src, cut = (cuda(a) for a in world.request("direct"))
    for name in ("recent", "uniform"):
        a = g.sample_temporal(src, cut, 33, strategy=name, seed=SEED, call_counter=CC)
        b = g.sample_temporal(src, cut, 33, strategy=name, seed=SEED, call_counter=CC)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    u1 = g.sample_temporal(src, cut, 33, strategy="uniform", seed=SEED, call_counter=CC + 1)
    assert not torch.equal(u1[0], a[0])  # another call counter is another stream


@pytest.mark.parametrize("inclusive", (False, True))
def test_uniform_is_the_random_sampler_on_the_prefix_graph(world, inclusive):
    """bit for bit glx_sample(RANDOM) on the derived graph whose vertex i is request row i's prefix, under rng_rows"""
    import torch
    n = 160
    src, cut = (a[:n] for a in world.request("direct"))
    derived = tr.prefix_graph(world.g, src, cut, inclusive)
    assert derived["col"].shape[0] > 70000  # the hub's prefixes are in
    pg = glx.Graph(derived["row_ptr"], derived["col"], derived["eid"])
    streams = np.random.default_rng(5).permutation(1 << 20)[:n].astype(np.int64)
    g = world.graph("direct")
    for k in (1, 9, 17, 33, 130):
        nbr, eid, _, cnt = g.sample_temporal(cuda(src), cuda(cut), k, strategy="uniform", inclusive=inclusive, seed=SEED,
                                             call_counter=CC, default_neighbor_id=DEFAULT_ID, rng_rows=cuda(streams))
        rn, re = pg.sample("RandomSampler", cuda(np.arange(n, dtype=np.int64)), k, seed=SEED, call_counter=CC,
                           default_neighbor_id=DEFAULT_ID, rng_rows=cuda(streams))
        assert torch.equal(nbr, rn) and torch.equal(eid, re), k
        assert np.array_equal(cnt.cpu().numpy(), np.where(np.diff(derived["row_ptr"]) > 0, k, 0))
    pg.close()


def test_a_graph_without_timestamps_raises(world):
    g = world.g
    plain = glx.Graph(g["row_ptr"], g["col"], g["eid"], ids=g["ids"])
    assert not plain.has_timestamps
    src, cut = (cuda(a[:8]) for a in world.request("direct"))
    with pytest.raises(glx.GlxError) as e:
        plain.sample_temporal(src, cut, 4)
    assert e.value.code == 3 and "timestamps" in str(e.value)
    with pytest.raises(glx.GlxError) as e:
        glx.sample_temporal_hops([world.graph("direct"), plain], src, cut, [2, 2])
    assert e.value.code == 3 and "timestamps" in str(e.value)
    with pytest.raises(glx.GlxError):
        world.graph("direct").sample_temporal(src, cut, 0)  # k >= 1
    plain.close()


# ---- hops ------------------------------------------------------------------------------------------------------------
HOP_V = 48


@pytest.fixture(scope="module")
def hop_world():
    """two dense-id graphs over vertices 0 .. 47 whose neighbours are vertices; vertex 0 is real and has history (all of
    it before the default timestamp -1, so a default-filled slot taken for vertex 0 WOULD sample)"""
    rng = np.random.default_rng(23)
    out = []
    for seed in (31, 32):
        deg = rng.integers(0, 70, HOP_V)
        deg[0], deg[1] = 40, 0
        g = tr.build_graph(deg, seed=seed, num_dst=HOP_V)
        g["col"][rng.integers(0, g["col"].shape[0], 200)] = 0  # vertex 0 is sampled, too
        a, b = g["row_ptr"][0], g["row_ptr"][1]
        g["ts"][a:b] = np.sort(-rng.integers(5, 4000, b - a))
        dev = glx.Graph(g["row_ptr"], g["col"], g["eid"])
        dev.set_timestamps(g["ts"])
        out.append((g, dev))
    seeds = rng.integers(-1, HOP_V + 1, 70).astype(np.int64)
    cut = rng.integers(-500, 1500, 70).astype(np.int64)
    cut[:3] = [tr.I64_MAX, tr.I64_MIN, 0]
    return out, seeds, cut


@pytest.mark.parametrize("fanouts", ([3, 2], [10, 5]))
@pytest.mark.parametrize("name", ("recent", "uniform"))
def test_hops_equal_hand_chained_single_calls(hop_world, name, fanouts):
    import torch
    (ga, da), (gb, db) = hop_world[0]
    seeds, cut = hop_world[1], hop_world[2]
    strategy = tr.RECENT if name == "recent" else tr.UNIFORM
    kw = dict(strategy=name, seed=SEED, default_neighbor_id=0, default_timestamp=-1)
    got = glx.sample_temporal_hops([da, db], cuda(seeds), cuda(cut), fanouts, call_counter=CC, **kw)
    # by hand: hop 1's rows are hop 0's slots; a slot that holds no edge yields a default-filled row with cnt = 0
    n0, e0, t0, c0 = da.sample_temporal(cuda(seeds), cuda(cut), fanouts[0], call_counter=CC, **kw)
    n1, e1, t1, c1 = db.sample_temporal(n0.reshape(-1), t0.reshape(-1), fanouts[1], call_counter=CC + 1, **kw)
    dead = (torch.arange(fanouts[0], device="cuda")[None, :] >= c0[:, None]).reshape(-1)
    assert bool(dead.any()) and bool((c1[dead] > 0).any())  # vertex 0's history: the rule is not vacuous
    n1[dead], e1[dead], t1[dead], c1[dead] = 0, -1, -1, 0
    for h, hand in enumerate(((n0, e0, t0, c0), (n1, e1, t1, c1))):
        assert got[h][0].shape == (seeds.shape[0] * (fanouts[0] if h else 1), fanouts[h])
        assert all(torch.equal(x, y) for x, y in zip(got[h], hand)), (h, name)
    # and the restatement's hops rule
    want = tr.sample_temporal_hops([ga, gb], seeds, cut, fanouts, strategy, False, SEED, CC, 0, -1, orc=Oracle())
    for h in range(2):
        assert_equal(got[h], want[h], ("hop", h, name))
    # host pointers: one upload, the frontiers stay on the device, one download per output
    host = glx.sample_temporal_hops([da, db], seeds.copy(), cut.copy(), fanouts, call_counter=CC, **kw)
    for h in range(2):
        assert_equal(host[h], want[h], ("host hop", h, name))


def test_hops_with_an_empty_batch_and_three_hops(hop_world):
    (ga, da), (gb, db) = hop_world[0]
    seeds, cut = hop_world[1][:9], hop_world[2][:9]
    empty = glx.sample_temporal_hops([da, db], cuda(seeds[:0]), cuda(cut[:0]), [3, 2])
    assert [tuple(o[0].shape) for o in empty] == [(0, 3), (0, 2)]
    got = glx.sample_temporal_hops([da, db, da], cuda(seeds), cuda(cut), [4, 3, 2], strategy="recent", inclusive=True,
                                   seed=SEED, call_counter=CC)
    want = tr.sample_temporal_hops([ga, gb, ga], seeds, cut, [4, 3, 2], tr.RECENT, True, SEED, CC)
    for h in range(3):
        assert_equal(got[h], want[h], ("hop", h))
