"""gl.TemporalNeighborLoader end to end: a timestamped TSV source with a directed=False heterogeneous history type ->
the store -> glx_sample_temporal_hops per role, against the numpy restatement of the contract (tests/temporal_ref.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "graph-learn_amd"), os.path.join(ROOT, "graph-learn_amd", "python"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import temporal_ref as tr  # noqa: E402
from oracle_bindings import Oracle  # noqa: E402

pytestmark = pytest.mark.gpu

USERS, ITEMS, ITEM0 = 23, 17, 1000  # users 0 .. 22 (user 0 is real: the default neighbour id), items 1000 .. 1016
EVENTS, EDGE_DIM = 300, 3
FANOUTS = [4, 3]
BATCH = 64
SEED = 4242
ROLES = ("src", "dst", "neg")


def _events():
    rng = np.random.default_rng(9)
    src = rng.integers(0, USERS, EVENTS).astype(np.int64)
    dst = (ITEM0 + rng.integers(0, ITEMS, EVENTS)).astype(np.int64)
    t = rng.integers(-40, 120, EVENTS).astype(np.int64)  # many ties, in no order
    x = (rng.integers(-8, 9, (EVENTS, EDGE_DIM)) * 0.25).astype(np.float32)  # exact in the file's decimals
    return src, dst, t, x


def _csr(row_ids, nbr_ids, t):
    """the timestamp-ascending CSR the store builds: rows = distinct ids, ties in insertion order, edge id = index"""
    ids = np.unique(row_ids)
    order = np.lexsort((np.arange(len(t)), t, row_ids))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(ids, row_ids), minlength=len(ids)))])
    return dict(row_ptr=row_ptr.astype(np.int64), col=nbr_ids[order], eid=order.astype(np.int64), ts=t[order], ids=ids)


@pytest.fixture(scope="module")
def gl():
    import graphlearn
    return graphlearn


@pytest.fixture(scope="module")
def world(gl, tmp_path_factory):
    from graphlearn import settings
    before = dict(settings._MIRROR)  # pylint: disable=protected-access
    gl.set_default_neighbor_id(0)
    gl.set_default_timestamp(-1)
    gl.set_default_float_attribute(0.0)
    gl.set_sampling_seed(SEED)
    d = str(tmp_path_factory.mktemp("temporal"))
    src, dst, t, x = _events()
    path = os.path.join(d, "inter")
    with open(path, "w") as f:
        f.write("src_id:int64\tdst_id:int64\ttimestamp:int64\tfeature:string\n")
        for s, d_, t_, x_ in zip(src, dst, t, x):
            f.write("%d\t%d\t%d\t%s\n" % (s, d_, t_, ":".join("%.2f" % v for v in x_)))
    dec = gl.Decoder(timestamped=True, attr_types=["float"] * EDGE_DIM)
    g = gl.Graph() \
        .edge(path, ("user", "item", "inter"), dec, directed=False) \
        .edge(path, ("user", "item", "oneway"), dec, directed=True) \
        .init()
    yield dict(g=g, src=src, dst=dst, t=t, x=x, out=_csr(src, dst, t), inn=_csr(dst, src, t), orc=Oracle())
    g.close()
    gl.set_default_neighbor_id(before["default_neighbor_id"])
    gl.set_default_timestamp(before["default_timestamp"])
    gl.set_default_float_attribute(before["default_float_attr"])
    gl.set_sampling_seed(before["sampling_seed"])


def _np(a):
    return a.cpu().numpy()


def _epoch(gl, w, strategy, **kw):
    loader = gl.TemporalNeighborLoader(w["g"], "inter", "inter", FANOUTS, BATCH, strategy=strategy, negatives=2, **kw)
    assert len(loader) == (EVENTS + BATCH - 1) // BATCH
    return list(loader)


@pytest.mark.parametrize("strategy", ("recent", "uniform"))
def test_batches_equal_the_restatement(gl, world, strategy):
    w = world
    batches = _epoch(gl, w, strategy, edge_columns=("timestamps",))
    order = np.lexsort((np.arange(EVENTS), w["t"]))  # ascending (t, edge id)
    assert np.array_equal(np.concatenate([_np(b.eid) for b in batches]), order)
    assert np.array_equal(np.concatenate([_np(b.t) for b in batches]), w["t"][order])
    assert np.array_equal(np.concatenate([_np(b.src) for b in batches]), w["src"][order])
    assert np.array_equal(np.concatenate([_np(b.dst) for b in batches]), w["dst"][order])
    host_neg = w["g"].negative_sampler("inter", 2, "random")
    graphs = {"src": [w["out"], w["inn"]], "dst": [w["inn"], w["out"]], "neg": [w["inn"], w["out"]]}
    code = tr.RECENT if strategy == "recent" else tr.UNIFORM
    for i, b in enumerate(batches):
        # negatives: what the host's "random" negative sampler draws under the pinned call counter
        host_neg.set_call_counter(i)
        assert np.array_equal(_np(b.neg_dst), np.asarray(host_neg.get(_np(b.src)).ids).reshape(-1, 2))
        assert np.isin(_np(b.neg_dst), w["dst"]).all()
        t = _np(b.t)
        seeds = {"src": (_np(b.src), t), "dst": (_np(b.dst), t), "neg": (_np(b.neg_dst).reshape(-1), np.repeat(t, 2))}
        for r, role in enumerate(ROLES):
            ids, cut = seeds[role]
            want = tr.sample_temporal_hops(graphs[role], ids, cut, FANOUTS, code, False, SEED, (i * 3 + r) * len(FANOUTS),
                                           0, -1, orc=w["orc"])
            for h in range(len(FANOUTS)):
                blk = b.block(role, h)
                for name, a, ref in zip(("nbr", "eid", "ts", "cnt"), (blk.nbr, blk.eid, blk.ts, blk.cnt), want[h]):
                    assert np.array_equal(_np(a), ref), (i, role, h, name)
                nbr, eid, ts, cnt, cutoff = (_np(a) for a in (blk.nbr, blk.eid, blk.ts, blk.cnt, blk.cutoff))
                assert np.array_equal(cutoff, cut)
                valid = eid >= 0
                assert np.array_equal(valid, np.arange(FANOUTS[h])[None, :] < cnt[:, None])
                # no leak: every sampled edge happened strictly before its row's cutoff, and it IS that edge
                assert (ts[valid] < np.broadcast_to(cutoff[:, None], ts.shape)[valid]).all()
                assert np.array_equal(w["t"][eid[valid]], ts[valid])
                assert np.array_equal(_np(blk.rel_t), np.where(valid, cutoff[:, None] - ts, 0))
                # the edges' attributes and columns by edge id; a slot without an edge answers the defaults
                assert np.array_equal(_np(blk.edge_x), np.where(valid[..., None], w["x"][np.maximum(eid, 0)], np.float32(0)))
                assert np.array_equal(_np(blk.edge_cols["timestamps"]), np.where(valid, ts, -1))
                # ragged: the valid slots only, row after row
                rows, reid, rts, counts, at = b.ragged(role, h, with_positions=True)
                assert np.array_equal(_np(rows), nbr[valid]) and np.array_equal(_np(reid), eid[valid])
                assert np.array_equal(_np(rts), ts[valid]) and np.array_equal(_np(counts), cnt)
                assert np.array_equal(_np(at), np.flatnonzero(valid.reshape(-1)))
                assert len(b.ragged(role, h)) == 4
                cut = ts.reshape(-1)
    assert any((_np(b.block("src", 0).cnt) < FANOUTS[0]).any() for b in batches)  # short histories are in
    assert any((_np(b.block("src", 0).cnt) == FANOUTS[0]).any() for b in batches)


def test_an_epoch_repeats_bit_for_bit_and_the_next_differs(gl, world):
    import torch
    first = gl.TemporalNeighborLoader(world["g"], "inter", "inter", FANOUTS, BATCH, strategy="uniform", negatives=2)
    again = gl.TemporalNeighborLoader(world["g"], "inter", "inter", FANOUTS, BATCH, strategy="uniform", negatives=2)
    a, b, a_next = list(first), list(again), list(first)
    same_next = True
    for x, y, z in zip(a, b, a_next):
        assert torch.equal(x.neg_dst, y.neg_dst)
        same_next = same_next and torch.equal(x.neg_dst, z.neg_dst)
        for role in ROLES:
            for h in range(len(FANOUTS)):
                p, q, n = x.block(role, h), y.block(role, h), z.block(role, h)
                for name in ("nbr", "eid", "ts", "cnt", "rel_t", "edge_x"):
                    assert torch.equal(getattr(p, name), getattr(q, name)), (role, h, name)
                same_next = same_next and torch.equal(p.eid, n.eid)
    assert not same_next  # epoch 1 draws from other streams


def test_events_given_as_arrays_and_an_inclusive_cutoff(gl, world):
    w = world
    pick = np.array([5, 200, 17, 17, 120], np.int64)
    ev = (w["src"][pick], w["dst"][pick], w["t"][pick], pick)
    loader = gl.TemporalNeighborLoader(w["g"], ev, "inter", [12], 4, inclusive=True, edge_features=False, drop_last=True)
    batches = list(loader)
    assert len(batches) == 1 and batches[0].neg_dst.shape == (4, 0) and batches[0].blocks["neg"] == []
    order = np.lexsort((pick, w["t"][pick]))[:4]
    b = batches[0]
    assert np.array_equal(_np(b.eid), pick[order])
    blk = b.block("src", 0)
    assert blk.edge_x is None and blk.edge_cols is None
    want = tr.sample_temporal(w["out"], w["src"][pick][order], w["t"][pick][order], 12, tr.RECENT, True, SEED, 0, 0, -1)
    assert np.array_equal(_np(blk.nbr), want[0]) and np.array_equal(_np(blk.cnt), want[3])
    assert (_np(blk.eid) == pick[order][:, None]).any(axis=1).sum() >= 1  # inclusive: an event may see itself


def test_a_history_without_its_twin_is_refused(gl, world):
    with pytest.raises(ValueError) as e:
        gl.TemporalNeighborLoader(world["g"], "oneway", "oneway", [3], 8)
    assert "oneway_reverse" in str(e.value)
    with pytest.raises(ValueError):
        gl.TemporalNeighborLoader(world["g"], "inter", "inter", [3], 8, strategy="latest")


def test_transformer_conv_runs_on_a_batch(gl, world):
    import torch
    from graphlearn.nn.pytorch import TransformerConv
    torch.manual_seed(0)
    batch = _epoch(gl, world, "recent")[2]
    rows, _, _, counts, at = batch.ragged("src", 0, with_positions=True)
    blk = batch.block("src", 0)
    x = torch.randn(USERS + ITEMS, 8, device="cuda", requires_grad=True)  # users, then items
    edge = torch.cat([blk.edge_x.reshape(-1, EDGE_DIM)[at], torch.cos(blk.rel_t.reshape(-1)[at].float())[:, None]], dim=1)
    conv = TransformerConv(8, 4, heads=2, edge_dim=EDGE_DIM + 1).cuda()
    out = conv(x, batch.src, USERS + rows - ITEM0, counts, edge)
    assert out.shape == (batch.src.shape[0], 8) and bool(torch.isfinite(out).all())
    out.square().sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and bool((x.grad != 0).any())
    assert bool((conv.lin_edge.weight.grad != 0).any())
