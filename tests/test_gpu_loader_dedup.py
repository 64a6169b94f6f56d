"""gl.NeighborLoader(..., dedup=True): the same sample as the plain loader, delivered over the batch's distinct node
set (glx_unique) -- one feature row per distinct node, hop edges in node-set positions, one node set per node type."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

USERS, ITEMS = 150, 90  # user ids 0 .. 149, item ids 1000 .. 1089


def _write(d):
    rng = np.random.default_rng(12)
    users, items = os.path.join(d, "users"), os.path.join(d, "items")
    with open(users, "w") as fo:
        fo.write("id:int64\tfeature:string\n")
        for v in range(USERS):
            fo.write("%d\t%s\n" % (v, ":".join("%.9g" % a for a in rng.standard_normal(4))))
    with open(items, "w") as fo:
        fo.write("id:int64\tfeature:string\n")
        for v in range(ITEMS):
            fo.write("%d\t%s\n" % (1000 + v, ":".join("%.9g" % a for a in rng.standard_normal(3))))
    u2u, u2i, i2u = os.path.join(d, "u2u"), os.path.join(d, "u2i"), os.path.join(d, "i2u")
    with open(u2u, "w") as fo:
        fo.write("src_id:int64\tdst_id:int64\tweight:float\n")
        for v in range(USERS):
            for step in (1, 2, 7, 40):  # a few hubs on top: everybody also points at users 0 .. 2
                fo.write("%d\t%d\t%f\n" % (v, (v + step) % USERS, 0.1 + (v % 9) / 10.0))
            fo.write("%d\t%d\t%f\n" % (v, v % 3, 2.0))
    with open(u2i, "w") as fo:
        fo.write("src_id:int64\tdst_id:int64\tweight:float\n")
        for v in range(USERS):
            for step in (0, 5, 11):
                fo.write("%d\t%d\t%f\n" % (v, 1000 + (v + step) % ITEMS, 0.5 + step / 10.0))
    with open(i2u, "w") as fo:
        fo.write("src_id:int64\tdst_id:int64\tweight:float\n")
        for v in range(ITEMS):
            for step in (3, 4):
                fo.write("%d\t%d\t%f\n" % (1000 + v, (v * step) % USERS, 1.0 + step))
    return users, items, u2u, u2i, i2u


@pytest.fixture(scope="module")
def gl():
    import graphlearn
    return graphlearn


@pytest.fixture(scope="module")
def g(gl, tmp_path_factory):
    users, items, u2u, u2i, i2u = _write(str(tmp_path_factory.mktemp("dedup_data")))
    graph = gl.Graph() \
        .node(users, "user", gl.Decoder(attr_types=["float"] * 4)) \
        .node(items, "item", gl.Decoder(attr_types=["float"] * 3)) \
        .edge(u2u, ("user", "user", "u2u"), gl.Decoder(weighted=True)) \
        .edge(u2i, ("user", "item", "u2i"), gl.Decoder(weighted=True)) \
        .edge(i2u, ("item", "user", "i2u"), gl.Decoder(weighted=True)) \
        .init()
    yield graph
    graph.close()


def _first_occurrence_unique(ids):
    u, first = np.unique(ids, return_index=True)
    return u[np.argsort(first, kind="stable")]


def test_homogeneous_compact_batches(gl, g):
    import torch
    kw = dict(batch_size=40, strategy="edge_weight", shuffle=True)
    plain = list(gl.NeighborLoader(g, "user", ["u2u", "u2u"], [5, 3], **kw))
    compact = list(gl.NeighborLoader(g, "user", ["u2u", "u2u"], [5, 3], dedup=True, **kw))
    assert len(plain) == len(compact) == 4  # 150 users: 40 + 40 + 40 + 30
    for a, b in zip(plain, compact):
        assert isinstance(a, gl.NeighborBatch) and not isinstance(a, gl.CompactBatch)
        assert isinstance(b, gl.CompactBatch) and b.num_hops == 2
        # the sample itself is bit-identical
        assert torch.equal(a.seeds, b.seeds)
        for h in range(2):
            assert torch.equal(a.nbr[h], b.nbr[h]) and torch.equal(a.eid[h], b.eid[h])
        # the node set: distinct, seeds first, first-occurrence order, prefix per frontier
        stream = np.concatenate([a.frontier(h).cpu().numpy() for h in range(3)])
        nodes = b.nodes.cpu().numpy()
        np.testing.assert_array_equal(nodes, _first_occurrence_unique(stream))
        assert nodes.shape[0] < stream.shape[0]  # hubs repeat
        bs = a.seeds.shape[0]
        assert torch.equal(b.nodes[:bs], b.seeds)
        upto = b.num_nodes_upto.cpu().numpy()
        assert upto[0] == bs and upto[-1] == nodes.shape[0]
        at = 0
        for h in range(3):
            at += a.frontier(h).numel()
            np.testing.assert_array_equal(nodes[:upto[h]], _first_occurrence_unique(stream[:at]))
            # positions and rows
            assert tuple(b.local[h].shape) == ((bs,) if h == 0 else tuple(a.nbr[h - 1].shape))
            assert torch.equal(b.nodes[b.local[h].reshape(-1)], a.frontier(h))
            assert tuple(b.x_nodes.shape) == (nodes.shape[0], 4)
            assert torch.equal(b.x_nodes[b.local[h].reshape(-1)].view(torch.int32), a.x[h].view(torch.int32)), h
        for h in range(2):
            src, dst = b.edge_index(h)
            k = a.nbr[h].shape[1]
            assert torch.equal(b.nodes[src], a.frontier(h).repeat_interleave(k))
            assert torch.equal(b.nodes[dst], a.frontier(h + 1))
            psrc, pdst = a.edge_index(h)  # the plain batch's frontier-local COO names the same edges
            assert torch.equal(a.frontier(h)[psrc], b.nodes[src]) and torch.equal(a.frontier(h + 1)[pdst], b.nodes[dst])


def test_second_epoch_and_default_are_untouched(gl, g):
    import torch
    la = gl.NeighborLoader(g, "user", ["u2u"], [4], batch_size=64, shuffle=True)
    lb = gl.NeighborLoader(g, "user", ["u2u"], [4], batch_size=64, shuffle=True, dedup=True)
    for epoch in range(2):
        for a, b in zip(list(la), list(lb)):
            assert torch.equal(a.seeds, b.seeds) and torch.equal(a.nbr[0], b.nbr[0]) and torch.equal(a.eid[0], b.eid[0])
            assert b.x is None and a.x is not None
            assert torch.equal(b.x_nodes[b.local[1].reshape(-1)].view(torch.int32), a.x[1].view(torch.int32))


def test_two_type_meta_path_keeps_one_node_set_per_type(gl, g):
    """user -u2i-> item -i2u-> user: frontiers 0 and 2 share the user set, frontier 1 has the item set."""
    import torch
    kw = dict(batch_size=50, strategy="edge_weight", shuffle=True)
    plain = list(gl.NeighborLoader(g, "user", ["u2i", "i2u"], [3, 2], **kw))
    compact = list(gl.NeighborLoader(g, "user", ["u2i", "i2u"], [3, 2], dedup=True, **kw))
    assert len(plain) == len(compact) == 3
    for a, b in zip(plain, compact):
        assert b.types == ["user", "item", "user"]
        assert sorted(b.nodes) == ["item", "user"] and sorted(b.x_nodes) == ["item", "user"]
        assert torch.equal(a.seeds, b.seeds)
        for h in range(2):
            assert torch.equal(a.nbr[h], b.nbr[h]) and torch.equal(a.eid[h], b.eid[h])
        users = np.concatenate([a.frontier(0).cpu().numpy(), a.frontier(2).cpu().numpy()])
        items = a.frontier(1).cpu().numpy()
        np.testing.assert_array_equal(b.nodes["user"].cpu().numpy(), _first_occurrence_unique(users))
        np.testing.assert_array_equal(b.nodes["item"].cpu().numpy(), _first_occurrence_unique(items))
        assert (b.nodes["item"] >= 1000).all() and (b.nodes["user"] < 1000).all()
        upto = b.num_nodes_upto.cpu().numpy()
        assert upto[0] == a.seeds.shape[0]
        assert upto[1] == b.nodes["item"].shape[0] and upto[2] == b.nodes["user"].shape[0]
        assert tuple(b.x_nodes["user"].shape) == (b.nodes["user"].shape[0], 4)
        assert tuple(b.x_nodes["item"].shape) == (b.nodes["item"].shape[0], 3)
        for h in range(3):
            t = b.types[h]
            assert b.nodes_of(h) is b.nodes[t]
            assert torch.equal(b.nodes[t][b.local[h].reshape(-1)], a.frontier(h))
            assert torch.equal(b.x_nodes[t][b.local[h].reshape(-1)].view(torch.int32), a.x[h].view(torch.int32)), h
        for h in range(2):
            src, dst = b.edge_index(h)
            k = a.nbr[h].shape[1]
            assert torch.equal(b.nodes_of(h)[src], a.frontier(h).repeat_interleave(k))
            assert torch.equal(b.nodes_of(h + 1)[dst], a.frontier(h + 1))


def test_without_features(gl, g):
    b = next(iter(gl.NeighborLoader(g, "user", ["u2u"], [4], batch_size=32, with_features=False, dedup=True)))
    assert b.x_nodes is None and b.nodes.is_cuda and b.local[1].shape == b.nbr[0].shape
