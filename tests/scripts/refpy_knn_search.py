"""Run with the STAGED reference Python layer on the path (tests/refpy.py env()).  The reference's own Graph.search
(python/graph.py, python/operator/knn_operator.py) on this engine's pywrap_graphlearn: set_knn_metric, an IndexOption
with name "knn" on a node source, KnnOption(k) -- for both metrics, against the contract's restatement (tests/knn_ref.py);
a type loaded without the option is the reference's invalid-argument error; two graphs in sequence with the same type
name search their own tables.
usage: refpy_knn_search.py <work dir>"""
import os
import sys

import numpy as np

import graphlearn as gl
from graphlearn.python.errors import InvalidArgumentError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import knn_ref  # noqa: E402

work = sys.argv[1]
D, K = 6, 5


def write_nodes(name, ids, X):
    path = os.path.join(work, name)
    with open(path, "w") as f:
        f.write("id:int64\tattrs:string\n")
        for i, row in zip(ids, X):
            f.write("%d\t%s\n" % (i, ":".join(repr(float(v)) for v in row)))  # repr of a float32's double round-trips
    return path


def knn_option():
    opt = gl.IndexOption()
    opt.name = "knn"
    opt.index_type = "flat"
    return opt


def check(g, node_type, Q, X, ids, metric):
    gl.set_knn_metric(metric)
    got_ids, got_dist = g.search(node_type, Q, gl.KnnOption(k=K))
    want = knn_ref.search(Q, X, K, metric, ids=ids)
    assert got_ids.shape == (Q.shape[0], K) and got_dist.shape == (Q.shape[0], K)
    assert knn_ref.same((got_ids, got_dist), want), (metric, got_ids, want[0])


rng = np.random.default_rng(2)
ids_a = (1000 + 7 * rng.permutation(200)).astype(np.int64)
X_a = (rng.integers(-8, 9, (200, D)) / 4).astype(np.float32)
ids_b = np.arange(50, dtype=np.int64)
X_b = rng.standard_normal((50, D)).astype(np.float32)
Q = rng.standard_normal((9, D)).astype(np.float32)
dec = gl.Decoder(attr_types=["float"] * D)

g = gl.Graph() \
    .node(write_nodes("i_a", ids_a, X_a), node_type="i", decoder=dec, option=knn_option()) \
    .node(write_nodes("u_a", ids_b, X_b), node_type="u", decoder=dec)
g.init()
for metric in (0, 1, 0):
    check(g, "i", Q, X_a, ids_a, metric)
# a one-dimensional input is one query (knn_operator.py:47-53)
one_ids, one_dist = g.search("i", Q[0], gl.KnnOption(k=K))
assert knn_ref.same((one_ids, one_dist), knn_ref.search(Q[:1], X_a, K, 0, ids=ids_a))
try:
    g.search("u", Q, gl.KnnOption(k=K))  # loaded without the option: not indexed
except InvalidArgumentError as e:
    assert "Invalid node type" in str(e), e
else:
    raise AssertionError("a search on an unindexed type must fail")
g.close()

# a second graph in the same process, the same type name, another table: it searches its own rows
g2 = gl.Graph().node(write_nodes("i_b", ids_b, X_b), node_type="i", decoder=dec, option=knn_option())
g2.init()
for metric in (1, 0):
    check(g2, "i", Q, X_b, ids_b, metric)
g2.close()
print("KNN OK")
