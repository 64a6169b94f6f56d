"""A two-head TransformerConv layer with attention dropout and edge features on RAGGED full-neighbour hops.

    python examples/train_transformer_conv.py [epochs] [vertices]            (needs one GPU)

The layer of the reference's GPU PyTorch model (graphlearn/examples/pytorch/tgn/train_and_eval.py:38-50:
TransformerConv(in, out // 2, heads=2, dropout=0.1, edge_dim=...)) as graphlearn.nn.pytorch.TransformerConv: the
query, key and value maps once per distinct node, the edge map once per sampled edge, then ONE fused kernel going
forward for the scaled dot products of every seed with its whole neighbourhood, the softmax over each seed's own
neighbours, dropout 0.1 on the coefficients and the weighted sum of the values (dot_attention) -- neither
`k[index] + edge` nor `v[index] + edge` is ever materialised.  TGN's memory module, message store and temporal loader
are not part of this example: the graph is a small static one with a float attribute per edge.

The seeds come from gl.NeighborLoader(..., edge_features=True) over a one-neighbour hop, which also puts the edge
type's float attributes in HBM; the loader's hops have a fixed fan-out, so the full-neighbour hop itself is the device
graph's sample_full, and its edges' features are gathered by edge id from the table the loader gathers from.

The dropout mask is a function of (seed, step, position, head) -- the engine's contract generator, not the device's
-- and no backward uses a float atomic, so a (seed, epoch, batch) triple reproduces its loss bit for bit: main()
trains twice from one seed, prints both runs' per-batch losses as bits and exits non-zero if they differ.
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

import torch  # noqa: E402
import graphlearn as gl  # noqa: E402
import glx  # noqa: E402
from graphlearn.nn.pytorch import TransformerConv, gather_rows  # noqa: E402

CLASSES, DIM, EDGE_DIM, DEG = 5, 16, 4, 12
BATCH, HEADS, DROPOUT = 512, 2, 0.1
MAX_LIMIT = 0  # every neighbour


def write_sources(directory, vertices):
    """vertices of CLASSES classes with noisy class centres as features; a vertex has 1 .. 2 DEG - 1 out-edges, most of
    them inside its class, and an edge's attributes say (noisily) whether it stays inside the class"""
    rng = np.random.default_rng(0)
    label = rng.integers(0, CLASSES, vertices)
    centers = rng.standard_normal((CLASSES, DIM)) * 0.35
    feats = centers[label] + rng.standard_normal((vertices, DIM))
    by_class = [np.flatnonzero(label == c) for c in range(CLASSES)]
    npath, epath = os.path.join(directory, "node"), os.path.join(directory, "edge")
    with open(npath, "w") as f:
        f.write("id:int64\tlabel:int64\tfeature:string\n")
        for v in range(vertices):
            f.write("%d\t%d\t%s\n" % (v, label[v], ":".join("%.4f" % x for x in feats[v])))
    with open(epath, "w") as f:
        f.write("src_id:int64\tdst_id:int64\tfeature:string\n")
        for v in range(vertices):
            deg = int(rng.integers(1, 2 * DEG))
            same = rng.random(deg) < 0.7
            dst = np.where(same, rng.choice(by_class[label[v]], deg), rng.integers(0, vertices, deg))
            attr = np.where(label[dst] == label[v], 1.0, -1.0)[:, None] + rng.standard_normal((deg, EDGE_DIM))
            f.writelines("%d\t%d\t%s\n" % (v, d, ":".join("%.4f" % x for x in a)) for d, a in zip(dst, attr))
    return npath, epath


class ConvTransformer(torch.nn.Module):
    """z = relu(enc(x)) per distinct node; a two-head TransformerConv over each seed's whole neighbourhood with the
    edges' attributes in key and value; a linear classifier on the seed's own row next to the layer's output"""

    def __init__(self, dim, hidden, classes, heads=HEADS):
        super().__init__()
        assert hidden % heads == 0
        self.enc = torch.nn.Linear(dim, hidden)
        self.conv = TransformerConv(hidden, hidden // heads, heads=heads, dropout=DROPOUT, edge_dim=EDGE_DIM)
        self.out = torch.nn.Linear(2 * hidden, classes)

    def forward(self, x_nodes, local0, local, deg, edge_attr):
        z = torch.relu(self.enc(x_nodes))                                           # [M, hidden], M distinct nodes
        h = torch.relu(self.conv(z, local0, local, deg, edge_attr))                 # [S, hidden]
        return self.out(torch.cat([gather_rows(z, local0), h], dim=1))


def main(epochs=1, vertices=20000, quiet=False):
    """two runs from one seed -> ([run][epoch] = (losses, accuracy), whether the two runs' losses are the same bits)"""
    # the dense layers' own backward must not use atomics either (split-K GEMMs), or the loss would not reproduce
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        paths = write_sources(tempfile.mkdtemp(prefix="glx_transformer_conv_"), vertices)
        runs = [_train(paths, epochs, quiet, run) for run in range(2)]
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    same = all(float(a).hex() == float(b).hex() for (la, _), (lb, _) in zip(*runs) for a, b in zip(la, lb))
    if not quiet:
        print("the two runs' losses are %s" % ("the same bits" if same else "NOT the same bits"))
    return runs, same


def _train(paths, epochs, quiet, run):
    npath, epath = paths
    gl.set_padding_mode(gl.CIRCULAR)
    gl.set_sampling_seed(7)
    torch.manual_seed(0)  # the parameters' initial values AND the seed of the dropout masks
    g = gl.Graph() \
        .node(npath, "n", gl.Decoder(labeled=True, attr_types=["float"] * DIM)) \
        .edge(epath, ("n", "n", "e"), gl.Decoder(attr_types=["float"] * EDGE_DIM)) \
        .init()
    loader = gl.NeighborLoader(g, "n", ["e"], [1], batch_size=BATCH, strategy="random", shuffle=True,
                               with_features=False, node_columns=("labels",), edge_features=True)
    csr, feats, edge_feats = g.device_graph("e"), g.device_features("n"), g.device_edge_features("e")
    model = ConvTransformer(DIM, 64, CLASSES).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    history = []
    for epoch in range(epochs):
        t0, seen, correct, losses, longest = time.time(), 0, 0, [], 0
        model.train()
        for batch in loader:  # one epoch: every vertex once, in random order
            seeds = batch.seeds
            deg, nbr, eid = csr.sample_full(seeds, MAX_LIMIT)                       # the ragged full-neighbour hop
            nodes, (local0, local), _ = glx.unique([seeds, nbr])
            logits = model(feats.lookup(nodes), local0, local, deg, edge_feats.lookup(eid))
            labels = batch.y.long()
            loss = torch.nn.functional.cross_entropy(logits, labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
            seen += labels.shape[0]
            correct += int((logits.argmax(1) == labels).sum())
            losses.append(float(loss.detach()))
            longest = max(longest, int(deg.max()))
        half = len(losses) // 2
        history.append((losses, correct / seen))
        if not quiet:
            print("run %d epoch %d: loss %.4f -> %.4f (first / second half of the epoch), accuracy %.3f, %d vertices in "
                  "%.2f s, longest neighbourhood %d, %d dropout masks drawn, bits %s"
                  % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), correct / seen, seen, time.time() - t0,
                     longest, model.conv.calls, ",".join(float(x).hex() for x in losses)))
    g.close()
    return history


if __name__ == "__main__":
    _, same = main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
    sys.exit(0 if same else 1)
