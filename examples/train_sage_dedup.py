"""The GraphSAGE classifier of train_sage_pytorch.py with a learned encoder BELOW the aggregation, trained on compact
batches: one encoder pass per distinct node, differentiable segment reductions on top.

    python examples/train_sage_dedup.py [epochs] [vertices]            (needs one GPU)

gl.NeighborLoader(dedup=True, node_columns=("labels",)) yields the distinct nodes of a two-hop sample, ONE feature row
per node (batch.x_nodes) and every sampled slot's position in that set (batch.local[h]).  The model computes
z = relu(enc(x_nodes)) once per distinct node -- the point of the dedup -- and reads it back per slot through
graphlearn.nn.pytorch.segment_aggregate (hop 2, reduced to one row per hop-1 slot without the [n, D] gather) and
gather_rows (the slots' own rows).  Both go backward through glx_aggregate_backward: no float atomics, every element
of z.grad accumulated in ascending slot order, so a (seed, epoch, batch) triple reproduces its loss bit for bit --
which the `bits` this script prints let a caller check (torch's z[local] goes backward through index_add_ with float
atomics, in whatever order they land).

The graph is train_sage_pytorch.py's: classes that are hard to tell from a vertex's own 16 noisy features and easy from
its neighbourhood's.
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
from graphlearn.nn.pytorch import gather_rows, segment_aggregate  # noqa: E402

CLASSES, DIM, DEG = 5, 16, 12
FANOUT = (10, 5)
BATCH = 512


def write_sources(directory, vertices):
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
        f.write("src_id:int64\tdst_id:int64\n")
        for v in range(vertices):
            same = rng.random(DEG) < 0.8
            dst = np.where(same, rng.choice(by_class[label[v]], DEG), rng.integers(0, vertices, DEG))
            f.writelines("%d\t%d\n" % (v, d) for d in dst)
    return npath, epath


class DedupSage(torch.nn.Module):
    """z = relu(enc(x)) per distinct node; h1 = relu(W1 [z_v || mean z of v's sampled neighbours]) per hop-1 slot;
    h0 = relu(W2 [z_seed || mean h1 of the seed's slots]); a linear classifier on h0."""

    def __init__(self, dim, hidden, classes):
        super().__init__()
        self.enc = torch.nn.Linear(dim, hidden)
        self.l1 = torch.nn.Linear(2 * hidden, hidden)
        self.l2 = torch.nn.Linear(2 * hidden, hidden)
        self.out = torch.nn.Linear(hidden, classes)

    def forward(self, batch):
        local0, local1, local2 = batch.local  # [B], [B, f1], [B * f1, f2]: positions in batch.nodes
        b, f1 = local1.shape
        z = torch.relu(self.enc(batch.x_nodes))                                    # [M, H], M distinct nodes
        n1 = segment_aggregate(z, local2, num_segments=b * f1, op="mean")          # [B * f1, H], no [B f1 f2, H] gather
        h1 = torch.relu(self.l1(torch.cat([gather_rows(z, local1.reshape(-1)), n1], dim=1)))
        h0 = torch.relu(self.l2(torch.cat([gather_rows(z, local0), h1.view(b, f1, -1).mean(1)], dim=1)))
        return self.out(h0)


def main(epochs=2, vertices=20000, quiet=False):
    # the dense layers' own backward must not use atomics either (split-K GEMMs), or the loss would not reproduce
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        return _train(epochs, vertices, quiet)
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])


def _train(epochs, vertices, quiet):
    d = tempfile.mkdtemp(prefix="glx_sage_dedup_")
    npath, epath = write_sources(d, vertices)
    gl.set_padding_mode(gl.CIRCULAR)
    gl.set_sampling_seed(7)
    torch.manual_seed(0)
    g = gl.Graph() \
        .node(npath, "n", gl.Decoder(labeled=True, attr_types=["float"] * DIM)) \
        .edge(epath, ("n", "n", "e"), gl.Decoder()) \
        .init()
    loader = gl.NeighborLoader(g, "n", ["e", "e"], list(FANOUT), batch_size=BATCH, strategy="random", shuffle=True,
                               dedup=True, node_columns=("labels",))
    model = DedupSage(DIM, 64, CLASSES).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    history = []
    for epoch in range(epochs):
        t0, seen, correct, losses, nodes = time.time(), 0, 0, [], 0
        for batch in loader:  # one epoch: every vertex once, in random order
            logits = model(batch)
            labels = batch.y.long()
            loss = torch.nn.functional.cross_entropy(logits, labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
            seen += labels.shape[0]
            correct += int((logits.argmax(1) == labels).sum())
            losses.append(float(loss.detach()))
            nodes += int(batch.nodes.shape[0])
        half = len(losses) // 2
        history.append((losses, correct / seen))
        if not quiet:
            print("epoch %d: loss %.4f -> %.4f (first / second half of the epoch), accuracy %.3f, %d vertices in %.2f s, "
                  "%d distinct nodes for %d slots per batch, bits %s"
                  % (epoch, np.mean(losses[:half]), np.mean(losses[half:]), correct / seen, seen, time.time() - t0,
                     nodes // len(losses), BATCH * (1 + FANOUT[0] * (1 + FANOUT[1])),
                     ",".join(float(x).hex() for x in losses)))
    g.close()
    return history


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
