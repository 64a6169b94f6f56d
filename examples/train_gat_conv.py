"""A two-head GATConv layer with attention dropout on RAGGED full-neighbour hops.

    python examples/train_gat_conv.py [epochs] [vertices]            (needs one GPU)

train_gat_full.py's model and graph with its hand-written attention step replaced by the layer
graphlearn.nn.pytorch.GATConv (the reference's gat_conv.py:29-119): the linear map, the two halves of the logit per
distinct node, then ONE fused kernel per direction for leaky_relu, the softmax over each seed's own neighbours and
dropout 0.4 on the coefficients (gat_attention), and the weighted reduce.  Every seed also attends to itself.

The dropout mask is a function of (seed, step, position, head) -- the engine's contract generator, not the device's
-- and no backward uses a float atomic, so a (seed, epoch, batch) triple reproduces its loss bit for bit: main()
trains twice from one seed, prints both runs' per-batch losses as bits and exits non-zero if they differ.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import graphlearn.graph  # noqa: E402,F401  (puts the engine's ctypes harness on sys.path)
import glx  # noqa: E402
from graphlearn.nn.pytorch import GATConv, gather_rows  # noqa: E402
from train_gat_full import BATCH, CLASSES, DIM, HEADS, MAX_LIMIT, make_graph  # noqa: E402

DROPOUT = 0.4


class ConvGat(torch.nn.Module):
    """z = relu(enc(x)) per distinct node; a two-head GATConv over each seed's whole neighbourhood and itself; a linear
    classifier on the seed's own row next to the layer's output"""

    def __init__(self, dim, hidden, classes, heads=HEADS):
        super().__init__()
        assert hidden % heads == 0
        self.enc = torch.nn.Linear(dim, hidden)
        self.conv = GATConv(hidden, hidden // heads, num_heads=heads, concat=True, dropout=DROPOUT, use_bias=True)
        self.out = torch.nn.Linear(2 * hidden, classes)

    def forward(self, x_nodes, local0, local, deg):
        z = torch.relu(self.enc(x_nodes))                                           # [M, hidden], M distinct nodes
        h = torch.relu(self.conv(z, local0, local, deg))                            # [S, hidden]
        return self.out(torch.cat([gather_rows(z, local0), h], dim=1))


def main(epochs=1, vertices=20000, quiet=False):
    """two runs from one seed -> ([run][epoch] = (losses, accuracy), whether the two runs' losses are the same bits)"""
    # the dense layers' own backward must not use atomics either (split-K GEMMs), or the loss would not reproduce
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        data = make_graph(vertices)
        runs = [_train(data, epochs, quiet, run) for run in range(2)]
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    same = all(float(a).hex() == float(b).hex() for (la, _), (lb, _) in zip(*runs) for a, b in zip(la, lb))
    if not quiet:
        print("the two runs' losses are %s" % ("the same bits" if same else "NOT the same bits"))
    return runs, same


def _train(data, epochs, quiet, run):
    src, dst, feats, label = (torch.from_numpy(a).cuda() for a in data)
    vertices = int(feats.shape[0])
    torch.manual_seed(0)  # the parameters' initial values AND the seed of the dropout masks
    order = torch.Generator()
    order.manual_seed(7)
    g = glx.Graph.from_edges(src, dst, sort_by_weight=False)
    model = ConvGat(DIM, 64, CLASSES).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    history = []
    for epoch in range(epochs):
        t0, seen, correct, losses, longest = time.time(), 0, 0, [], 0
        perm = torch.randperm(vertices, generator=order).cuda()  # one epoch: every vertex once, in random order
        model.train()
        for at in range(0, vertices, BATCH):
            seeds = perm[at:at + BATCH].contiguous()
            deg, nbr, _ = g.sample_full(seeds, MAX_LIMIT)
            nodes, (local0, local), _ = glx.unique([seeds, nbr])
            logits = model(feats[nodes], local0, local, deg)
            labels = label[seeds]
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
