"""Unsupervised GraphSAGE with sampled negatives, scored with pair_dot.

    python examples/train_sage_unsup.py [epochs] [vertices]            (needs one GPU)

The link-prediction half of the reference's examples (examples/tf/sage/train.py:56-57 with python/nn/tf/loss.py:28-42)
on train_gat_dedup.py's clustered synthetic graph, everything on the device:

  edges      B source vertices of a shuffled pass over the type, one sampled out-edge each: (src, dst)
  negatives  glx.Negative.from_graph(g, by_in_degree=True).sample(src, K): K popularity-weighted candidates per source
  node set   glx.unique([src, dst, neg]): every distinct endpoint once, and each slot's position in that set
  encoder    one sampled hop over the distinct endpoints, reduced with segment_aggregate (mean): z once per node
  scores     pos = pair_dot(z, l_src, z, l_dst)  [B];  negs = pair_dot(z, l_src, z, l_neg.view(B, K))  [B, K] -- no
             [B * K, D] gather going forward, no index_add_ with float atomics going back
  loss       the reference's sigmoid_cross_entropy_loss: mean(xent(pos, 1)) + mean(xent(negs, 0))

No backward uses a float atomic, so a (seed, epoch, batch) triple reproduces its loss bit for bit: main() trains twice
from one seed, prints both runs' per-batch losses as bits and exits non-zero if they differ.
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import graphlearn as gl  # noqa: E402
from graphlearn.nn.pytorch import pair_dot, segment_aggregate  # noqa: E402
from train_gat_dedup import DIM, write_sources  # noqa: E402

BATCH = 256    # edges per batch
NEGATIVES = 5  # K
FANOUT = 10
HIDDEN = 64
SEED = 7


def _glx():
    import glx  # graphlearn put the engine's harness on sys.path
    return glx


class UnsupSage(torch.nn.Module):
    """h = relu(enc(x)) per node of the hop; z = l1([h_v, mean of h over v's sampled neighbours]) per distinct endpoint"""

    def __init__(self, dim, hidden):
        super().__init__()
        self.enc = torch.nn.Linear(dim, hidden)
        self.l1 = torch.nn.Linear(2 * hidden, hidden)

    def forward(self, x_all, l_nbr, m):
        # x_all: features of the endpoints (the first m rows) and of their sampled neighbours; l_nbr [m, f]: rows of it
        h = torch.relu(self.enc(x_all))
        nbr = segment_aggregate(h, l_nbr, num_segments=m, op="mean")
        return self.l1(torch.cat([h[:m], nbr], dim=1)).contiguous()


def sigmoid_cross_entropy_loss(pos_logit, neg_logit):
    """loss.py:28-42: labels 1 for the edges, 0 for the negatives; the mean of each, added"""
    xent = torch.nn.functional.binary_cross_entropy_with_logits
    return xent(pos_logit, torch.ones_like(pos_logit)) + xent(neg_logit, torch.zeros_like(neg_logit))


def main(epochs=1, vertices=20000, quiet=False):
    """two runs from one seed -> ([run][epoch] = losses, whether the two runs' losses are the same bits)"""
    # the dense layers' own backward must not use atomics either (split-K GEMMs), or the loss would not reproduce
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        d = tempfile.mkdtemp(prefix="glx_sage_unsup_")
        paths = write_sources(d, vertices)
        runs = [_train(paths, vertices, epochs, quiet, run) for run in range(2)]
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    same = all(float(a).hex() == float(b).hex() for la, lb in zip(*runs) for a, b in zip(la, lb))
    if not quiet:
        print("the two runs' losses are %s" % ("the same bits" if same else "NOT the same bits"))
    return runs, same


def _train(paths, vertices, epochs, quiet, run):
    glx = _glx()
    npath, epath = paths
    gl.set_padding_mode(gl.CIRCULAR)
    torch.manual_seed(0)
    g = gl.Graph() \
        .node(npath, "n", gl.Decoder(labeled=True, attr_types=["float"] * DIM)) \
        .edge(epath, ("n", "n", "e"), gl.Decoder(weighted=True)) \
        .init()
    graph, feats = g.device_graph("e"), g.device_features("n")
    negative = glx.Negative.from_graph(graph, by_in_degree=True)
    model = UnsupSage(DIM, HIDDEN).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    order = torch.Generator().manual_seed(SEED)
    history, calls = [], 0
    for epoch in range(epochs):
        t0, losses = time.time(), []
        perm = torch.randperm(vertices, generator=order).cuda()
        for at in range(0, vertices - BATCH + 1, BATCH):  # one epoch: every vertex once as a source, in random order
            src = perm[at:at + BATCH].contiguous()
            dst = graph.sample("RandomSampler", src, 1, seed=SEED, call_counter=calls)[0].reshape(-1)
            neg = negative.sample(src, NEGATIVES, seed=SEED, call_counter=calls + 1)          # [B, K]
            nodes, (l_src, l_dst, l_neg), _ = glx.unique([src, dst, neg.reshape(-1)])
            m = int(nodes.shape[0])
            nbr = graph.sample("RandomSampler", nodes, FANOUT, seed=SEED, call_counter=calls + 2)[0]   # [m, f]
            calls += 3
            # the hop's own distinct set: the endpoints come first in it (first occurrence), in their own order
            every, (_, l_nbr), _ = glx.unique([nodes, nbr])
            z = model(feats.lookup(every), l_nbr, m)                                          # [m, HIDDEN]
            pos = pair_dot(z, l_src, z, l_dst)                                                # [B]
            negs = pair_dot(z, l_src, z, l_neg.view(BATCH, NEGATIVES))                        # [B, K]
            loss = sigmoid_cross_entropy_loss(pos, negs)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        half = len(losses) // 2
        history.append(losses)
        if not quiet:
            print("run %d epoch %d: loss %.4f -> %.4f (first / second half of the epoch), %d edges in %.2f s, bits %s"
                  % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), len(losses) * BATCH,
                     time.time() - t0, ",".join(float(x).hex() for x in losses)))
    negative.close()
    g.close()
    return history


if __name__ == "__main__":
    _, same_bits = main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
    sys.exit(0 if same_bits else 1)
