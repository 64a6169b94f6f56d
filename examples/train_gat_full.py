"""A two-head GAT layer on RAGGED full-neighbour hops, over segment_softmax and weighted_segment_aggregate.

    python examples/train_gat_full.py [epochs] [vertices]            (needs one GPU)

train_gat_dedup.py's GAT layer (gat_conv.py:96-112) without a fan-out: every seed attends to ALL of its neighbours, as
a FullSampler hop delivers them -- Graph.sample_full returns (degrees, nbr, eid), segment s being the next degrees[s]
positions of nbr, anything from one neighbour to a hub's two thousand.

  seeds -> hop     deg, nbr, _ = graph.sample_full(seeds, MAX_LIMIT); glx.unique([seeds, nbr]) relabels both into one
                   list of distinct nodes; z = enc(x_nodes) once per distinct node;
                   e = leaky_relu(a_l . z_v + a_r . z_u) per neighbour position (v, u) and head, read per position
                   through gather_rows; alpha = segment_softmax(e, S, counts=deg): the softmax over each seed's own
                   neighbours, whatever their number; h = weighted_segment_aggregate(z, local, alpha, S, counts=deg):
                   the rows of z scaled per head and summed per seed, without the [n, D] gather.

No backward here uses a float atomic, so a (seed, epoch, batch) triple reproduces its loss bit for bit: main() trains
twice from one seed, prints both runs' per-batch losses as bits and exits non-zero if they differ.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

import torch  # noqa: E402
import graphlearn.graph  # noqa: E402,F401  (puts the engine's ctypes harness on sys.path)
import glx  # noqa: E402
from graphlearn.nn.pytorch import gather_rows, segment_softmax, weighted_segment_aggregate  # noqa: E402

CLASSES, DIM = 5, 16
BATCH = 512
HEADS = 2
HUBS, HUB_DEGREE = 8, 2000
MAX_LIMIT = 0  # every neighbour


def make_graph(vertices):
    """(src, dst, features, labels): train_gat_dedup.py's clustered graph with ragged rows -- 1 to 24 neighbours, four
    in five of them of the vertex's own class, and HUBS vertices with HUB_DEGREE"""
    rng = np.random.default_rng(0)
    label = rng.integers(0, CLASSES, vertices)
    centers = rng.standard_normal((CLASSES, DIM)) * 0.35
    feats = (centers[label] + rng.standard_normal((vertices, DIM))).astype(np.float32)
    degree = rng.integers(1, 25, vertices)
    degree[rng.choice(vertices, HUBS, replace=False)] = HUB_DEGREE
    src = np.repeat(np.arange(vertices), degree)
    by_class = np.argsort(label, kind="stable")
    first = np.searchsorted(label[by_class], np.arange(CLASSES))
    size = np.bincount(label, minlength=CLASSES)
    own = by_class[first[label[src]] + (rng.random(len(src)) * size[label[src]]).astype(np.int64)]
    dst = np.where(rng.random(len(src)) < 0.8, own, rng.integers(0, vertices, len(src)))
    return src.astype(np.int64), dst.astype(np.int64), feats, label.astype(np.int64)


class FullGat(torch.nn.Module):
    """z = enc(x) per distinct node; a two-head GAT layer over each seed's whole neighbourhood; a linear classifier."""

    def __init__(self, dim, hidden, classes, heads=HEADS):
        super().__init__()
        assert hidden % heads == 0
        self.heads, self.hidden = heads, hidden
        self.enc = torch.nn.Linear(dim, hidden, bias=False)
        self.a_l = torch.nn.Parameter(torch.randn(heads, hidden // heads) * 0.1)
        self.a_r = torch.nn.Parameter(torch.randn(heads, hidden // heads) * 0.1)
        self.l1 = torch.nn.Linear(2 * hidden, hidden)
        self.out = torch.nn.Linear(hidden, classes)

    def forward(self, x_nodes, local0, local, deg):
        """x_nodes [M, dim]: the distinct nodes' features; local0 [S]: the seeds' positions among them; local [n]: the
        neighbours', segment s being the next deg[s] of them"""
        s, n = local0.numel(), local.numel()
        z = self.enc(x_nodes)                                                       # [M, H * C], M distinct nodes
        zh = z.view(-1, self.heads, self.hidden // self.heads)
        # the two halves of the attention logit, once per distinct node; read per position through gather_rows
        src_e = (zh * self.a_l).sum(-1).contiguous()                                # [M, H]
        dst_e = (zh * self.a_r).sum(-1).contiguous()
        seed_of = torch.repeat_interleave(local0, deg.long(), output_size=n)        # the seed each position belongs to
        e = torch.nn.functional.leaky_relu(gather_rows(src_e, seed_of) + gather_rows(dst_e, local), 0.2)   # [n, H]
        alpha = segment_softmax(e.contiguous(), s, counts=deg)                      # over each seed's own neighbours
        h = weighted_segment_aggregate(z, local, alpha, s, counts=deg)              # [S, hidden]
        h0 = torch.relu(self.l1(torch.cat([gather_rows(z, local0), h], dim=1)))
        return self.out(h0)


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
    torch.manual_seed(0)
    order = torch.Generator()
    order.manual_seed(7)
    g = glx.Graph.from_edges(src, dst, sort_by_weight=False)
    model = FullGat(DIM, 64, CLASSES).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    history = []
    for epoch in range(epochs):
        t0, seen, correct, losses, longest = time.time(), 0, 0, [], 0
        perm = torch.randperm(vertices, generator=order).cuda()  # one epoch: every vertex once, in random order
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
                  "%.2f s, longest neighbourhood %d, bits %s"
                  % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), correct / seen, seen, time.time() - t0,
                     longest, ",".join(float(x).hex() for x in losses)))
    g.close()
    return history


if __name__ == "__main__":
    _, same = main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
    sys.exit(0 if same else 1)
