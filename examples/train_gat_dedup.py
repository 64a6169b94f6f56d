"""A two-head GAT layer and a GCN-style layer on compact batches, over weighted_segment_aggregate.

    python examples/train_gat_dedup.py [epochs] [vertices]            (needs one GPU)

train_sage_dedup.py's classifier with its two mean aggregations replaced by the reference's other two layer families:

  hop 2 -> hop 1   GAT (gat_conv.py:96-110), two heads.  z = enc(x_nodes) once per distinct node;
                   e = leaky_relu(a_l . z_v + a_r . z_u) per sampled edge (v, u) and head, read per slot through
                   gather_rows; alpha = softmax(e) over the fan-out -- a dense sampler response, so plain torch.softmax
                   over [S, k, H]; then weighted_segment_aggregate(z, local2, alpha): the rows of z scaled per head and
                   summed per hop-1 slot, without the [n, D] gather.  alpha is learned: its gradient is the second
                   output of the operator's backward.
  hop 1 -> seeds   GCN-style (gcn_conv.py:52-73): the loader's edge_columns=("weights",) delivers the sampled edges'
                   weights from HBM, one per slot; each row of h1 is scaled by its edge's weight, normalised over the
                   fan-out, and summed per seed.

Neither backward uses a float atomic, so a (seed, epoch, batch) triple reproduces its loss bit for bit: main() trains
twice from one seed and prints both runs' per-batch losses as bits.
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
from graphlearn.nn.pytorch import gather_rows, weighted_segment_aggregate  # noqa: E402

CLASSES, DIM, DEG = 5, 16, 12
FANOUT = (10, 5)
BATCH = 512
HEADS = 2


def write_sources(directory, vertices):
    """train_sage_dedup.py's graph with edge weights: an edge inside a class weighs about twice one across classes"""
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
        f.write("src_id:int64\tdst_id:int64\tweight:float\n")
        for v in range(vertices):
            same = rng.random(DEG) < 0.8
            dst = np.where(same, rng.choice(by_class[label[v]], DEG), rng.integers(0, vertices, DEG))
            w = np.where(label[dst] == label[v], 1.0, 0.5) + 0.2 * rng.random(DEG)
            f.writelines("%d\t%d\t%.4f\n" % (v, d, x) for d, x in zip(dst, w))
    return npath, epath


class DedupGat(torch.nn.Module):
    """z = enc(x) per distinct node; a two-head GAT layer from hop 2 to hop 1; a GCN-style layer weighted by the
    sampled edges' own weights from hop 1 to the seeds; a linear classifier."""

    def __init__(self, dim, hidden, classes, heads=HEADS):
        super().__init__()
        assert hidden % heads == 0
        self.heads, self.hidden = heads, hidden
        self.enc = torch.nn.Linear(dim, hidden, bias=False)
        self.a_l = torch.nn.Parameter(torch.randn(heads, hidden // heads) * 0.1)
        self.a_r = torch.nn.Parameter(torch.randn(heads, hidden // heads) * 0.1)
        self.l1 = torch.nn.Linear(2 * hidden, hidden)
        self.l2 = torch.nn.Linear(2 * hidden, hidden)
        self.out = torch.nn.Linear(hidden, classes)

    def forward(self, batch):
        local0, local1, local2 = batch.local  # [B], [B, f1], [B * f1, f2]: positions in batch.nodes
        b, f1 = local1.shape
        s, k = local2.shape
        z = self.enc(batch.x_nodes)                                                 # [M, H * C], M distinct nodes
        zh = z.view(-1, self.heads, self.hidden // self.heads)
        # the two halves of the attention logit, once per distinct node; read per slot through gather_rows
        e_l = (zh * self.a_l).sum(-1).contiguous()                                  # [M, H]
        e_r = (zh * self.a_r).sum(-1).contiguous()
        e = gather_rows(e_l, local1.reshape(-1)).unsqueeze(1) + gather_rows(e_r, local2)   # [S, k, H]
        alpha = torch.softmax(torch.nn.functional.leaky_relu(e, 0.2), dim=1)        # over the fan-out
        n1 = weighted_segment_aggregate(z, local2, alpha.reshape(s * k, self.heads), num_segments=s, op="sum")
        h1 = torch.relu(self.l1(torch.cat([gather_rows(z, local1.reshape(-1)), n1], dim=1)))   # [B * f1, hidden]
        # GCN-style: hop 1's rows scaled by their edges' weights, normalised over the seed's fan-out
        w = batch.edge_cols[0]["weights"]                                           # [B, f1], from HBM
        w = (w / w.sum(1, keepdim=True).clamp_min(1e-12)).reshape(-1).contiguous()
        slots = torch.arange(b * f1, device=h1.device)
        n0 = weighted_segment_aggregate(h1.contiguous(), slots, w, num_segments=b, op="sum")
        h0 = torch.relu(self.l2(torch.cat([gather_rows(z, local0), n0], dim=1)))
        return self.out(h0)


def main(epochs=1, vertices=20000, quiet=False):
    """two runs from one seed -> [run][epoch] = (losses, accuracy); the losses of the two runs are the same bits"""
    # the dense layers' own backward must not use atomics either (split-K GEMMs), or the loss would not reproduce
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        d = tempfile.mkdtemp(prefix="glx_gat_dedup_")
        paths = write_sources(d, vertices)
        runs = [_train(paths, epochs, quiet, run) for run in range(2)]
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    same = all(float(a).hex() == float(b).hex() for (la, _), (lb, _) in zip(*runs) for a, b in zip(la, lb))
    if not quiet:
        print("the two runs' losses are %s" % ("the same bits" if same else "NOT the same bits"))
    return runs


def _train(paths, epochs, quiet, run):
    npath, epath = paths
    gl.set_padding_mode(gl.CIRCULAR)
    gl.set_sampling_seed(7)
    torch.manual_seed(0)
    g = gl.Graph() \
        .node(npath, "n", gl.Decoder(labeled=True, attr_types=["float"] * DIM)) \
        .edge(epath, ("n", "n", "e"), gl.Decoder(weighted=True)) \
        .init()
    loader = gl.NeighborLoader(g, "n", ["e", "e"], list(FANOUT), batch_size=BATCH, strategy="edge_weight", shuffle=True,
                               dedup=True, node_columns=("labels",), edge_columns=("weights",))
    model = DedupGat(DIM, 64, CLASSES).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    history = []
    for epoch in range(epochs):
        t0, seen, correct, losses = time.time(), 0, 0, []
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
        half = len(losses) // 2
        history.append((losses, correct / seen))
        if not quiet:
            print("run %d epoch %d: loss %.4f -> %.4f (first / second half of the epoch), accuracy %.3f, %d vertices in "
                  "%.2f s, bits %s" % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), correct / seen, seen,
                                       time.time() - t0, ",".join(float(x).hex() for x in losses)))
    g.close()
    return history


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
