"""A memory-less temporal attention model (TGAT-style) for link prediction on a stream of timestamped interactions.

    python examples/train_tgat.py [epochs] [events]            (needs one GPU)

The workload the reference's TGN example reaches for (graphlearn/examples/pytorch/tgn/train_and_eval.py with
temporal_batch_loader.py:70-80) without its leak: that loader takes a time-blind topk sample of the whole interaction
graph, so an event is predicted from edges of its own future.  gl.TemporalNeighborLoader walks the events in time order
and samples, for every end point of every event, the neighbours over edges STRICTLY BEFORE the event's time
(glx_sample_temporal_hops: one cutoff per request row); batches never leave the GPU.

The model: a trainable embedding per node; one two-head TransformerConv over ragged("src" | "dst" | "neg", 0) -- the
valid slots of the 10 most recent interactions -- whose edge input is the interaction's float attributes next to a
cos(w * rel_t + b) encoding of how long before the event it happened; pair_dot scores of (src, dst) against
(src, neg_dst), binary cross-entropy.  TGN's memory module and message store are not part of it.

main() exits non-zero unless every sampled edge's timestamp is below its event's, and unless two runs from one seed print
the same per-batch losses bit for bit (no kernel on the path uses a float atomic; the dropout masks come from the
engine's contract generator).
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
from graphlearn.nn.pytorch import TransformerConv, pair_dot  # noqa: E402

USERS, ITEMS, GROUPS = 600, 400, 8
DIM, HIDDEN, HEADS, EDGE_DIM, TIME_DIM = 32, 32, 2, 4, 8
BATCH, FANOUT, NEGATIVES, DROPOUT = 200, 10, 1, 0.1


def write_source(directory, events):
    """users 0 .. USERS - 1 and items USERS .. USERS + ITEMS - 1 in GROUPS groups; a user interacts mostly with items of
    its group, and an interaction's attributes say (noisily) whether it stayed inside the group.  Timestamps ascend
    with ties; the file lists the interactions in no particular order."""
    rng = np.random.default_rng(0)
    user_group = rng.integers(0, GROUPS, USERS)
    item_group = rng.integers(0, GROUPS, ITEMS)
    by_group = [np.flatnonzero(item_group == c) for c in range(GROUPS)]
    src = rng.integers(0, USERS, events)
    inside = rng.random(events) < 0.8
    dst = np.array([rng.choice(by_group[user_group[u]]) if s and len(by_group[user_group[u]]) else rng.integers(0, ITEMS)
                    for u, s in zip(src, inside)])
    t = np.sort(rng.integers(0, max(events // 2, 1), events))
    attr = np.where(item_group[dst] == user_group[src], 1.0, -1.0)[:, None] + rng.standard_normal((events, EDGE_DIM))
    path = os.path.join(directory, "interaction")
    with open(path, "w") as f:
        f.write("src_id:int64\tdst_id:int64\ttimestamp:int64\tfeature:string\n")
        for i in rng.permutation(events):
            f.write("%d\t%d\t%d\t%s\n" % (src[i], USERS + dst[i], t[i], ":".join("%.4f" % x for x in attr[i])))
    return path


class TemporalAttention(torch.nn.Module):
    """h(v, t) = TransformerConv(embedding, v, the neighbours of v before t, [edge attributes, cos(w dt + b)])"""

    def __init__(self, nodes):
        super().__init__()
        self.emb = torch.nn.Parameter(torch.randn(nodes, DIM) * DIM ** -0.5)
        self.time_w = torch.nn.Parameter(10.0 ** -torch.linspace(0, 3, TIME_DIM))
        self.time_b = torch.nn.Parameter(torch.zeros(TIME_DIM))
        self.conv = TransformerConv(DIM, HIDDEN // HEADS, heads=HEADS, dropout=DROPOUT, edge_dim=EDGE_DIM + TIME_DIM)

    def forward(self, batch, role):
        blk = batch.block(role, 0)
        rows, _, _, counts, at = batch.ragged(role, 0, with_positions=True)
        rel_t = blk.rel_t.reshape(-1)[at].to(torch.float32)
        edge = torch.cat([blk.edge_x.reshape(-1, EDGE_DIM)[at], torch.cos(rel_t[:, None] * self.time_w + self.time_b)], 1)
        return self.conv(self.emb, batch.seeds(role), rows, counts, edge)


def leaks(batch):
    """sampled edges that did NOT happen before their event"""
    n = 0
    for role in ("src", "dst", "neg"):
        blk = batch.block(role, 0)
        n += int((blk.valid & (blk.ts >= blk.cutoff[:, None])).sum())
    return n


def main(epochs=1, events=20000, quiet=False):
    """two runs from one seed -> ([run][epoch] = (losses, accuracy), leaked edges, whether the losses are the same bits)"""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        path = write_source(tempfile.mkdtemp(prefix="glx_tgat_"), events)
        runs = [_train(path, epochs, quiet, run) for run in range(2)]
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    leaked = sum(r[1] for r in runs)
    same = all(float(a).hex() == float(b).hex() for (la, _), (lb, _) in zip(runs[0][0], runs[1][0]) for a, b in zip(la, lb))
    if not quiet:
        print("%d sampled edges at or after their event's time" % leaked)
        print("the two runs' losses are %s" % ("the same bits" if same else "NOT the same bits"))
    return [r[0] for r in runs], leaked, same


def _train(path, epochs, quiet, run):
    gl.set_default_neighbor_id(0)
    gl.set_sampling_seed(7)
    torch.manual_seed(0)  # the parameters' initial values AND the seed of the dropout masks
    g = gl.Graph() \
        .edge(path, ("user", "item", "interaction"), gl.Decoder(timestamped=True, attr_types=["float"] * EDGE_DIM),
              directed=False) \
        .init()
    loader = gl.TemporalNeighborLoader(g, "interaction", "interaction", [FANOUT], BATCH, strategy="recent",
                                       negatives=NEGATIVES, edge_features=True)
    model = TemporalAttention(USERS + ITEMS).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    history, leaked = [], 0
    for epoch in range(epochs):
        t0, seen, correct, losses = time.time(), 0, 0, []
        model.train()
        for batch in loader:  # the events in time order
            leaked += leaks(batch)
            h_src, h_dst, h_neg = model(batch, "src"), model(batch, "dst"), model(batch, "neg")
            each = torch.arange(batch.src.shape[0], device=h_src.device)
            pos = pair_dot(h_src, each, h_dst, each)
            neg = pair_dot(h_src, each, h_neg, torch.arange(h_neg.shape[0], device=h_src.device).reshape(-1, NEGATIVES))
            logits = torch.cat([pos, neg.reshape(-1)])
            target = torch.cat([torch.ones_like(pos), torch.zeros(neg.numel(), device=pos.device)])
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, target)
            opt.zero_grad()
            loss.backward()
            opt.step()
            seen += logits.shape[0]
            correct += int(((logits > 0) == (target > 0)).sum())
            losses.append(float(loss.detach()))
        half = len(losses) // 2
        history.append((losses, correct / seen))
        if not quiet:
            print("run %d epoch %d: loss %.4f -> %.4f (first / second half of the stream), accuracy %.3f, %d events in "
                  "%.2f s, bits %s" % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), correct / seen,
                                       len(losses) * BATCH, time.time() - t0, ",".join(float(x).hex() for x in losses)))
    g.close()
    return history, leaked


if __name__ == "__main__":
    _, leaked, same = main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
    sys.exit(0 if same and leaked == 0 else 1)
