"""TGN for link prediction on a stream of timestamped interactions: the reference's own PyTorch model
(graphlearn/examples/pytorch/tgn/train_and_eval.py) on this engine, memory module included.

    python examples/train_tgn.py [epochs] [events]            (needs one GPU)

The three parts of the reference's model:
  memory     graphlearn.nn.pytorch.TGNMemory -- torch_geometric's TGNMemory with IdentityMessage and LastAggregator
             (train_and_eval.py:70-78) with its message store in HBM: one pending slot per node, written by
             glx_tgn_store_update, read by glx_tgn_message; no Python dict, no n_id.tolist(), no host sync
  embedding  the reference's GraphAttentionEmbedding (train_and_eval.py:38-50): rel_t = last_update[nbr] - ts, edge
             input [time_enc(rel_t), edge_x], on TransformerConv(memory_dim, embedding_dim // 2, heads=2, dropout=0.1);
             it shares the memory's time encoder
  predictor  the reference's LinkPredictor (train_and_eval.py:53-63)
Batches come from gl.TemporalNeighborLoader in time order -- for every end point of every event the 10 most recent
interactions STRICTLY BEFORE the event (the reference's loader samples time-blind) --, one random negative per event,
relabelled with glx.unique; an event's raw message is the float attributes of its edge.  As in the reference a batch's
events enter the memory (update_state) before its backward.  The first 80 % of the stream train the model, the rest
is scored in eval mode while the memory keeps moving, as the reference's validation split.

main() exits non-zero unless every sampled edge's timestamp is below its event's, and unless two runs from one seed print
the same per-batch losses bit for bit (the store keeps the LATEST event per node with ties decided by position, no
kernel on the path uses a float atomic, the dropout masks come from the engine's contract generator).
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
from graphlearn.nn.pytorch import TGNMemory, TransformerConv  # noqa: E402
from train_tgat import EDGE_DIM, ITEMS, USERS, leaks, write_source  # noqa: E402  (the synthetic timestamped source)

MEMORY_DIM = TIME_DIM = EMBEDDING_DIM = 100  # the reference's defaults (train_and_eval.py:233-235)
BATCH, FANOUT, NEGATIVES, DROPOUT, TRAIN_SHARE = 200, 10, 1, 0.1, 0.8
ROLES = ("src", "dst", "neg")


class GraphAttentionEmbedding(torch.nn.Module):

    def __init__(self, in_channels, out_channels, msg_dim, time_enc):
        super().__init__()
        self.time_enc = time_enc
        self.conv = TransformerConv(in_channels, out_channels // 2, heads=2, dropout=DROPOUT,
                                    edge_dim=msg_dim + time_enc.out_channels)

    def forward(self, x, last_update, seed_local, nbr_local, counts, t, msg):
        rel_t = last_update[nbr_local] - t
        edge_attr = torch.cat([self.time_enc(rel_t.to(x.dtype)), msg], dim=-1)
        return self.conv(x, seed_local, nbr_local, counts, edge_attr)


class LinkPredictor(torch.nn.Module):

    def __init__(self, in_channels):
        super().__init__()
        self.lin_src = torch.nn.Linear(in_channels, in_channels)
        self.lin_dst = torch.nn.Linear(in_channels, in_channels)
        self.lin_final = torch.nn.Linear(in_channels, 1)

    def forward(self, z_src, z_dst):
        return self.lin_final((self.lin_src(z_src) + self.lin_dst(z_dst)).relu())


def embed(memory, gnn, batch):
    """the three roles' embeddings of one batch: [B, EMBEDDING_DIM] each"""
    import glx
    ragged = {role: batch.ragged(role, 0, with_positions=True) for role in ROLES}
    parts = [batch.seeds(role) for role in ROLES] + [ragged[role][0] for role in ROLES]
    n_id, local, _ = glx.unique(parts)  # the batch's distinct nodes and every part's rows among them
    z, last_update = memory(n_id)
    out = []
    for r, role in enumerate(ROLES):
        _, _, ts, counts, at = ragged[role]
        msg = batch.block(role, 0).edge_x.reshape(-1, EDGE_DIM)[at]
        out.append(gnn(z, last_update, local[r], local[3 + r], counts, ts, msg))
    return out


def main(epochs=1, events=20000, quiet=False):
    """two runs from one seed -> ([run][epoch] = (training losses, accuracy on the held-out end of the stream), leaked
    edges, whether the losses are the same bits)"""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        path = write_source(tempfile.mkdtemp(prefix="glx_tgn_"), events)
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
    raw_of = g.device_edge_features("interaction")
    memory = TGNMemory(USERS + ITEMS, EDGE_DIM, MEMORY_DIM, TIME_DIM).cuda()
    gnn = GraphAttentionEmbedding(MEMORY_DIM, EMBEDDING_DIM, EDGE_DIM, memory.time_enc).cuda()
    link_pred = LinkPredictor(EMBEDDING_DIM).cuda()
    modules = (memory, gnn, link_pred)
    params = {id(p): p for m in modules for p in m.parameters()}  # the time encoder is shared: once
    opt = torch.optim.Adam(list(params.values()), lr=1e-3)
    criterion = torch.nn.BCEWithLogitsLoss()
    split = max(int(len(loader) * TRAIN_SHARE), 1)
    history, leaked = [], 0
    for epoch in range(epochs):
        t0, losses, seen, correct = time.time(), [], 0, 0
        memory.reset_state()  # start with a fresh memory
        for i, batch in enumerate(loader):  # the events in time order
            training = i < split
            for m in modules:
                m.train(training)
            leaked += leaks(batch)
            with torch.set_grad_enabled(training):
                z_src, z_dst, z_neg = embed(memory, gnn, batch)
                pos_out, neg_out = link_pred(z_src, z_dst), link_pred(z_src, z_neg)
                loss = criterion(pos_out, torch.ones_like(pos_out)) + criterion(neg_out, torch.zeros_like(neg_out))
            # update the memory with the ground-truth events -- before the backward, as the reference does
            memory.update_state(batch.src, batch.dst, batch.t, raw_of.lookup(batch.eid, 0.0))
            if training:
                opt.zero_grad()
                loss.backward()
                opt.step()
                memory.detach()
                losses.append(float(loss.detach()))
            else:
                seen += pos_out.numel() + neg_out.numel()
                correct += int((pos_out > 0).sum()) + int((neg_out <= 0).sum())
        accuracy = correct / max(seen, 1)
        history.append((losses, accuracy))
        if not quiet:
            half = len(losses) // 2
            print("run %d epoch %d: loss %.4f -> %.4f (first / second half of the training stream), held-out accuracy "
                  "%.3f, %d events in %.2f s, bits %s" % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), accuracy,
                                                          len(loader) * BATCH, time.time() - t0,
                                                          ",".join(float(x).hex() for x in losses)))
    g.close()
    return history, leaked


if __name__ == "__main__":
    _, leaked, same = main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
    sys.exit(0 if same and leaked == 0 else 1)
