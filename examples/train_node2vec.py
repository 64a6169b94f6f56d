"""node2vec with trainable id embeddings: two SparseEmbedding tables and SparseAdam.

    python examples/train_node2vec.py [epochs] [vertices]            (needs one GPU)

The reference's examples/tf/node2vec (node2vec.py:49-50: a target and a context EmbeddingColumn over all node ids; the
window pairs of :53-66; the loss of :100-111) on train_gat_dedup.py's clustered synthetic graph, everything on the device:

  walks      B start vertices of a shuffled pass over the type, 9 biased steps each (p = q = 0.25): [B, 10] with the start
  negatives  glx.Negative.from_graph(g, by_in_degree=True).sample(walk positions, K): K candidates per walk position
  node set   glx.unique([walks, negs]): every distinct id once, and each slot's position in that set
  tables     zt = target(nodes, distinct=True), zc = context(nodes, distinct=True): one row per distinct id -- the only
             rows the step reads or writes; no gradient of the tables' size exists at any point
  scores     pos = pair_dot(zt, l_src, zc, l_dst) over the window pairs (two to the left, two to the right);
             neg = pair_dot(zt, l_walk, zc, l_neg.view(-1, K))
  loss       mean(xent(pos, 1)) + mean(xent(neg, 0))
  step       SparseAdam on both tables: the noted row gradients applied in place by one kernel per table

No float atomic anywhere, so a (seed, epoch, batch) triple reproduces its loss bit for bit: main() trains twice from one
seed, prints both runs' per-batch losses as bits and exits non-zero if they differ.
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
from graphlearn.nn.pytorch import SparseAdam, SparseEmbedding, pair_dot  # noqa: E402
from train_gat_dedup import DIM, write_sources  # noqa: E402

BATCH = 256      # walks per batch
STEPS = 9        # steps per walk: WALK_LEN positions with the start
WALK_LEN = STEPS + 1
LEFT = RIGHT = 2  # window
NEGATIVES = 5    # K
EMB_DIM = 128
P = Q = 0.25
SEED = 7


def _glx():
    import glx  # graphlearn put the engine's harness on sys.path
    return glx


def window_pairs(walk_len, left, right):
    """(src, dst) positions inside one walk: every position with its `left` predecessors and its `right` successors"""
    src, dst = [], []
    for i in range(walk_len):
        for j in list(range(max(i - left, 0), i)) + list(range(i + 1, min(i + right + 1, walk_len))):
            src.append(i)
            dst.append(j)
    return src, dst


def sigmoid_cross_entropy_loss(pos_logit, neg_logit):
    xent = torch.nn.functional.binary_cross_entropy_with_logits
    return xent(pos_logit, torch.ones_like(pos_logit)) + xent(neg_logit, torch.zeros_like(neg_logit))


def main(epochs=1, vertices=20000, quiet=False):
    """two runs from one seed -> ([run][epoch] = losses, whether the two runs' losses are the same bits)"""
    d = tempfile.mkdtemp(prefix="glx_node2vec_")
    paths = write_sources(d, vertices)
    runs = [_train(paths, vertices, epochs, quiet, run) for run in range(2)]
    same = all(float(a).hex() == float(b).hex() for la, lb in zip(*runs) for a, b in zip(la, lb))
    if not quiet:
        print("the two runs' losses are %s" % ("the same bits" if same else "NOT the same bits"))
    return runs, same


def _train(paths, vertices, epochs, quiet, run):
    glx = _glx()
    npath, epath = paths
    gl.set_padding_mode(gl.CIRCULAR)
    g = gl.Graph() \
        .node(npath, "n", gl.Decoder(labeled=True, attr_types=["float"] * DIM)) \
        .edge(epath, ("n", "n", "e"), gl.Decoder(weighted=True)) \
        .init()
    graph = g.device_graph("e")
    negative = glx.Negative.from_graph(graph, by_in_degree=True)
    target = SparseEmbedding(vertices, EMB_DIM, seed=SEED)
    context = SparseEmbedding(vertices, EMB_DIM, seed=SEED + 1)
    opt = SparseAdam([target, context], lr=0.01)
    w_src, w_dst = (torch.tensor(x, device="cuda") for x in window_pairs(WALK_LEN, LEFT, RIGHT))
    order = torch.Generator().manual_seed(SEED)
    history, calls = [], 0
    for epoch in range(epochs):
        t0, losses = time.time(), []
        perm = torch.randperm(vertices, generator=order).cuda()
        for at in range(0, vertices - BATCH + 1, BATCH):  # one epoch: every vertex once as a start, in random order
            src = perm[at:at + BATCH].contiguous()
            steps = graph.random_walk(src, STEPS, p=P, q=Q, seed=SEED, call_counter=calls)          # [B, 9]
            walks = torch.cat([src[:, None], steps], dim=1).contiguous()                             # [B, 10]
            negs = negative.sample(walks.reshape(-1), NEGATIVES, seed=SEED, call_counter=calls + STEPS)  # [B * 10, K]
            calls += STEPS + 1
            nodes, (l_walk, l_neg), _ = glx.unique([walks, negs])
            zt, zc = target(nodes, distinct=True), context(nodes, distinct=True)
            l_src = l_walk[:, w_src].reshape(-1).contiguous()   # local positions of the window pairs
            l_dst = l_walk[:, w_dst].reshape(-1).contiguous()
            pos = pair_dot(zt, l_src, zc, l_dst)                                                     # [B * pairs]
            neg = pair_dot(zt, l_walk.reshape(-1), zc, l_neg.view(-1, NEGATIVES))                    # [B * 10, K]
            loss = sigmoid_cross_entropy_loss(pos, neg)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        half = len(losses) // 2
        history.append(losses)
        if not quiet:
            print("run %d epoch %d: loss %.4f -> %.4f (first / second half of the epoch), %d walks in %.2f s, bits %s"
                  % (run, epoch, np.mean(losses[:half]), np.mean(losses[half:]), len(losses) * BATCH,
                     time.time() - t0, ",".join(float(x).hex() for x in losses)))
    negative.close()
    g.close()
    return history


if __name__ == "__main__":
    _, same_bits = main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
    sys.exit(0 if same_bits else 1)
