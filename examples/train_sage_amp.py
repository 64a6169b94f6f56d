"""train_sage_dedup.py's model under torch.autocast("cuda", dtype=torch.bfloat16): the usual way to train on an MI355X.

    python examples/train_sage_amp.py [epochs] [vertices]              (needs one GPU)

Inside the autocast region `z = relu(enc(batch.x_nodes))` is bfloat16.  segment_aggregate and gather_rows read it as
it is -- every row upcast exactly as it is loaded, summed in float32 in the float32 order -- and answer in float32;
going back, glx_aggregate_backward_ex writes z.grad in bfloat16 itself: the float32 gradient rounded once per element,
with no float32 [M, H] copy of z kept for the backward and no float32 [M, H] gradient allocated.  z feeds three ops, so
torch adds their three bfloat16 gradients in bfloat16 (its roundings, in a fixed order).  Nothing uses a float atomic,
so a (seed, epoch, batch) triple still reproduces its loss bit for bit.

The script trains twice from one seed and exits non-zero unless the loss falls inside the first epoch and the two runs
print the same per-batch losses, bit for bit.
"""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_sage_dedup as base  # noqa: E402  (the graph, the model and the paths of the float32 example)
import torch  # noqa: E402
import graphlearn as gl  # noqa: E402


def _train(epochs, vertices, quiet):
    d = tempfile.mkdtemp(prefix="glx_sage_amp_")
    npath, epath = base.write_sources(d, vertices)
    gl.set_padding_mode(gl.CIRCULAR)
    gl.set_sampling_seed(7)
    torch.manual_seed(0)
    g = gl.Graph() \
        .node(npath, "n", gl.Decoder(labeled=True, attr_types=["float"] * base.DIM)) \
        .edge(epath, ("n", "n", "e"), gl.Decoder()) \
        .init()
    loader = gl.NeighborLoader(g, "n", ["e", "e"], list(base.FANOUT), batch_size=base.BATCH, strategy="random",
                               shuffle=True, dedup=True, node_columns=("labels",))
    model = base.DedupSage(base.DIM, 64, base.CLASSES).cuda()  # float32 master weights; autocast casts per op
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    history = []
    for epoch in range(epochs):
        t0, seen, correct, losses = time.time(), 0, 0, []
        for batch in loader:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = model(batch)
                labels = batch.y.long()
                loss = torch.nn.functional.cross_entropy(logits.float(), labels)
            opt.zero_grad()
            loss.backward()  # bfloat16 needs no loss scaling
            opt.step()
            seen += labels.shape[0]
            correct += int((logits.argmax(1) == labels).sum())
            losses.append(float(loss.detach()))
        half = len(losses) // 2
        history.append((losses, correct / seen))
        if not quiet:
            print("epoch %d: loss %.4f -> %.4f (first / second half of the epoch), accuracy %.3f, %d vertices in %.2f s, "
                  "bits %s" % (epoch, np.mean(losses[:half]), np.mean(losses[half:]), correct / seen, seen,
                               time.time() - t0, ",".join(float(x).hex() for x in losses)))
    g.close()
    return history


def main(epochs=2, vertices=20000, quiet=False):
    # the dense layers' own backward must not use atomics either (split-K GEMMs), or the loss would not reproduce
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        runs = [_train(epochs, vertices, quiet) for _ in range(2)]
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    losses = runs[0][0][0]
    half = len(losses) // 2
    falls = half > 0 and np.mean(losses[half:]) < np.mean(losses[:half])
    same = [[float(x).hex() for x in ls] for ls, _ in runs[0]] == [[float(x).hex() for x in ls] for ls, _ in runs[1]]
    print("loss falls inside the first epoch: %s; two runs from one seed give the same bits: %s" % (falls, same))
    return 0 if falls and same else 1


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 2, int(sys.argv[2]) if len(sys.argv) > 2 else 20000))
