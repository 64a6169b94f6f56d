"""The bfloat16 training path on the id stream of a real C3 step (RMAT 10 M / 100 M, EdgeWeight [25, 10], 65,536
seeds), deduplicated (glx.unique) and run at dim = 256 over a [distinct nodes, 256] matrix z, heads 1 and 4:

  segment_aggregate (mean, max) and weighted_segment_aggregate over hop 2 (16.4 M positions into 1.64 M segments of 10),
  pair_dot of every hop-1 slot against K = 5 random rows of z (both sides the one table),

each with three legs in one process, interleaved:

  f32     z float32                              what a float32 model runs
  cast    z bfloat16, the op called on z.float() what a model under bfloat16 autocast had to write before
  bf16    z bfloat16, handed to the op as it is  the native path

Forward and backward are timed apart with device events (3 warm-up + 10 timed repetitions, medians), and the peak
memory of forward + backward above the tables is reported per leg.  The bf16 leg's outputs are first checked bit for
bit against the cast leg's, and its z.grad against the cast leg's float32 gradient rounded once.  By the shapes the
forward's gathered bytes halve; the backward only halves its [M, D] write -- grad_out stays float32 and its gathers
dominate -- so the backward may not move.  Nothing here is a requirement of the test suite.
Usage: python scripts/bf16_training_probe.py [nodes] [edges] [batch] > profiles/bf16_training/probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import pair_dot, segment_aggregate, weighted_segment_aggregate  # noqa: E402

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]
D, K = 256, 5
LEGS = ("f32", "cast", "bf16")


def run_leg(leg, z32, z16, op, grad_out, times=None):
    """one forward + backward of `op` on the leg's leaf; appends (forward ms, backward ms) to `times`"""
    leaf = (z32 if leg == "f32" else z16).detach().requires_grad_(True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    out = op(leaf.float() if leg == "cast" else leaf)
    ev[1].record()
    ev[2].record()
    out.backward(grad_out)
    ev[3].record()
    ev[3].synchronize()
    if times is not None:
        times.append((ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])))
    return out.detach(), leaf.grad


def median(v):
    return sorted(v)[len(v) // 2]


def probe(name, z32, z16, op, out_shape, gen, note=None):
    grad_out = torch.randn(out_shape, device=z32.device, generator=gen)
    # correctness first: the native leg against the cast leg
    o_c, g_c = run_leg("cast", z32, z16, op, grad_out)
    o_b, g_b = run_leg("bf16", z32, z16, op, grad_out)
    same_out = bool(torch.equal(o_c.view(torch.int32), o_b.view(torch.int32)))
    same_grad = bool(torch.equal(g_c.view(torch.int16), g_b.view(torch.int16)))
    assert g_b.dtype == torch.bfloat16 and o_b.dtype == torch.float32
    del o_c, g_c, o_b, g_b
    times = {leg: [] for leg in LEGS}
    for rep in range(WARMUP + REPS):
        for leg in (LEGS if rep % 2 == 0 else LEGS[::-1]):
            run_leg(leg, z32, z16, op, grad_out, times[leg] if rep >= WARMUP else None)
    peaks = {}
    for leg in LEGS:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run_leg(leg, z32, z16, op, grad_out)
        peaks[leg] = (torch.cuda.max_memory_allocated() - base) / 1e9
    print("\n%s   (bf16 out == cast out bit for bit: %s; bf16 z.grad == cast z.grad bit for bit: %s)"
          % (name, same_out, same_grad), flush=True)
    if note:
        print("  " + note, flush=True)
    for leg in LEGS:
        f, b = [t[0] for t in times[leg]], [t[1] for t in times[leg]]
        print("  %-5s forward median %8.3f ms (min %8.3f max %8.3f)   backward median %8.3f ms (min %8.3f max %8.3f)   "
              "peak above the tables %6.2f GB" % (leg, median(f), min(f), max(f), median(b), min(b), max(b), peaks[leg]),
              flush=True)
    fm = {leg: median([t[0] for t in times[leg]]) for leg in LEGS}
    bm = {leg: median([t[1] for t in times[leg]]) for leg in LEGS}
    print("  bf16 / cast: forward %.3f backward %.3f     bf16 / f32: forward %.3f backward %.3f"
          % (fm["bf16"] / fm["cast"], bm["bf16"] / bm["cast"], fm["bf16"] / fm["f32"], bm["bf16"] / bm["f32"]), flush=True)
    del grad_out
    torch.cuda.empty_cache()


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    dev = torch.device("cuda", 0)
    print("device: %s   graph: RMAT %d vertices / %d edges   EdgeWeight %s   %d seeds   dim %d"
          % (torch.cuda.get_device_name(0), V, E, FANOUTS, B, D), flush=True)
    src, dst, w = synth.rmat_edges_torch(V, E, 1, dev, weighted=True)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, w)
    del src, dst, w
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    hops = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, FANOUTS, seed=42, call_counter=0)
    nodes, inverse, _ = glx.unique([seeds, hops[0][0], hops[1][0]])
    index = inverse[2].reshape(-1).contiguous()
    slots = inverse[1].reshape(-1).contiguous()
    n, M, f = int(index.numel()), int(nodes.shape[0]), FANOUTS[1]
    S = n // f
    del g, hops
    torch.cuda.empty_cache()
    z16 = torch.randn(M, D, device=dev, generator=gen).to(torch.bfloat16)
    z32 = z16.float()  # the same values: the legs differ in storage only
    neg = torch.randint(0, M, (int(slots.numel()), K), device=dev, generator=gen)
    print("hop 2: %d positions into %d segments of %d over %d distinct nodes; pair_dot: %d sources x %d"
          % (n, S, f, M, int(slots.numel()), K), flush=True)
    print("legs: f32 = float32 z; cast = bfloat16 z through z.float(); bf16 = bfloat16 z natively", flush=True)

    for op_name in ("mean", "max"):
        probe("segment_aggregate %s" % op_name, z32, z16,
              lambda z, o=op_name: segment_aggregate(z, index, S, op=o), (S, D), gen)
    for heads in (1, 4):
        wts = torch.softmax(torch.randn(S, f, heads, device=dev, generator=gen), dim=1).reshape(n, heads).contiguous()
        probe("weighted_segment_aggregate sum, heads %d" % heads, z32, z16,
              lambda z, wt=wts: weighted_segment_aggregate(z, index, wt, S, op="sum"), (S, D), gen)
        del wts
    for heads in (1, 4):
        probe("pair_dot K = %d, heads %d (one table on both sides)" % (K, heads), z32, z16,
              lambda z, h=heads: pair_dot(z, slots, z, neg, heads=h), (int(slots.numel()), K, heads), gen,
              note="(one table on both sides: the bf16 leg adds its two rounded gradients in bfloat16 -- torch's add -- "
                   "where the cast leg rounds their float32 sum, so the two z.grad need not agree to the bit)")


if __name__ == "__main__":
    main()
