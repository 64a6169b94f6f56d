"""Differentiable aggregation on the id stream of a real C3 step (RMAT 10 M / 100 M, EdgeWeight [25, 10], 65,536 seeds:
18.1 M slots), deduplicated (glx.unique) and reduced at dim = 256 over a [distinct nodes, 256] matrix that needs a
gradient -- hop 2, 16.4 M positions into 1.64 M segments of 10:

  1. forward + backward of Mean and Max through graphlearn.nn.pytorch.segment_aggregate against torch's own autograd of
     x[index].view(S, f, D).mean(1) / .amax(1) (gather + index_add_ with float atomics) on the same stream, in the
     same process, legs interleaved; the largest |difference| of the two gradients; whether each leg repeats its own
     gradient bit for bit; peak memory of each leg (the [n, D] gather is 16.8 GB at this size);
  2. the backward's two halves apart: the transpose (keys + stable radix sort + row_ptr) and the reduce.  They are one
     entry point; the transpose is timed as a backward at dim = 1 (its transpose is the same, its reduce reads 4 B per
     position), the reduce as the difference;
  3. the longest row list of the batch next to its share of the reduce: the reduce of the same request with the
     longest list's positions redirected to an unreferenced row range is timed beside the real one (one lane group
     walks a long list alone: the contract's order requires it).

One process, HIP events, 3 warm-up + 10 timed repetitions.
Usage: python scripts/r11/agg_backward_probe.py [nodes] [edges] [batch] > profiles/r11/agg_backward.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import segment_aggregate  # noqa: E402

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]
D = 256


def timed(legs):
    times = {k: [] for k in legs}
    for rep in range(WARMUP + REPS):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= WARMUP:
                times[name].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in times.items()}


def show(name, ts):
    med = ts[len(ts) // 2]
    print("  %-58s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]), flush=True)
    return med


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
    n, M, f = int(index.numel()), int(nodes.shape[0]), FANOUTS[1]
    S = n // f
    del g, hops
    torch.cuda.empty_cache()
    x = torch.randn(M, D, device=dev, generator=gen)
    grad_out = torch.randn(S, D, device=dev, generator=gen)
    lengths = torch.bincount(index, minlength=M)
    longest, hub = int(lengths.max()), int(lengths.argmax())
    print("hop 2: %d positions into %d segments of %d over %d distinct nodes; longest row list %d (median %d)"
          % (n, S, f, M, longest, int(lengths.median())), flush=True)

    def engine(op):
        xr = x.detach().requires_grad_(True)
        segment_aggregate(xr, index, S, op=op).backward(grad_out)
        return xr.grad

    def plain(op):
        xr = x.detach().requires_grad_(True)
        gathered = xr[index].view(S, f, D)
        (gathered.mean(1) if op == "mean" else gathered.amax(1)).backward(grad_out)
        return xr.grad

    print("\n[1] forward + backward, segment_aggregate against torch's gather + reduction", flush=True)
    for op in ("mean", "max"):
        t = timed({"engine " + op: lambda: engine(op), "torch  " + op: lambda: plain(op)})
        e_ms, t_ms = show("segment_aggregate(op=%r) fwd + bwd" % op, t["engine " + op]), show(
            "x[index].view(S, f, D).%s(1) fwd + bwd" % ("mean" if op == "mean" else "amax"), t["torch  " + op])
        print("  torch / engine: %.2f" % (t_ms / e_ms), flush=True)
        for name, fn in (("engine", engine), ("torch", plain)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            a = fn(op)
            peak = torch.cuda.max_memory_allocated() - base
            same = bool(torch.equal(a.view(torch.int32), fn(op).view(torch.int32)))
            print("  %-6s %-4s peak memory above the inputs %7.2f GB; repeats its own gradient bit for bit: %s"
                  % (name, op, peak / 1e9, same), flush=True)
        print("  largest |engine - torch| gradient element (%s): %.3e" % (op, float((engine(op) - plain(op)).abs().max())),
              flush=True)

    print("\n[2] the backward's halves (Mean, implied layout)", flush=True)
    go1 = grad_out[:, :1].contiguous()
    t = timed({"whole": lambda: glx.aggregate_backward(glx.MEAN, index, None, grad_out, M),
               "dim1": lambda: glx.aggregate_backward(glx.MEAN, index, None, go1, M)})
    whole, dim1 = show("glx_aggregate_backward, dim 256", t["whole"]), show(
        "glx_aggregate_backward, dim 1 (~ the transpose alone)", t["dim1"])
    print("  reduce at dim 256 ~ %.3f ms; it reads %d x 1 KiB grad_out rows and writes %d x 1 KiB: %.2f GB -> %.1f GB/s"
          % (whole - dim1, n, M, (n + M) * D * 4 / 1e9, (n + M) * D * 4 / max(whole - dim1, 1e-6) / 1e6), flush=True)

    print("\n[3] the longest list", flush=True)
    spread = index.clone()
    at = torch.nonzero(index == hub).reshape(-1)
    spread[at] = M + torch.arange(at.numel(), device=dev)  # rows M .. M + longest - 1: one position each
    t = timed({"real": lambda: glx.aggregate_backward(glx.MEAN, index, None, grad_out, M + longest),
               "spread": lambda: glx.aggregate_backward(glx.MEAN, spread, None, grad_out, M + longest)})
    real, flat = show("backward, longest list %d (row %d)" % (longest, hub), t["real"]), show(
        "backward, that list spread over %d rows of their own" % longest, t["spread"])
    print("  the list is %.4f of the positions and costs %.3f ms = %.3f of the reduce's %.3f ms"
          % (longest / n, real - flat, (real - flat) / max(whole - dim1, 1e-6), whole - dim1), flush=True)


if __name__ == "__main__":
    main()
