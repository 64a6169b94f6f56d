"""Weighted segment aggregation on the id stream of a real C3 step (RMAT 10 M / 100 M, EdgeWeight [25, 10], 65,536
seeds: 18.1 M slots), deduplicated (glx.unique) and reduced at dim = 256 over a [distinct nodes, 256] matrix -- hop 2,
16.4 M positions into 1.64 M segments of 10 -- with heads = 1 and heads = 4 weights that need a gradient too:

  1. forward + both backwards through graphlearn.nn.pytorch.weighted_segment_aggregate against torch's own autograd of
     (z[index] * w.repeat_interleave(C, 1)).view(S, f, D).sum(1) (gather + index_add_ with float atomics) on the same
     tensors, in the same process, legs interleaved; the largest |difference| of the outputs and of both gradients;
     whether each leg repeats its own gradients bit for bit; peak memory of each leg (the [n, D] gather is 16.8 GB at
     this size, and torch keeps the product as well);
  2. the three entry points apart (glx_aggregate_weighted, _backward_x, _backward_w) with the bytes each must move,
     _backward_w also with explicit counts: there every lane group finds its position's segment by a binary search over
     the prefix sums before it reads a row, which the implied layout does not need -- the difference is that search.

One process, HIP events, 3 warm-up + 10 timed repetitions.  Nothing here is a requirement of the test suite.
Usage: python scripts/r12/agg_weighted_probe.py [nodes] [edges] [batch] > profiles/r12/agg_weighted.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import weighted_segment_aggregate  # noqa: E402

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
    print("  %-62s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]), flush=True)
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
    counts = torch.full((S,), f, dtype=torch.int32, device=dev)
    print("hop 2: %d positions into %d segments of %d over %d distinct nodes" % (n, S, f, M), flush=True)

    for heads in (1, 4):
        C = D // heads
        # attention-like coefficients: a softmax over the fan-out
        wts = torch.softmax(torch.randn(S, f, heads, device=dev, generator=gen), dim=1).reshape(n, heads).contiguous()

        def engine():
            xr, wr = x.detach().requires_grad_(True), wts.detach().requires_grad_(True)
            out = weighted_segment_aggregate(xr, index, wr, S, op="sum")
            out.backward(grad_out)
            return out.detach(), xr.grad, wr.grad

        def plain():
            xr, wr = x.detach().requires_grad_(True), wts.detach().requires_grad_(True)
            out = (xr[index] * wr.repeat_interleave(C, 1)).view(S, f, D).sum(1)
            out.backward(grad_out)
            return out.detach(), xr.grad, wr.grad

        print("\n[1] heads = %d: forward + both backwards, weighted_segment_aggregate against torch's gather * w" % heads,
              flush=True)
        t = timed({"engine": engine, "torch": plain})
        e_ms = show("weighted_segment_aggregate fwd + bwd", t["engine"])
        t_ms = show("(z[index] * w).view(S, f, D).sum(1) fwd + bwd", t["torch"])
        print("  torch / engine: %.2f" % (t_ms / e_ms), flush=True)
        for name, fn in (("engine", engine), ("torch", plain)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            a = fn()
            peak = torch.cuda.max_memory_allocated() - base
            b = fn()
            same = [bool(torch.equal(p.view(torch.int32), q.view(torch.int32))) for p, q in zip(a[1:], b[1:])]
            print("  %-6s peak memory above the inputs %7.2f GB; repeats its own x.grad / w.grad bit for bit: %s / %s"
                  % (name, peak / 1e9, same[0], same[1]), flush=True)
            del a, b
        got, want = engine(), plain()
        print("  largest |engine - torch|: out %.3e   x.grad %.3e   w.grad %.3e"
              % tuple(float((p - q).abs().max()) for p, q in zip(got, want)), flush=True)
        del got, want

        print("[2] heads = %d: the entry points apart (Sum, implied layout)" % heads, flush=True)
        t = timed({
            "fwd": lambda: glx.aggregate_weighted(glx.SUM, x, index, wts, S),
            "bwd_x": lambda: glx.aggregate_weighted_backward_x(glx.SUM, index, wts, None, grad_out, M),
            "bwd_w": lambda: glx.aggregate_weighted_backward_w(glx.SUM, x, index, heads, None, grad_out),
            "bwd_w_cnt": lambda: glx.aggregate_weighted_backward_w(glx.SUM, x, index, heads, counts, grad_out),
        })
        row = D * 4
        for key, name, nbytes in (
                ("fwd", "glx_aggregate_weighted", n * (row + 8 + 4 * heads) + S * row),
                ("bwd_x", "glx_aggregate_weighted_backward_x (transpose + reduce)", n * (row + 8 + 4 * heads) + M * row),
                ("bwd_w", "glx_aggregate_weighted_backward_w", n * (row + 8 + 4 * heads) + S * row),
                ("bwd_w_cnt", "glx_aggregate_weighted_backward_w, explicit counts",
                 n * (row + 8 + 4 * heads) + S * row)):
            ms = show(name, t[key])
            print("    at least %.2f GB by the shapes (rows read once per position) -> %.1f GB/s"
                  % (nbytes / 1e9, nbytes / max(ms, 1e-6) / 1e6), flush=True)
        del wts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
