"""Pair scores on the id stream of a real C3 step (RMAT 10 M / 100 M, EdgeWeight [25, 10], 65,536 seeds),
deduplicated (glx.unique): B = 65,536 sources (the seeds' positions in the distinct set), each scored at dim = 256,
heads = 1, against K in {1, 5, 20} candidates (the positions of the first K hop-2 slots under the seed) over one
[distinct nodes, 256] matrix z that needs a gradient from both sides:

  1. forward + both backwards through graphlearn.nn.pytorch.pair_dot(z, src, z, cand) against torch's own autograd of
     (z[src].unsqueeze(1) * z[cand]).sum(-1) (two gathers + two index_add_ with float atomics) on the same tensors, in
     the same process, legs interleaved; the largest |difference| of the outputs and of z.grad; whether each leg
     repeats its own z.grad bit for bit; peak memory of each leg;
  2. the entry points apart (glx_pair_dot, glx_pair_dot_backward side 0 and side 1) with the bytes each must move.

The parent of this change has no such entry point, so torch is the only baseline.  One process, HIP events, 3 warm-up +
10 timed repetitions, medians.  Nothing here is a requirement of the test suite.
Usage: python scripts/r14/pair_dot_probe.py [nodes] [edges] [batch] > profiles/r14/pair_dot.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import pair_dot  # noqa: E402

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]
D = 256
KS = (1, 5, 20)


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
    M = int(nodes.shape[0])
    l_src = inverse[0].reshape(-1).contiguous()            # [B]
    under = inverse[2].reshape(B, -1)                      # [B, 250]: the hop-2 slots under each seed
    del g, hops
    torch.cuda.empty_cache()
    z = torch.randn(M, D, device=dev, generator=gen)
    print("%d sources over %d distinct nodes" % (B, M), flush=True)

    for K in KS:
        cand = under[:, :K].contiguous()                   # [B, K]
        n = B * K
        grad_out = torch.randn(B, K, device=dev, generator=gen)

        def engine():
            zr = z.detach().requires_grad_(True)
            out = pair_dot(zr, l_src, zr, cand)
            out.backward(grad_out)
            return out.detach(), zr.grad

        def plain():
            zr = z.detach().requires_grad_(True)
            out = (zr[l_src].unsqueeze(1) * zr[cand]).sum(-1)
            out.backward(grad_out)
            return out.detach(), zr.grad

        print("\n[1] K = %d (%d pairs): forward + both backwards, pair_dot against torch's gather * gather" % (K, n),
              flush=True)
        t = timed({"engine": engine, "torch": plain})
        e_ms = show("pair_dot(z, src, z, cand) fwd + bwd", t["engine"])
        t_ms = show("(z[src].unsqueeze(1) * z[cand]).sum(-1) fwd + bwd", t["torch"])
        print("  torch / engine: %.2f" % (t_ms / e_ms), flush=True)
        for name, fn in (("engine", engine), ("torch", plain)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            a = fn()
            peak = torch.cuda.max_memory_allocated() - base
            b = fn()
            same = bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
            print("  %-6s peak memory above the inputs %7.3f GB; repeats its own z.grad bit for bit: %s"
                  % (name, peak / 1e9, same), flush=True)
            del a, b
        got, want = engine(), plain()
        print("  largest |engine - torch|: out %.3e   z.grad %.3e"
              % tuple(float((p - q).abs().max()) for p, q in zip(got, want)), flush=True)
        del got, want

        print("[2] K = %d: the entry points apart" % K, flush=True)
        flat, gflat = cand.reshape(-1), grad_out.reshape(n, 1)
        t = timed({
            "fwd": lambda: glx.pair_dot(z, l_src, z, flat, repeat=K),
            "bwd_a": lambda: glx.pair_dot_backward(0, l_src, flat, gflat, z, M, repeat=K),
            "bwd_b": lambda: glx.pair_dot_backward(1, l_src, flat, gflat, z, M, repeat=K),
        })
        row = D * 4
        for key, name, nbytes in (
                ("fwd", "glx_pair_dot", B * (row + 8) + n * (row + 8 + 4)),
                ("bwd_a", "glx_pair_dot_backward side 0 (transpose of %d + reduce)" % B, n * (row + 8 + 4) + B * 8 + M * row),
                ("bwd_b", "glx_pair_dot_backward side 1 (transpose of %d + reduce)" % n, n * (2 * row + 8 + 4) + M * row)):
            ms = show(name, t[key])
            print("    at least %.3f GB by the shapes -> %.1f GB/s" % (nbytes / 1e9, nbytes / max(ms, 1e-6) / 1e6),
                  flush=True)


if __name__ == "__main__":
    main()
