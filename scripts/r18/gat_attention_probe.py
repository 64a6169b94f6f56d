"""A first measurement of the fused GAT attention (glx_gat_attention, graphlearn.nn.pytorch.gat_attention): forward +
backward of the attention step of a GAT layer -- from the two [M, H] halves of the logit to the coefficients and back
to the halves' gradients -- three ways:

  fused      s = gather_rows(src_e, seed_local); gat_attention(s, dst_e, local, S, counts, dropout): one kernel per
             direction, the Sum backward of the [S, H] gather and the narrow row gradient of dst_e
  composite  what examples/train_gat_full.py writes with the ops that existed before: repeat_interleave,
             two gather_rows, add, leaky_relu, segment_softmax, torch.nn.functional.dropout
  torch      the same in plain torch: two index selects (index_add_ going back), scatter_reduce(amax), exp,
             index_add_, divide, dropout

on
  dense    the hop-2 stream of a C3 step (EdgeWeight [25, 10], 65,536 seeds: 16.4 M positions) as 1.64 M segments of
           10 with explicit counts, the neighbours' rows drawn from 2^20 distinct nodes;
  ragged   a FullSampler hop over 65,536 seeds of the RMAT 10 M / 100 M graph, hubs included, relabelled by glx.unique,
at heads 1 and 4 and dropout 0 and 0.4.

One process, HIP events, 3 warm-up + 10 timed repetitions, legs interleaved, medians.  Nothing here is a requirement
of the test suite, and no ratio is promised.
Usage: python scripts/r18/gat_attention_probe.py [nodes] [edges] [batch] > profiles/r18/gat_attention.txt"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import gat_attention, gather_rows, segment_softmax  # noqa: E402

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]
SLOPE = 0.2


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
    print("  %-74s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]), flush=True)
    return med


def torch_softmax(e, seg, S):
    H = e.shape[1]
    idx = seg[:, None].expand(-1, H)
    m = torch.full((S, H), -math.inf, device=e.device).scatter_reduce(0, idx, e.detach(), "amax")
    t = torch.exp(e - m[seg])
    z = torch.zeros((S, H), device=e.device).index_add_(0, seg, t)
    return t / z[seg]


def compare(title, M, local0, local, counts, heads, p, gen, dev):
    n, S = int(local.numel()), int(local0.numel())
    src_e = torch.randn(M, heads, device=dev, generator=gen)
    dst_e = torch.randn(M, heads, device=dev, generator=gen)
    g = torch.randn(n, heads, device=dev, generator=gen)
    seg = torch.repeat_interleave(torch.arange(S, device=dev), counts.long(), output_size=n)
    step = [0]

    def leaves():
        return src_e.detach().requires_grad_(True), dst_e.detach().requires_grad_(True)

    def fused():
        a, b = leaves()
        step[0] += 1
        out = gat_attention(gather_rows(a, local0), b, local, S, counts=counts, negative_slope=SLOPE, dropout=p,
                            seed=1, call=step[0])
        out.backward(g)
        return out.detach(), a.grad, b.grad

    def composite():
        a, b = leaves()
        seed_of = torch.repeat_interleave(local0, counts.long(), output_size=n)
        e = torch.nn.functional.leaky_relu(gather_rows(a, seed_of) + gather_rows(b, local), SLOPE)
        out = segment_softmax(e.contiguous(), S, counts=counts)
        if p:
            out = torch.nn.functional.dropout(out, p)
        out.backward(g)
        return out.detach(), a.grad, b.grad

    def plain():
        a, b = leaves()
        e = torch.nn.functional.leaky_relu(a[local0[seg]] + b[local], SLOPE)
        out = torch_softmax(e, seg, S)
        if p:
            out = torch.nn.functional.dropout(out, p)
        out.backward(g)
        return out.detach(), a.grad, b.grad

    print("\n%s, heads = %d, dropout = %.1f: %d positions in %d segments, %d rows" % (title, heads, p, n, S, M),
          flush=True)
    t = timed({"fused": fused, "composite": composite, "torch": plain})
    f_ms = show("fused: gather_rows [S, H] + gat_attention, fwd + bwd", t["fused"])
    c_ms = show("composite: 2 gather_rows + add + leaky_relu + segment_softmax + dropout, fwd + bwd", t["composite"])
    t_ms = show("plain torch, fwd + bwd", t["torch"])
    nbytes = n * (8 * 2 + heads * 4 * 4)  # rows twice; soft + alpha out, soft + grad_alpha in, grad_e out is the 5th
    print("  composite / fused: %.2f   plain torch / fused: %.2f   (fused moves at least %.2f GB over [n]-sized "
          "arrays -> %.1f GB/s)" % (c_ms / f_ms, t_ms / f_ms, nbytes / 1e9, nbytes / max(f_ms, 1e-6) / 1e6), flush=True)
    step[0] = 100
    a = fused()
    step[0] = 100
    b = fused()
    print("  fused repeats alpha / src_e.grad / dst_e.grad bit for bit under one (seed, call): %s"
          % " / ".join(str(bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))) for x, y in zip(a, b)),
          flush=True)
    if not p:
        want = composite()
        print("  largest |fused - composite|: alpha %.3e   src_e.grad %.3e   dst_e.grad %.3e"
              % tuple(float((x - y).abs().max()) for x, y in zip(a, want)), flush=True)
    else:
        print("  share of the consumed coefficients dropped: %.4f" % float((a[0] == 0).float().mean()), flush=True)
    return f_ms, c_ms


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    dev = torch.device("cuda", 0)
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    summary = []

    f = FANOUTS[1]
    S = B * FANOUTS[0]
    n, M = S * f, 1 << 20
    local0 = torch.randint(0, M, (S,), device=dev, generator=gen)
    local = torch.randint(0, M, (n,), device=dev, generator=gen)
    counts = torch.full((S,), f, dtype=torch.int32, device=dev)
    for heads in (1, 4):
        for p in (0.0, 0.4):
            ms = compare("dense (C3 hop 2, EdgeWeight %s, %d seeds) as segments of %d" % (FANOUTS, B, f), M, local0, local,
                         counts, heads, p, gen, dev)
            summary.append(("dense", heads, p) + ms)
    del local0, local, counts
    torch.cuda.empty_cache()

    print("\ngraph: RMAT %d vertices / %d edges, FullSampler over %d seeds" % (V, E, B), flush=True)
    src, dst, _ = synth.rmat_edges_torch(V, E, 1, dev, weighted=False)
    pool = torch.unique(src)
    graph = glx.Graph.from_edges(src, dst, sort_by_weight=False)
    del src, dst
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    deg, nbr, _ = graph.sample_full(seeds, 0)
    nodes, (local0, local), _ = glx.unique([seeds, nbr])
    print("ragged hop: %d positions in %d segments over %d distinct nodes; longest %d, median %d, %d segments above 1024 "
          "positions" % (int(nbr.numel()), int(deg.numel()), int(nodes.numel()), int(deg.max()), int(deg.median()),
                         int((deg > 1024).sum())), flush=True)
    M = int(nodes.numel())
    del graph, nbr, nodes
    torch.cuda.empty_cache()
    for heads in (1, 4):
        for p in (0.0, 0.4):
            ms = compare("ragged FullSampler hop", M, local0, local, deg, heads, p, gen, dev)
            summary.append(("ragged", heads, p) + ms)

    print("\nsummary (medians, ms): stream heads dropout fused composite composite/fused")
    for stream, heads, p, f_ms, c_ms in summary:
        print("  %-6s %d %.1f %9.3f %9.3f %6.2f" % (stream, heads, p, f_ms, c_ms, c_ms / f_ms))


if __name__ == "__main__":
    main()
