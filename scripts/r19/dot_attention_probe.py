"""A first measurement of the fused dot-product attention (glx_dot_attention, graphlearn.nn.pytorch.dot_attention):
forward + backward of a transformer-style layer's attention -- from the [M, D] query / key / value rows (and the
[n, D] edge term) to the [S, D] output and back to their gradients -- three ways:

  fused      q = gather_rows(q_nodes, seed_local); dot_attention(q, k, v, local, S, counts, edge, heads): one kernel
             going forward, one per-segment kernel and two row gradients on one transpose going back
  composite  the ops that existed before: pair_dot(q, segment_of_position, k, local) * scale, segment_softmax,
             weighted_segment_aggregate(v, local, alpha); with an edge term kk = gather_rows(k, local) + edge and
             vv = gather_rows(v, local) + edge are materialised first and take the place of k and v
  torch      the same in plain torch: index selects (index_add_ going back), scatter_reduce(amax), exp, index_add_

on
  dense    the deduplicated hop-2 stream of a C3 step (EdgeWeight [25, 10], 65,536 seeds: 16.4 M positions) as 1.64 M
           segments of 10 with explicit counts, the neighbours' rows drawn from 2^20 distinct nodes;
  ragged   a FullSampler hop over 65,536 seeds of the RMAT 10 M / 100 M graph, hubs included, relabelled by glx.unique,
at dim 256, heads 4, each with and without the edge term, and it reports the longest segment's share of the fused time
(the same call on that segment alone: one lane group walks it).

One process, HIP events, 3 warm-up + 10 timed repetitions, legs interleaved, medians.  A leg that does not fit the
device's memory is reported as such.  Nothing here is a requirement of the test suite, and no ratio is promised.
Usage: python scripts/r19/dot_attention_probe.py [nodes] [edges] [batch] > profiles/r19/dot_attention.txt"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import (dot_attention, gather_rows, pair_dot, segment_softmax,  # noqa: E402
                                   weighted_segment_aggregate)

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]
DIM, HEADS = 256, 4


def timed(legs):
    times = {k: [] for k in legs}
    for rep in range(WARMUP + REPS):
        for name, fn in legs.items():
            if times[name] is None:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            try:
                a.record()
                fn()
                b.record()
                b.synchronize()
            except torch.cuda.OutOfMemoryError:
                times[name] = None
                torch.cuda.empty_cache()
                continue
            if rep >= WARMUP:
                times[name].append(a.elapsed_time(b))
    return {k: (None if v is None else sorted(v)) for k, v in times.items()}


def show(name, ts):
    if ts is None:
        print("  %-78s does not fit the device's memory" % name, flush=True)
        return float("nan")
    med = ts[len(ts) // 2]
    print("  %-78s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]), flush=True)
    return med


def torch_softmax(e, seg, S):
    H = e.shape[1]
    idx = seg[:, None].expand(-1, H)
    m = torch.full((S, H), -math.inf, device=e.device).scatter_reduce(0, idx, e.detach(), "amax")
    t = torch.exp(e - m[seg])
    z = torch.zeros((S, H), device=e.device).index_add_(0, seg, t)
    return t / z[seg]


def compare(title, M, local0, local, counts, with_edge, gen, dev):
    n, S = int(local.numel()), int(local0.numel())
    C = DIM // HEADS
    scale = 1.0 / math.sqrt(C)
    tabs = [torch.randn(M, DIM, device=dev, generator=gen) * 0.25 for _ in range(3)]
    edge0 = torch.randn(n, DIM, device=dev, generator=gen) * 0.25 if with_edge else None
    g = torch.randn(S, DIM, device=dev, generator=gen)
    seg = torch.repeat_interleave(torch.arange(S, device=dev), counts.long(), output_size=n)
    every = torch.arange(n, device=dev)

    def leaves():
        ts = [t.detach().requires_grad_(True) for t in tabs]
        return ts + [None if edge0 is None else edge0.detach().requires_grad_(True)]

    def grads(out, ls):
        out.backward(g)
        return [out.detach()] + [x.grad for x in ls if x is not None]

    def fused():
        ls = leaves()
        qa, k, v, e = ls
        return grads(dot_attention(gather_rows(qa, local0), k, v, local, S, counts=counts, edge=e, heads=HEADS), ls)

    def composite():
        ls = leaves()
        qa, k, v, e = ls
        q = gather_rows(qa, local0)
        if e is None:
            logit = pair_dot(q, seg, k, local, heads=HEADS) * scale
            alpha = segment_softmax(logit.contiguous(), S, counts=counts)
            return grads(weighted_segment_aggregate(v, local, alpha, S, counts=counts), ls)
        kk, vv = gather_rows(k, local) + e, gather_rows(v, local) + e
        logit = pair_dot(q, seg, kk, every, heads=HEADS) * scale
        alpha = segment_softmax(logit.contiguous(), S, counts=counts)
        return grads(weighted_segment_aggregate(vv, every, alpha, S, counts=counts), ls)

    def plain():
        ls = leaves()
        qa, k, v, e = ls
        kk, vv = k[local], v[local]
        if e is not None:
            kk, vv = kk + e, vv + e
        logit = (qa[local0][seg] * kk).view(n, HEADS, C).sum(-1) * scale
        alpha = torch_softmax(logit, seg, S)
        out = torch.zeros(S, DIM, device=dev).index_add_(0, seg, (alpha[:, :, None] * vv.view(n, HEADS, C)).view(n, DIM))
        return grads(out, ls)

    print("\n%s, %s: %d positions in %d segments, %d rows of %d columns in %d heads"
          % (title, "with an edge term" if with_edge else "no edge term", n, S, M, DIM, HEADS), flush=True)
    t = timed({"fused": fused, "composite": composite, "torch": plain})
    f_ms = show("fused: gather_rows [S, D] + dot_attention, fwd + bwd", t["fused"])
    c_ms = show("composite: pair_dot + segment_softmax + weighted_segment_aggregate%s, fwd + bwd"
                % (" over materialised kk / vv" if with_edge else ""), t["composite"])
    t_ms = show("plain torch, fwd + bwd", t["torch"])
    rows = 3 + (1 if with_edge else 0)  # forward: k, v (and edge) rows; backward: v and k again (and edge), grad_edge
    nbytes = n * DIM * 4 * (2 * rows - 1)
    print("  composite / fused: %.2f   plain torch / fused: %.2f   (fused moves at least %.2f GB of [n, D] rows -> "
          "%.1f GB/s)" % (c_ms / f_ms, t_ms / f_ms, nbytes / 1e9, nbytes / max(f_ms, 1e-6) / 1e6), flush=True)
    a, b = fused(), fused()
    print("  fused repeats out and every gradient bit for bit: %s"
          % all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(a, b)), flush=True)
    if t["composite"] is not None:
        want = composite()
        print("  largest |fused - composite|: " + "  ".join("%.3e" % float((x - y).abs().max()) for x, y in zip(a, want)),
              flush=True)
    # the longest segment alone: the same call on one segment is what its lane group spends on it
    top = int(counts.argmax())
    lo = int(counts[:top].long().sum())
    hi = lo + int(counts[top])
    one = counts[top:top + 1].contiguous()
    sub_e = None if edge0 is None else edge0[lo:hi].contiguous()

    def longest():
        q = tabs[0][local0[top:top + 1]].requires_grad_(True)
        e = None if sub_e is None else sub_e.detach().requires_grad_(True)
        out = dot_attention(q, tabs[1], tabs[2], local[lo:hi].contiguous(), 1, counts=one, edge=e, heads=HEADS)
        out.backward(g[top:top + 1])

    l_ms = show("the two per-segment kernels on the longest segment alone (%d positions; no row gradients)" % (hi - lo),
                timed({"longest": longest})["longest"])
    print("  longest segment's share of the fused time: at most %.3f" % (l_ms / f_ms), flush=True)
    return f_ms, c_ms, t_ms


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
    for with_edge in (False, True):
        ms = compare("dense (C3 hop 2, EdgeWeight %s, %d seeds) as segments of %d" % (FANOUTS, B, f), M, local0, local,
                     counts, with_edge, gen, dev)
        summary.append(("dense", with_edge) + ms)
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
    print("ragged hop: %d positions in %d segments over %d distinct nodes; longest %d, median %d"
          % (int(nbr.numel()), int(deg.numel()), int(nodes.numel()), int(deg.max()), int(deg.median())), flush=True)
    M = int(nodes.numel())
    del graph, nbr, nodes
    torch.cuda.empty_cache()
    for with_edge in (False, True):
        ms = compare("ragged FullSampler hop", M, local0, local, deg, with_edge, gen, dev)
        summary.append(("ragged", with_edge) + ms)

    print("\nsummary (medians, ms): stream edge fused composite torch composite/fused torch/fused")
    for stream, with_edge, f_ms, c_ms, t_ms in summary:
        print("  %-6s %-5s %9.3f %9.3f %9.3f %6.2f %6.2f" % (stream, with_edge, f_ms, c_ms, t_ms, c_ms / f_ms, t_ms / f_ms))


if __name__ == "__main__":
    main()
