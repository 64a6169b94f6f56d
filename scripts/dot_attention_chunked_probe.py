"""The chunked order of the fused dot-product attention (dot_attention(chunked=True): glx_dot_attention_chunked,
glx_dot_attention_backward_chunked) measured beside the default order and the composite of the ops that existed before
it, forward + backward, on the two workloads of scripts/r19/dot_attention_probe.py:

  dense    the deduplicated hop-2 stream of a C3 step (EdgeWeight [25, 10], 65,536 seeds: 16.4 M positions) as 1.64 M
           segments of 10: no long segment, no long row -- what the directory pass and the idle launches cost;
  ragged   a FullSampler hop over 65,536 seeds of the RMAT 10 M / 100 M graph, hubs included, relabelled by glx.unique:
           what splitting the hub segments (and the hub rows of grad_k / grad_v) buys,

at dim 256, heads 4, each with and without the edge term.

  default    q = gather_rows(q_nodes, seed_local); dot_attention(q, k, v, local, S, counts, edge, heads)
  chunked    the same call with chunked=True
  composite  pair_dot * scale, segment_softmax, weighted_segment_aggregate (over materialised kk / vv with an edge term)

One process, HIP events around the whole call, 3 warm-up + 10 timed repetitions, the three legs interleaved, medians.
On the dense workload the chunked median is set against the default's own min .. max.  Nothing here is a requirement of
the test suite, and no ratio is promised.
Usage: python scripts/dot_attention_chunked_probe.py [out.txt] [nodes] [edges] [batch]
       (out.txt defaults to profiles/dot_attention_chunked/probe.txt)"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
OUT = None


def say(text=""):
    print(text, flush=True)
    OUT.write(text + "\n")
    OUT.flush()


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
        say("  %-78s does not fit the device's memory" % name)
        return float("nan")
    med = ts[len(ts) // 2]
    say("  %-78s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]))
    return med


def compare(title, M, local0, local, counts, with_edge, gen, dev):
    n, S = int(local.numel()), int(local0.numel())
    scale = 1.0 / math.sqrt(DIM // HEADS)
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

    def fused(chunked):
        ls = leaves()
        qa, k, v, e = ls
        return grads(dot_attention(gather_rows(qa, local0), k, v, local, S, counts=counts, edge=e, heads=HEADS,
                                   chunked=chunked), ls)

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

    say("\n%s, %s: %d positions in %d segments, %d rows of %d columns in %d heads"
        % (title, "with an edge term" if with_edge else "no edge term", n, S, M, DIM, HEADS))
    say("  segments of more than 256 positions: %d (longest %d); rows named more than 256 times: %d"
        % (int((counts > 256).sum()), int(counts.max()), int((torch.bincount(local, minlength=M) > 256).sum())))
    t = timed({"default": lambda: fused(False), "chunked": lambda: fused(True), "composite": composite})
    d_ms = show("default: gather_rows [S, D] + dot_attention, fwd + bwd", t["default"])
    c_ms = show("chunked: gather_rows [S, D] + dot_attention(chunked=True), fwd + bwd", t["chunked"])
    o_ms = show("composite: pair_dot + segment_softmax + weighted_segment_aggregate%s, fwd + bwd"
                % (" over materialised kk / vv" if with_edge else ""), t["composite"])
    say("  default / chunked: %.2f   composite / chunked: %.2f   composite / default: %.2f"
        % (d_ms / c_ms, o_ms / c_ms, o_ms / d_ms))
    if t["default"] is not None and t["chunked"] is not None:
        lo, hi = t["default"][0], t["default"][-1]
        say("  chunked median against the default median: %+.2f %%; the default's own repeats span %+.2f %% .. %+.2f %%"
            " of its median: the chunked median lies %s that span"
            % (100.0 * (c_ms / d_ms - 1.0), 100.0 * (lo / d_ms - 1.0), 100.0 * (hi / d_ms - 1.0),
               "inside" if lo <= c_ms <= hi else "outside"))
    a, b, d = fused(True), fused(True), fused(False)
    say("  chunked repeats out and every gradient bit for bit: %s"
        % all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(a, b)))
    say("  chunked has the default's bits in: " + "  ".join(
        "%s %s" % (name, bool(torch.equal(x.view(torch.int32), y.view(torch.int32))))
        for name, x, y in zip(("out", "grad_q_nodes", "grad_k", "grad_v", "grad_edge"), a, d)))
    say("  largest |chunked - default|: " + "  ".join("%.3e" % float((x - y).abs().max()) for x, y in zip(a, d)))
    return d_ms, c_ms, o_ms


def main():
    global OUT
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dot_attention_chunked", "probe.txt")
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    E = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000_000
    B = int(sys.argv[4]) if len(sys.argv) > 4 else 65536
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    OUT = open(path, "w")
    dev = torch.device("cuda", 0)
    say("device: %s" % torch.cuda.get_device_name(0))
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

    say("\ngraph: RMAT %d vertices / %d edges, FullSampler over %d seeds" % (V, E, B))
    src, dst, _ = synth.rmat_edges_torch(V, E, 1, dev, weighted=False)
    pool = torch.unique(src)
    graph = glx.Graph.from_edges(src, dst, sort_by_weight=False)
    del src, dst
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    deg, nbr, _ = graph.sample_full(seeds, 0)
    nodes, (local0, local), _ = glx.unique([seeds, nbr])
    say("ragged hop: %d positions in %d segments over %d distinct nodes; longest %d, median %d"
        % (int(nbr.numel()), int(deg.numel()), int(nodes.numel()), int(deg.max()), int(deg.median())))
    M = int(nodes.numel())
    del graph, nbr, nodes
    torch.cuda.empty_cache()
    for with_edge in (False, True):
        ms = compare("ragged FullSampler hop", M, local0, local, deg, with_edge, gen, dev)
        summary.append(("ragged", with_edge) + ms)

    say("\nsummary (medians, ms): stream edge default chunked composite default/chunked composite/chunked")
    for stream, with_edge, d_ms, c_ms, o_ms in summary:
        say("  %-6s %-5s %9.3f %9.3f %9.3f %6.2f %6.2f"
            % (stream, with_edge, d_ms, c_ms, o_ms, d_ms / c_ms, o_ms / c_ms))
    OUT.close()


if __name__ == "__main__":
    main()
