"""Frontier dedup on the id stream of a real C3 step (RMAT 10 M / 100 M, EdgeWeight [25, 10], 65,536 seeds):

  1. glx.unique(seeds, hop 1, hop 2) against torch.unique(torch.cat(parts), return_inverse=True) on the same tensors
     (the sort-based call does less: ascending order, no per-part counts);
  2. distinct / total ids per frontier and the bytes x_nodes writes against x[h] at dim 256;
  3. NeighborLoader time per batch with dedup off and on, features at dim 256.

One process, HIP events, 3 warm-up + 20 timed repetitions, legs interleaved.
Usage: python scripts/r09/unique_probe.py [nodes] [edges] [batch] [dedup-only] > profiles/r09/frontier_unique.txt
(dedup-only: stop after section 1 -- the target of a `rocprofv3 --kernel-trace --stats` run of its own)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402

WARMUP, REPS = 3, 20
FANOUTS = [25, 10]


def timed(legs):
    """legs: {name: callable}.  Interleaved; -> {name: sorted list of REPS times in ms}."""
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


def show(name, ts, n):
    med = ts[len(ts) // 2]
    print("  %-44s median %8.3f ms  min %8.3f  max %8.3f   %6.2f ns/id  %6.1f M ids/s"
          % (name, med, ts[0], ts[-1], med * 1e6 / n, n / med / 1e3), flush=True)
    return med


class _Sampler(object):
    def __init__(self, g, fanouts):
        self.g, self.fanouts = g, fanouts

    def get_device(self, seeds, seed=None, call_counter=0):
        return glx.sample_hops([self.g] * len(self.fanouts), "EdgeWeightSampler", seeds, self.fanouts, seed=42,
                               call_counter=call_counter)


class _Graph(object):
    """What NeighborLoader asks of a gl.Graph, over glx handles built from the edge list (a 100 M-edge TSV load is not
    what this probe measures)."""

    def __init__(self, g, feats):
        self.g, self.feats = g, feats

    def neighbor_sampler(self, meta_path, fanouts, strategy="random"):
        return _Sampler(self.g, list(fanouts))

    def get_topology(self):
        return self

    def get_dst_type(self, edge_type):
        return "v"

    def device_features(self, node_type):
        return self.feats


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    D = 256
    dev = torch.device("cuda", 0)
    print("device: %s   graph: RMAT %d vertices / %d edges   EdgeWeight %s   %d seeds   dim %d"
          % (torch.cuda.get_device_name(0), V, E, FANOUTS, B, D), flush=True)
    src, dst, w = synth.rmat_edges_torch(V, E, 1, dev, weighted=True)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, w)
    del src, dst, w
    feats = glx.Features(synth.features_torch(V, D, 2, dev))
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    hops = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, FANOUTS, seed=42, call_counter=0)
    parts = [seeds, hops[0][0], hops[1][0]]
    lens = [int(p.numel()) for p in parts]
    n = sum(lens)

    # ---- 1. the dedup itself
    print("\n[1] dedup of one step's id stream: n = %d ids in parts %s" % (n, lens), flush=True)
    t = timed({
        "glx.unique": lambda: glx.unique(parts),
        "torch.unique(cat, return_inverse=True)": lambda: torch.unique(torch.cat([p.reshape(-1) for p in parts]),
                                                                       return_inverse=True),
        "glx.unique(return_inverse=False)": lambda: glx.unique(parts, return_inverse=False),
        "torch.unique(cat)": lambda: torch.unique(torch.cat([p.reshape(-1) for p in parts])),
    })
    med = {k: show(k, v, n) for k, v in t.items()}
    print("  glx.unique / torch.unique (both with inverse): %.3f   (without: %.3f)"
          % (med["glx.unique"] / med["torch.unique(cat, return_inverse=True)"],
             med["glx.unique(return_inverse=False)"] / med["torch.unique(cat)"]), flush=True)
    nodes, local, part_end = glx.unique(parts)
    u, inv = torch.unique(torch.cat([p.reshape(-1) for p in parts]), return_inverse=True)
    same_set = bool(torch.equal(torch.sort(nodes).values, u))
    same_map = bool(torch.equal(nodes[torch.cat([v.reshape(-1) for v in local])], u[inv]))
    print("  same distinct set as torch.unique: %s   same id behind every slot: %s" % (same_set, same_map), flush=True)

    if len(sys.argv) > 4 and sys.argv[4] == "dedup-only":
        return

    # ---- 2. what repeats
    ends = part_end.cpu().numpy()
    m = int(ends[-1])
    print("\n[2] distinct / total ids (cumulative node set after each frontier)")
    prev = 0
    for h, k in enumerate(lens):
        print("  frontier %d: %9d slots, %8d new distinct ids, node set %8d" % (h, k, ends[h] - prev, ends[h]))
        prev = ends[h]
    row = D * 4
    print("  distinct / total = %d / %d = %.4f" % (m, n, m / n))
    print("  feature bytes per batch at dim %d: x_nodes %.3f GB, x[0..2] %.3f GB  (%.1f x less written)"
          % (D, m * row / 1e9, n * row / 1e9, n / m), flush=True)
    del nodes, local, part_end, u, inv
    torch.cuda.empty_cache()

    # ---- 3. the loader, dedup off / on
    import graphlearn as gl
    shim = _Graph(g, feats)
    ids = pool.cpu().numpy()

    def batches(**kw):  # epoch after epoch: a small [nodes] [batch] has fewer batches per epoch than repetitions
        loader = gl.NeighborLoader(shim, "v", ["e", "e"], FANOUTS, batch_size=B, strategy="edge_weight", seed_ids=ids, **kw)
        while True:
            for batch in loader:
                yield batch

    off, on = batches(), batches(dedup=True)
    print("\n[3] NeighborLoader, ms per batch (sample 2 hops + features of the batch at dim %d)" % D, flush=True)
    t = timed({"dedup=False (x[h]: one row per slot)": lambda: next(off),
               "dedup=True  (x_nodes: one row per node)": lambda: next(on)})
    for k, v in t.items():
        show(k, v, n)


if __name__ == "__main__":
    main()
