"""A first measurement of temporal neighbour sampling (glx_sample_temporal, glx.Graph.sample_temporal): "the neighbours
of v over edges before t" with a cutoff per request row, against the composite available without it -- sample_full of
every request row, a timestamp lookup by edge id, a torch mask `ts < cutoff` and a per-segment top-k of the k latest (or
k uniform picks among the masked) -- on the same machine in the same run.

  graph    RMAT (a, b, c, d = 0.57, 0.19, 0.19, 0.05), 2^17 vertices, 4 M timestamped edges: hubs included
  events   200 .. 65,536 request rows: the source and the time of random edges (so hubs are asked for often)
  k        10 and 20; RECENT and UNIFORM

Reported: the longest row's share of the edges, the W-ary search's rounds (loop rounds + the last one) for the longest
row and averaged over the request, both legs' medians, and whether the RECENT answers are equal.  The composite is
skipped where its response would pass 2^29 slots.

One process, HIP events, 2 warm-up + 10 timed repetitions, legs interleaved, medians.  Nothing here is a requirement of
the test suite, and no ratio is promised.
Usage: python scripts/r22/temporal_probe.py [edges] > profiles/r22/temporal.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

WARMUP, REPS = 2, 10
SCALE = 17
SLOT_CAP = 1 << 29


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
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def rmat(edges, gen):
    src = torch.zeros(edges, dtype=torch.int64, device="cuda")
    dst = torch.zeros(edges, dtype=torch.int64, device="cuda")
    for _ in range(SCALE):
        u = torch.rand(edges, device="cuda", generator=gen)
        src = src * 2 + (u >= 0.76).long()                                  # c + d
        dst = dst * 2 + (((u >= 0.57) & (u < 0.76)) | (u >= 0.95)).long()   # b, d
    return src, dst


def rounds(deg, W):
    """rounds of the W-ary search of a row of `deg` slots: the loop's (the widest interval a round can leave) + the last"""
    n, r = int(deg), 0
    while n > W:
        # m probes lie before the cutoff: the interval runs from past probe m - 1 (or its start) to probe m (or its end)
        lo = [(m * n) // (W + 1) + 1 if m else 0 for m in range(W + 1)]
        hi = [((m + 1) * n) // (W + 1) if m < W else n for m in range(W + 1)]
        n = max(h - l for l, h in zip(lo, hi))
        r += 1
    return r + 1


def composite(g, ts_by_eid, src, cutoff, k, uniform, gen):
    deg, nbr, eid = g.sample_full(src)
    ts = ts_by_eid[eid]
    off = torch.zeros(src.shape[0] + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(deg.long(), 0)
    seg = torch.repeat_interleave(torch.arange(src.shape[0], device="cuda"), deg.long())
    before = torch.zeros(ts.shape[0] + 1, dtype=torch.int64, device="cuda")
    before[1:] = torch.cumsum((ts < cutoff[seg]).long(), 0)
    c = before[off[1:]] - before[off[:-1]]  # rows are timestamp-ascending: the masked slots are the first c
    j = torch.arange(k, device="cuda")[None, :]
    if uniform:
        pick = (torch.rand((src.shape[0], k), device="cuda", generator=gen) * c[:, None]).long()
        valid = (c > 0)[:, None].expand(-1, k)
    else:
        pick = c[:, None] - 1 - j
        valid = j < c[:, None]
    at = (off[:-1, None] + pick).clamp_(0, max(int(ts.shape[0]) - 1, 0))
    return (torch.where(valid, nbr[at], 0), torch.where(valid, eid[at], -1), torch.where(valid, ts[at], -1))


def main():
    edges = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    src, dst = rmat(edges, gen)
    t = torch.randint(0, 1_000_000, (edges,), device="cuda", generator=gen)
    g = glx.Graph.from_edges(src, dst, timestamp=t)
    assert g.has_timestamps
    degs = torch.bincount(src)
    longest = int(degs.max())
    print("temporal probe: RMAT 2^%d vertices, %d edges, %d rows, medians of %d, device %s"
          % (SCALE, edges, g.num_rows, REPS, torch.cuda.get_device_name(0)))
    print("longest row: %d slots = %.2f%% of the edges; search rounds for it: %s (a binary search: %d)"
          % (longest, 100.0 * longest / edges, ", ".join("W=%d: %d" % (W, rounds(longest, W)) for W in (8, 16, 32, 64)),
             longest.bit_length()))
    print("%6s %3s %8s | %9s %8s | %10s %8s | %7s %5s" % ("rows", "k", "strategy", "glx ms", "rounds", "composite", "slots",
                                                          "ratio", "equal"))
    for rows in (200, 1024, 4096, 16384, 65536):
        ev = torch.randint(0, edges, (rows,), device="cuda", generator=gen)
        q, cut = src[ev].contiguous(), t[ev].contiguous()
        qdeg = degs[q]
        slots = int(qdeg.sum())
        for k in (10, 20):
            W = 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64
            by_deg = {int(d): rounds(int(d), W) for d in torch.unique(qdeg).tolist()}
            mean_rounds = sum(by_deg[int(d)] for d in qdeg.tolist()) / rows
            for name in ("recent", "uniform"):
                legs = {"glx": lambda: g.sample_temporal(q, cut, k, strategy=name, seed=1, call_counter=2)}
                if slots <= SLOT_CAP:
                    legs["composite"] = lambda: composite(g, t, q, cut, k, name == "uniform", gen)
                tm = timed(legs)
                equal = "-"
                if "composite" in legs and name == "recent":
                    a = g.sample_temporal(q, cut, k, strategy=name)
                    b = composite(g, t, q, cut, k, False, gen)
                    equal = "yes" if all(torch.equal(x, y) for x, y in zip(a[:3], b)) else "NO"
                comp = "%10.3f" % tm["composite"] if "composite" in tm else "   skipped"
                ratio = "%7.1f" % (tm["composite"] / tm["glx"]) if "composite" in tm else "      -"
                print("%6d %3d %8s | %9.4f %8.2f | %s %8d | %s %5s" % (rows, k, name, tm["glx"], mean_rounds, comp, slots,
                                                                     ratio, equal))
                sys.stdout.flush()


if __name__ == "__main__":
    main()
