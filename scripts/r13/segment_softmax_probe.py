"""Two first measurements for the ragged segment softmax (glx_segment_softmax, graphlearn.nn.pytorch.segment_softmax).

  (a) E, the error of the platform's float32 exp in ulp, which the tolerance of the forward contract needs and which
      must not come from the kernel under test: float32 torch.exp on the device against float64 numpy.exp of the same
      float32 arguments -- 2^22 of them spread over [-104, 0], plus the float32 neighbours of 0 and of -87.33 (where
      the result leaves the normal range).  Results of at least 2^-126 are measured in ulp of the exact value; below
      that the absolute error is given in units of 2^-126, the term the contract keeps for underflow.
      tests/segment_softmax_ref.py uses E = ceil(the maximum) + 1, and at least 2.
  (b) forward + backward of segment_softmax against a torch composite with its own autograd -- scatter_reduce(amax),
      gather, exp, index_add_, gather, divide -- at heads 1 and 4, on
        dense    the hop-2 stream of a C3 step (EdgeWeight [25, 10], 65,536 seeds: 16.4 M positions) as 1.64 M
                 segments of 10, with the implied layout and with explicit counts of 10;
        ragged   a FullSampler hop over 65,536 seeds of the RMAT 10 M / 100 M graph, hubs included,
      and the longest segment of the ragged request on its own, as a share of the whole request's time.

One process, HIP events, 3 warm-up + 10 timed repetitions, legs interleaved.  Nothing here is a requirement of the test
suite, and no ratio is promised.
Usage: python scripts/r13/segment_softmax_probe.py [nodes] [edges] [batch] > profiles/r13/segment_softmax.txt"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from graphlearn.nn.pytorch import segment_softmax  # noqa: E402

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]


def neighbours(c, steps=8):
    """the float32 values within `steps` of c, on both sides"""
    out, lo, hi = [np.float32(c)], np.float32(c), np.float32(c)
    for _ in range(steps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.array(out, np.float32)


def measure_exp():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-104.0, 0.0, 2 ** 22).astype(np.float32),
                        np.linspace(-104.0, 0.0, 2 ** 16, dtype=np.float32),
                        neighbours(0.0), neighbours(-87.33)])
    x = x[x <= 0]
    got = torch.exp(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
    exact = np.exp(x.astype(np.float64))
    normal = exact >= 2.0 ** -126
    ulp = 2.0 ** (np.floor(np.log2(exact[normal])) - 23)
    err = np.abs(got[normal] - exact[normal]) / ulp
    worst = int(np.argmax(err))
    print("(a) float32 torch.exp on the device against float64 numpy.exp, %d arguments in [-104, 0]" % len(x))
    print("    results >= 2^-126 (%d): maximum error %.4f ulp at x = %r; mean %.4f ulp; exp(0) == 1: %s"
          % (int(normal.sum()), float(err.max()), float(x[normal][worst]), float(err.mean()),
             bool(got[x == 0].min() == 1.0 and got[x == 0].max() == 1.0)))
    under = np.abs(got[~normal] - exact[~normal]) / 2.0 ** -126
    print("    results <  2^-126 (%d): maximum absolute error %.4f x 2^-126; flushed to zero: %d of them"
          % (int((~normal).sum()), float(under.max()), int((got[~normal] == 0).sum())))
    print("    E for tests/segment_softmax_ref.py: max(ceil(%.4f) + 1, 2) = %d"
          % (float(err.max()), max(int(math.ceil(float(err.max()))) + 1, 2)), flush=True)


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
    print("  %-66s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]), flush=True)
    return med


def composite(e, seg, S):
    """softmax over segments in plain torch: seg[n] int64 is the segment of each position"""
    H = e.shape[1]
    idx = seg[:, None].expand(-1, H)
    m = torch.full((S, H), -math.inf, device=e.device).scatter_reduce(0, idx, e.detach(), "amax")
    t = torch.exp(e - m[seg])
    z = torch.zeros((S, H), device=e.device).index_add_(0, seg, t)
    return t / z[seg]


def compare(title, n, S, counts, heads, gen, dev):
    e = torch.randn(n, heads, device=dev, generator=gen) * 3
    g = torch.randn(n, heads, device=dev, generator=gen)
    if counts is None:
        seg = torch.arange(n, device=dev) // (n // S)
    else:
        seg = torch.repeat_interleave(torch.arange(S, device=dev), counts.long(), output_size=n)

    def engine():
        er = e.detach().requires_grad_(True)
        out = segment_softmax(er, S, counts=counts)
        out.backward(g)
        return out.detach(), er.grad

    def plain():
        er = e.detach().requires_grad_(True)
        out = composite(er, seg, S)
        out.backward(g)
        return out.detach(), er.grad

    print("\n[b] %s, heads = %d: %d positions in %d segments" % (title, heads, n, S), flush=True)
    t = timed({"engine": engine, "torch": plain})
    e_ms = show("segment_softmax fwd + bwd", t["engine"])
    t_ms = show("scatter_reduce / gather / exp / index_add_ / gather / divide fwd + bwd", t["torch"])
    nbytes = n * heads * 4 * 5  # e in, alpha out; alpha and grad_alpha in, grad_e out
    print("  torch composite / segment_softmax: %.2f   (at least %.2f GB by the shapes -> %.1f GB/s)"
          % (t_ms / e_ms, nbytes / 1e9, nbytes / max(e_ms, 1e-6) / 1e6), flush=True)
    for name, fn in (("engine", engine), ("torch", plain)):
        a, b = fn(), fn()
        same = [bool(torch.equal(p.view(torch.int32), q.view(torch.int32))) for p, q in zip(a, b)]
        print("  %-6s repeats its own alpha / e.grad bit for bit: %s / %s" % (name, same[0], same[1]), flush=True)
    got, want = engine(), plain()
    print("  largest |engine - torch|: alpha %.3e   e.grad %.3e"
          % tuple(float((p - q).abs().max()) for p, q in zip(got, want)), flush=True)
    return e, g, e_ms


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    dev = torch.device("cuda", 0)
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    measure_exp()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    f = FANOUTS[1]
    n = B * FANOUTS[0] * f
    S = n // f
    for heads in (1, 4):
        compare("dense, implied layout (C3 hop 2, EdgeWeight %s, %d seeds)" % (FANOUTS, B), n, S, None, heads, gen, dev)
        counts = torch.full((S,), f, dtype=torch.int32, device=dev)
        compare("dense, explicit counts of %d" % f, n, S, counts, heads, gen, dev)
        del counts
        torch.cuda.empty_cache()

    print("\ngraph: RMAT %d vertices / %d edges, FullSampler over %d seeds" % (V, E, B), flush=True)
    src, dst, _ = synth.rmat_edges_torch(V, E, 1, dev, weighted=False)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, sort_by_weight=False)
    del src, dst
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    deg, nbr, _ = g.sample_full(seeds, 0)
    n, S = int(nbr.numel()), int(deg.numel())
    longest = int(deg.max())
    print("ragged hop: %d positions in %d segments; longest %d, median %d, %d segments above 1024 positions"
          % (n, S, longest, int(deg.median()), int((deg > 1024).sum())), flush=True)
    del g, nbr
    torch.cuda.empty_cache()
    first = int(deg.long().cumsum(0)[int(deg.argmax())]) - longest
    one = torch.tensor([longest], dtype=torch.int32, device=dev)
    for heads in (1, 4):
        e, grad, whole_ms = compare("ragged FullSampler hop", n, S, deg, heads, gen, dev)
        el, gl_ = e[first:first + longest].contiguous(), grad[first:first + longest].contiguous()

        def alone():
            er = el.detach().requires_grad_(True)
            segment_softmax(er, 1, counts=one).backward(gl_)

        ms = show("the longest segment (%d positions) as a request of its own" % longest, timed({"a": alone})["a"])
        print("  its share of the whole request's time: %.1f %% (an upper bound: a launch of its own is in it)"
              % (100.0 * ms / whole_ms), flush=True)


if __name__ == "__main__":
    main()
