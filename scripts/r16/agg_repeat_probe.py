"""Max / Min reduce without the loads of rows a segment has already folded (glx_aggregate.hip agg_first_occurrences):
same-process A/B of glx_tune("agg_repeats", 1 = every position loaded | 2 = first occurrences only | 0 = the default,
which skips where segments average 16 positions or more), alternated six times, on five requests over the C3 store --
the live hop-1 and hop-2 requests of the samplers, the hop-2 request of degree-biased seeds, ids uniform over the table
(no repeats: what the masks cost), and a C5-shaped Sum request over a 1 GiB table (must not see the knob).  Outputs
must be bit-equal under both settings.  Prints the distinct rows per segment of the live requests, computed from the
ids.  One process, one GPU, nothing read but the tree.

  python scripts/r16/agg_repeat_probe.py [OUT.txt]     (default: profiles/r16/agg_repeat_ab.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import glx  # noqa: E402
import synth  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16", "agg_repeat_ab.txt")
dev = torch.device("cuda", 0)
SMP, GS = "EdgeWeightSampler", 4
V, E, D, B0, k1, k2 = 10_000_000, 100_000_000, 256, 65536, 25, 10
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=True)
uniq, biased = torch.unique(src), src.clone()
g = glx.Graph.from_edges(src, dst, w)
del src, dst, w
f = glx.Features(synth.features_torch(V, D, GS + 1, dev))
gen = torch.Generator(device=dev)
gen.manual_seed(1000)


def two_hops(pool):
    seeds = pool[torch.randint(0, pool.shape[0], (B0,), generator=gen, device=dev)]
    n1, _ = g.sample(SMP, seeds, k1, seed=42, call_counter=0)
    n2, _ = g.sample(SMP, n1.view(-1), k2, seed=42, call_counter=1)
    torch.cuda.synchronize()
    return n1, n2


def distinct(n):
    """(mean distinct ids per row, share of positions that repeat an earlier id of their row)"""
    s = torch.sort(n, dim=1).values
    d = (s[:, 1:] != s[:, :-1]).sum(dim=1) + 1
    return float(d.double().mean()), 1.0 - float(d.sum()) / n.numel(), float((d == 1).double().mean())


n1, n2 = two_hops(uniq)
_, n2deg = two_hops(biased)
del uniq, biased
for name, n in (("hop 1", n1), ("hop 2", n2), ("hop 2, degree-biased seeds", n2deg)):
    d, rep, one = distinct(n)
    say("# %s: fanout %d, %.2f distinct rows per segment, %.1f %% of the positions repeat a row of their segment, "
        "%.1f %% of the segments hold one row" % (name, n.shape[1], d, 100 * rep, 100 * one))
# C5's item -> shop shape: 6.55 M ids over a 1 GiB float32 table (three segments per wave), Sum
Vs = (1 << 30) // (4 * D)
fs = glx.Features(synth.features_torch(Vs, D, GS + 2, dev))
Sg2 = B0 * k1
reqs = {  # name: (features, aggregator, ids, segments)
    "hop1": (f, "MaxAggregator", n1.reshape(-1).contiguous(), B0),
    "hop2": (f, "MaxAggregator", n2.reshape(-1).contiguous(), Sg2),
    "hop2_degree": (f, "MaxAggregator", n2deg.reshape(-1).contiguous(), Sg2),
    "uniform": (f, "MaxAggregator", torch.randint(0, V, (Sg2 * k2,), generator=gen, device=dev), Sg2),
    "c5_sum": (fs, "SumAggregator", torch.randint(0, Vs, (655360 * 10,), generator=gen, device=dev), 655360),
}
emb = torch.empty((Sg2, D), dtype=torch.float32, device=dev)
cnt = torch.empty(Sg2, dtype=torch.int32, device=dev)


def run(name):
    ft, agg, ids, sg = reqs[name]
    out = (emb[:sg], cnt[:sg])
    ft.aggregate(agg, ids, None, sg, out=out)
    return out


def timed(name, reps=3):
    r = []
    for _ in range(reps):
        torch.cuda.synchronize()
        glx.profile_enable(True)
        run(name)
        torch.cuda.synchronize()
        glx.profile_enable(False)
        r.append(float(glx.profile_collect(glx.KERNEL_AGGREGATE).sum()))
    return float(np.median(r))


try:
    for name in reqs:
        glx.tune("agg_repeats", 1)
        o = run(name)
        torch.cuda.synchronize()
        every = (o[0].clone(), o[1].clone())
        for mode in (2, 0):
            glx.tune("agg_repeats", mode)
            o = run(name)
            torch.cuda.synchronize()
            assert torch.equal(o[0].view(torch.int32), every[0].view(torch.int32)) and torch.equal(o[1], every[1]), (name, mode)
        del every
    cfgs = [(name, k) for name in reqs for k in (1, 2, 0)]
    res = {c: [] for c in cfgs}
    for rnd in range(6):
        for c in (cfgs if rnd % 2 == 0 else cfgs[::-1]):
            glx.tune("agg_repeats", c[1])
            res[c].append(timed(c[0]))
finally:
    glx.tune("agg_repeats", 0)
say("# C3 store (RMAT 10 M / 100 M, D = 256 float32), %s [%d, %d]; outputs bit-equal under all three settings" % (SMP, k1, k2))
say("# request  agg_repeats  median ms over 6 alternations (min .. max)")
for c in cfgs:
    r = res[c]
    say("%-12s %d  %.4f  (%.4f .. %.4f)" % (c[0], c[1], np.median(r), min(r), max(r)))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
