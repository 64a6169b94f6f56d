"""Half-precision feature tables on the headline C3 shape (RMAT 10 M / 100 M, EdgeWeight [25, 10], Max, D = 256,
batch 65536): float32 vs bfloat16 tables over the same ids, alternated in one process after warm-up, timed with
device events.  `ab`: the hop-2 reduce, the hop-1 reduce and the whole sample + aggregate step, each with the float32
and the bfloat16 table (plus the bfloat16 hop-2 reduce with the slice / load-width knobs: agg_xcd_slices, agg_half_ld16); the bfloat16 outputs are
checked bit for bit against the float32 table of the upcast values first.  `pmc`: a fixed launch sequence for a counter
pass (the hop-2 reduce: float32, bfloat16, three times each)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
import numpy as np, torch, glx, synth
mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
dev = torch.device("cuda", 0)
SMP, AGG, GS = "EdgeWeightSampler", "MaxAggregator", 4
V, E, D, B0, k1, k2 = 10_000_000, 100_000_000, 256, 65536, 25, 10
src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=True)
pool = torch.unique(src)
g = glx.Graph.from_edges(src, dst, w); del src, dst, w
X = synth.features_torch(V, D, GS + 1, dev)
tabs = {"f32": glx.Features(X), "bf16": glx.Features(X, dtype="bfloat16")}
if mode == "ab":
    up = glx.Features(X.to(torch.bfloat16).float())  # the float32 table of the upcast values (correctness only)
del X
torch.cuda.empty_cache()
gen = torch.Generator(device=dev); gen.manual_seed(1000)
Sg = B0 * k1
emb = torch.empty((Sg, D), dtype=torch.float32, device=dev); cnt = torch.empty(Sg, dtype=torch.int32, device=dev)
emb1 = torch.empty((B0, D), dtype=torch.float32, device=dev); cnt1 = torch.empty(B0, dtype=torch.int32, device=dev)
seeds = pool[torch.randint(0, pool.shape[0], (B0,), generator=gen, device=dev)]
n1, _ = g.sample(SMP, seeds, k1, seed=42, call_counter=0)
n2, _ = g.sample(SMP, n1.view(-1), k2, seed=42, call_counter=1)
torch.cuda.synchronize()
KN = {"agg_xcd_slices": 0, "agg_half_ld16": 0}


def setk(**kw):
    for k, v in KN.items():
        glx.tune(k, kw.get(k, v))


def hop2(f):
    return f.aggregate(AGG, n2.view(-1), None, Sg, out=(emb, cnt))


def hop1(f):
    return f.aggregate(AGG, n1.view(-1), None, B0, out=(emb1, cnt1))


def step(f):  # what bench.py's step does on one GPU: two sampled hops, then the two reduces (deepest first)
    a, _ = g.sample(SMP, seeds, k1, seed=42, call_counter=2)
    b, _ = g.sample(SMP, a.view(-1), k2, seed=42, call_counter=3)
    f.aggregate(AGG, b.view(-1), None, Sg, out=(emb, cnt))
    f.aggregate(AGG, a.view(-1), None, B0, out=(emb1, cnt1))


def timed(fn, f, reps=5):
    r = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record(); fn(f); e.record()
        e.synchronize()
        r.append(s.elapsed_time(e))
    return float(np.median(r))


if mode == "pmc":
    for rep in range(3):
        setk(); hop2(tabs["f32"]); hop2(tabs["bf16"])
    torch.cuda.synchronize()
    print("launch order: (float32 hop-2 reduce, bfloat16 hop-2 reduce) x 3 -- after the setup's sampling launches")
    sys.exit(0)

# correctness first: bfloat16 table == float32 table of the upcast values, bit for bit, for every configuration timed
for fn in (hop2, hop1):
    for kn in (dict(), dict(agg_xcd_slices=2), dict(agg_half_ld16=1)):
        setk()
        e, c = fn(up); e, c = e.clone(), c.clone()
        setk(**kn)
        eb, cb = fn(tabs["bf16"])
        torch.cuda.synchronize()
        assert torch.equal(e.view(torch.int32), eb.view(torch.int32)) and torch.equal(c, cb), (fn.__name__, kn)
del up, e, c
torch.cuda.empty_cache()
cfgs = [("hop2", "f32", {}), ("hop2", "bf16", {}), ("hop2", "bf16", dict(agg_xcd_slices=2)),
        ("hop2", "bf16", dict(agg_half_ld16=1)), ("hop2", "bf16", dict(agg_half_ld16=1, agg_xcd_slices=1)),
        ("hop1", "f32", {}), ("hop1", "bf16", {}), ("step", "f32", {}), ("step", "bf16", {})]
FN = {"hop2": hop2, "hop1": hop1, "step": step}
for c in cfgs:  # warm-up
    setk(**c[2]); FN[c[0]](tabs[c[1]])
torch.cuda.synchronize()
res = {i: [] for i in range(len(cfgs))}
for rnd in range(6):
    order = range(len(cfgs)) if rnd % 2 == 0 else reversed(range(len(cfgs)))
    for i in order:
        c = cfgs[i]
        setk(**c[2]); res[i].append(timed(FN[c[0]], tabs[c[1]]))
setk()
print("# c3: %s [%d,%d] %s D=%d batch %d; device-event ms, median of 5 per alternation, 6 alternations" % (SMP, k1, k2, AGG, D, B0))
print("# bfloat16 outputs verified bit-identical to the float32 table of the upcast values (every knob below)")
print("# what     table  knobs                                median  (min .. max of the 6 medians)")
for i, c in enumerate(cfgs):
    r = res[i]
    kn = ",".join("%s=%d" % kv for kv in c[2].items()) or "default"
    print("%-8s %-5s  %-36s %.4f  (%.4f .. %.4f)" % (c[0], c[1], kn, np.median(r), min(r), max(r)))
med = {(c[0], c[1], tuple(c[2].items())): np.median(res[i]) for i, c in enumerate(cfgs)}
for what in ("hop2", "hop1", "step"):
    print("ratio bf16 / f32 %-5s %.3f" % (what, med[(what, "bf16", ())] / med[(what, "f32", ())]))
