"""XCD stripes of the grouped reduce on the bench's request shapes (c3, c3deg = degree-biased seeds, c2, c4s = C4's sampler and
D on the C3-sized graph).  `ab <wl>`: same-process A/B of the slice / stripe / chunk knobs (glx_tune), alternated;
`dump <wl>`: the hop-2 and hop-1 id streams as 24-bit files for scripts/l2_stripe_sim.py; `pmc`: a fixed launch
sequence for a counter pass (the parent's launch and the new default, three times each)."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
import numpy as np, torch, glx, synth
mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
wl = sys.argv[2] if len(sys.argv) > 2 else "c3"
OUT = os.path.join(ROOT, "bench_outputs")  # git-ignored
os.makedirs(OUT, exist_ok=True)
dev = torch.device("cuda", 0)
SMP, AGG, GS = "EdgeWeightSampler", "MaxAggregator", 4
V, E, D, B0, k1, k2 = 10_000_000, 100_000_000, 256, 65536, 25, 10
if wl == "c2":
    V, E, D, k1, k2, SMP, AGG, GS = 2_400_000, 62_000_000, 128, 15, 10, "RandomWithoutReplacementSampler", "MeanAggregator", 2
elif wl == "c4s":  # C4's sampler / fanout / dim on the C3-sized graph
    D, k1, k2, SMP, AGG, GS = 128, 20, 15, "RandomSampler", "MeanAggregator", 6
src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=(SMP == "EdgeWeightSampler"))
pool = src.clone() if wl == "c3deg" else torch.unique(src)
g = glx.Graph.from_edges(src, dst, w); del src, dst, w
f = glx.Features(synth.features_torch(V, D, GS + 1, dev))
gen = torch.Generator(device=dev); gen.manual_seed(1000)
Sg = B0 * k1
emb = torch.empty((Sg, D), dtype=torch.float32, device=dev); cnt = torch.empty(Sg, dtype=torch.int32, device=dev)
emb1 = torch.empty((B0, D), dtype=torch.float32, device=dev); cnt1 = torch.empty(B0, dtype=torch.int32, device=dev)
seeds = pool[torch.randint(0, pool.shape[0], (B0,), generator=gen, device=dev)]
n1, _ = g.sample(SMP, seeds, k1, seed=42, call_counter=0)
n2, _ = g.sample(SMP, n1.view(-1), k2, seed=42, call_counter=1)
torch.cuda.synchronize()
ids = {"hop2": n2.view(-1).contiguous(), "hop1": n1.view(-1).contiguous(),
       "uniform": torch.randint(0, V, (Sg * k2,), generator=gen, device=dev)}
KN = ("agg_xcd_slices", "agg_xcd_stripes", "agg_xcd_chunk")
def setk(x, st, c):
    glx.tune("agg_xcd_slices", x); glx.tune("agg_xcd_stripes", st); glx.tune("agg_xcd_chunk", c)
def run(name):
    i, sg, out = (ids[name], B0, (emb1, cnt1)) if name == "hop1" else (ids[name], Sg, (emb, cnt))
    f.aggregate(AGG, i, None, sg, out=out)
    return out
def timed(name, reps=5):
    r = []
    for _ in range(reps):
        torch.cuda.synchronize(); glx.profile_enable(True)
        run(name)
        torch.cuda.synchronize(); glx.profile_enable(False)
        r.append(float(glx.profile_collect(glx.KERNEL_AGGREGATE).sum()))
    return float(np.median(r))
if mode == "pmc":
    for rep in range(3):
        setk(2, 0, 0); run("hop2")  # the parent's launch: two slices, no stripes
        setk(0, -1, 0); run("hop2")  # the default now: stripes, n = 1 at D = 256
    torch.cuda.synchronize()
    print("launch order: (old default x2 no stripes, new default) x 3, every one the C3 hop-2 request")
    sys.exit(0)
if mode == "dump":  # 24-bit little-endian ids (all < 2^24): the stream fits the copy-back budget
    for name, t in (("hop2", n2), ("hop1", n1)):
        a = t.view(-1).to(torch.int32).cpu().numpy()
        assert a.min() >= 0 and a.max() < (1 << 24)
        a.view(np.uint8).reshape(-1, 4)[:, :3].tofile(os.path.join(OUT, "%s_%s_ids.u24" % (wl, name)))
    sys.exit(0)
cfgs = [("hop2", 2, 0, 0), ("hop2", 1, 0, 0), ("hop2", 1, 1, 16), ("hop2", 1, 1, 32), ("hop2", 1, 1, 64),
        ("hop2", 1, 1, 256), ("hop2", 2, 1, 32), ("uniform", 2, 0, 0), ("uniform", 1, 0, 0), ("uniform", 1, 1, 32),
        ("hop1", 1, 0, 0), ("hop1", 1, 1, 32)]
ref = {}
for name in ("hop2", "uniform", "hop1"):
    setk(0, 0, 0); o = run(name); torch.cuda.synchronize(); ref[name] = (o[0].clone(), o[1].clone())
res = {c: [] for c in cfgs}
for rnd in range(6):
    for c in (cfgs if rnd % 2 == 0 else cfgs[::-1]):
        setk(*c[1:]); res[c].append(timed(c[0]))
        if rnd == 0:
            o = run(c[0]); torch.cuda.synchronize()
            assert torch.equal(o[0], ref[c[0]][0]) and torch.equal(o[1], ref[c[0]][1]), c
setk(0, -1, 0)
print("# %s: %s [%d,%d] %s D=%d" % (wl, SMP, k1, k2, AGG, D))
print("# request  n  stripes chunk  median ms over 6 alternations (min .. max)  -- outputs bit-identical to x1/off")
for c in cfgs:
    r = res[c]
    print("%-8s x%d  %-3s  %4d   %.4f  (%.4f .. %.4f)" % (c[0], c[1], "on" if c[2] else "off", c[3], np.median(r), min(r), max(r)))
json.dump({"%s_x%d_s%d_c%d" % c: res[c] for c in cfgs}, open(os.path.join(OUT, "stripe_ab_%s.json" % wl), "w"))
