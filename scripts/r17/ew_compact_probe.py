"""EdgeWeight sampling over 20-byte records against the 32-byte records (GlxEwRec20 / GlxEwRec, csrc/glx_common.h):
same-process A/B on the live C3 requests.

  python scripts/r17/ew_compact_probe.py [OUT.txt]          (default: profiles/r17/ew_compact_ab.txt)
  python scripts/r17/ew_compact_probe.py --counters 32|20   one store, each request twice: run it under
      rocprofv3 --pmc FETCH_SIZE TCP_TCC_READ_REQ_sum --kernel-include-regex glx_sample_slots (counters alone, no tracing)

The C3 store (RMAT 10 M / 100 M, weighted) is built twice in one process, once with GLX_EW_PACKED=32 set for the build
and once with the default rule; both fit many times over.  The live hop-1 request (65,536 seeds x 25) and hop-2 request
(1,638,400 rows x 10) run on each, six alternations, three timed launches per visit (the median of them counts);
outputs must be equal.  One process, one GPU, nothing read but the tree."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import glx  # noqa: E402
import synth  # noqa: E402

dev = torch.device("cuda", 0)
SMP, GS = "EdgeWeightSampler", 4
V, E, B0, k1, k2 = 10_000_000, 100_000_000, 65536, 25, 10


def build(src, dst, w, env):
    if env is None:
        os.environ.pop("GLX_EW_PACKED", None)
    else:
        os.environ["GLX_EW_PACKED"] = env
    try:
        return glx.Graph.from_edges(src, dst, w)
    finally:
        os.environ.pop("GLX_EW_PACKED", None)


def main():
    counters = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--counters" else None
    out_path = sys.argv[1] if len(sys.argv) > 1 and not counters else os.path.join(ROOT, "profiles", "r17", "ew_compact_ab.txt")
    src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=True)
    uniq = torch.unique(src)
    kinds = {"32": "32", "20": None}
    graphs = {name: build(src, dst, w, env) for name, env in kinds.items() if counters in (None, name)}
    del src, dst, w
    for name, g in graphs.items():
        assert g.edge_weight_record_bytes() == int(name), (name, g.edge_weight_record_bytes())
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    seeds = uniq[torch.randint(0, uniq.shape[0], (B0,), generator=gen, device=dev)]
    del uniq
    first = next(iter(graphs.values()))
    n1, _ = first.sample(SMP, seeds, k1, seed=42, call_counter=0)
    reqs = {"hop1": (seeds, k1, 0), "hop2": (n1.view(-1).contiguous(), k2, 1)}
    outs = {r: (torch.empty((ids.shape[0], k), dtype=torch.int64, device=dev),
                torch.empty((ids.shape[0], k), dtype=torch.int64, device=dev)) for r, (ids, k, _) in reqs.items()}

    def run(name, r):
        ids, k, cc = reqs[r]
        return graphs[name].sample(SMP, ids, k, seed=42, call_counter=cc, out=outs[r])

    if counters:
        for r in reqs:
            for _ in range(2):
                run(counters, r)
                torch.cuda.synchronize()
        return

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for r in reqs:  # the same answers from both tables
        a = [t.clone() for t in run("32", r)]
        b = run("20", r)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), r

    def timed(name, r, reps=3):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            glx.profile_enable(True)
            run(name, r)
            torch.cuda.synchronize()
            glx.profile_enable(False)
            t.append(float(glx.profile_collect(glx.KERNEL_SAMPLE).sum()))
        return float(np.median(t))

    cfgs = [(r, name) for r in reqs for name in ("32", "20")]
    res = {c: [] for c in cfgs}
    for rnd in range(6):
        for c in (cfgs if rnd % 2 == 0 else cfgs[::-1]):
            res[c].append(timed(c[1], c[0]))
    say("# C3 store (RMAT 10 M / 100 M, weighted), %s, both tables in one process; outputs equal" % SMP)
    say("# request  record bytes  median ms over 6 alternations (min .. max)  each alternation")
    for c in cfgs:
        t = res[c]
        say("%-5s %s  %.4f  (%.4f .. %.4f)  %s" % (c[0], c[1], np.median(t), min(t), max(t), " ".join("%.4f" % x for x in t)))
    for r in reqs:
        a, b = res[(r, "32")], res[(r, "20")]
        say("# %s: 20-byte faster in %d of 6 alternations; ranges %s; median %+.1f %%" % (
            r, sum(y < x for x, y in zip(a, b)), "do not overlap" if max(b) < min(a) else "OVERLAP",
            100.0 * (np.median(b) - np.median(a)) / np.median(a)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
