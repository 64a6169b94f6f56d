"""The samplers' row directory (GlxRowDir, csrc/glx_common.h) against the lookup it replaces (id map + row_ptr):
same-process A/B on the live C3 requests.

  python scripts/r21/row_dir_probe.py [OUT.txt]           (default: profiles/r21/row_dir_ab.txt)
  python scripts/r21/row_dir_probe.py --counters 0|dir|hash   one store, the EdgeWeight requests twice each: run it under
      rocprofv3 --pmc FETCH_SIZE TCP_TCC_READ_REQ_sum --kernel-include-regex glx_sample_slots (counters alone, no tracing)
  python scripts/r21/row_dir_probe.py --dump [OUT.npz]    the live hop-2 request ids and the store's row ids, for
      scripts/r21/row_dir_lines_model.py (default: build/r21/hop2_lookup.npz)

The C3 store (RMAT 10 M / 100 M, weighted) is built three times in one process: with GLX_ROW_DIR=0 (the parent's
launch), with the rule (GLX_ROW_DIR=1: direct for C3) and with GLX_ROW_DIR=hash.  The live hop-1 request (65,536 seeds x 25) and
hop-2 request (1,638,400 rows x 10) of EdgeWeightSampler run on each, six alternations, three timed launches per visit
(the median of them counts); then the same for RandomSampler with C4's fanouts (20, 15) and for TopkSampler (25, 10), on
the same store.  Outputs must be equal.  One process, one GPU, nothing read but the tree."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import glx  # noqa: E402
import synth  # noqa: E402

dev = torch.device("cuda", 0)
GS = 4
V, E, B0 = 10_000_000, 100_000_000, 65536
KINDS = {"0": "0", "dir": "1", "hash": "hash"}  # name -> GLX_ROW_DIR of the build ("1": the rule)
SAMPLERS = (("EdgeWeightSampler", 25, 10), ("RandomSampler", 20, 15), ("TopkSampler", 25, 10))


def build(src, dst, w, env):
    if env is None:
        os.environ.pop("GLX_ROW_DIR", None)
    else:
        os.environ["GLX_ROW_DIR"] = env
    try:
        return glx.Graph.from_edges(src, dst, w)
    finally:
        os.environ.pop("GLX_ROW_DIR", None)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].startswith("--") else None
    arg = sys.argv[2] if mode and len(sys.argv) > 2 else None
    out_path = sys.argv[1] if len(sys.argv) > 1 and not mode else os.path.join(ROOT, "profiles", "r21", "row_dir_ab.txt")
    src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=True)
    uniq = torch.unique(src)
    want = {"--counters": (arg,), "--dump": ("dir",)}.get(mode, tuple(KINDS))
    graphs = {name: build(src, dst, w, KINDS[name]) for name in want}
    del src, dst, w
    for name, g in graphs.items():
        print("# store %-4s row directory %s" % (name, g.row_dir()), flush=True)
    forms = {name: g.row_dir() for name, g in graphs.items()}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    seeds = uniq[torch.randint(0, uniq.shape[0], (B0,), generator=gen, device=dev)]
    first = next(iter(graphs.values()))

    def requests(smp, k1, k2):
        n1, _ = first.sample(smp, seeds, k1, seed=42, call_counter=0)
        reqs = {"hop1": (seeds, k1, 0), "hop2": (n1.view(-1).contiguous(), k2, 1)}
        outs = {r: (torch.empty((ids.shape[0], k), dtype=torch.int64, device=dev),
                    torch.empty((ids.shape[0], k), dtype=torch.int64, device=dev)) for r, (ids, k, _) in reqs.items()}
        return reqs, outs

    if mode == "--dump":
        out = arg or os.path.join(ROOT, "build", "r21", "hop2_lookup.npz")
        reqs, _ = requests(*SAMPLERS[0])
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        np.savez_compressed(out, ids=reqs["hop2"][0].cpu().numpy().astype(np.int32), uniq=uniq.cpu().numpy().astype(np.int32))
        print("dumped %d request ids, %d row ids -> %s" % (reqs["hop2"][0].shape[0], uniq.shape[0], out))
        return
    if mode == "--counters":
        reqs, outs = requests(*SAMPLERS[0])
        for r, (ids, k, cc) in reqs.items():
            for _ in range(2):
                graphs[arg].sample(SAMPLERS[0][0], ids, k, seed=42, call_counter=cc, out=outs[r])
                torch.cuda.synchronize()
        return

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# C3 store (RMAT 10 M / 100 M, weighted, %d rows), three builds in one process: %s" % (
        uniq.shape[0], ", ".join("%s = %s, %.1f MB" % (n, f[0], f[1] / 1e6) for n, f in forms.items())))
    say("# sampler  request  store  median ms over 6 alternations (min .. max)  each alternation")
    for smp, k1, k2 in SAMPLERS:
        reqs, outs = requests(smp, k1, k2)

        def run(name, r):
            ids, k, cc = reqs[r]
            return graphs[name].sample(smp, ids, k, seed=42, call_counter=cc, out=outs[r])

        for r in reqs:  # the same answers from all three
            a = [t.clone() for t in run("0", r)]
            for name in ("dir", "hash"):
                b = run(name, r)
                torch.cuda.synchronize()
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (smp, r, name)

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

        cfgs = [(r, name) for r in reqs for name in KINDS]
        res = {c: [] for c in cfgs}
        for rnd in range(6):
            for c in (cfgs if rnd % 2 == 0 else cfgs[::-1]):
                res[c].append(timed(c[1], c[0]))
        for c in cfgs:
            t = res[c]
            say("%-17s %-5s %dx%-2d %-4s  %.4f  (%.4f .. %.4f)  %s" % (
                smp, c[0], reqs[c[0]][0].shape[0], reqs[c[0]][1], c[1], np.median(t), min(t), max(t),
                " ".join("%.4f" % x for x in t)))
        for r in reqs:
            a = res[(r, "0")]
            for name in ("dir", "hash"):
                b = res[(r, name)]
                say("# %s %s: %s faster than 0 in %d of 6 alternations; ranges %s; median %+.1f %% (%+.4f ms)" % (
                    smp, r, name, sum(y < x for x, y in zip(a, b)), "do not overlap" if max(b) < min(a) else "OVERLAP",
                    100.0 * (np.median(b) - np.median(a)) / np.median(a), np.median(b) - np.median(a)))
    say("# outputs of the three stores compared equal in this run, for every sampler and request")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
