"""FP8 feature tables next to float32 and bfloat16 ones: what the quarter-size rows buy in time.  Nothing here is a
requirement of the test suite, and no ratio is promised.

  reduce   (default) one process, device events, medians of 10 after warm-up, repeated 3 times (the spread of the three
           medians is printed): C3's hop-2 request (RMAT 10 M / 100 M, EdgeWeight [25, 10], batch 65536: 16.4 M ids in
           1.64 M segments of 10, D = 256, Max) over the sampled id stream and over uniformly random ids -- the reduce on
           float32, bfloat16, float8_e4m3fn and float8_e5m2 tables at 4 columns per lane (agg_half_ld16=2) and, for the
           narrow types, at 8 columns per lane (agg_half_ld16=1); the lookup of the same id streams; C2's shape (D = 128, Mean) too.  Every
           narrow table's output is first checked bit for bit against the float32 table of its upcast values.
  pmc      a fixed launch sequence for a counter run of its own (rocprofv3 --pmc FETCH_SIZE, no tracing combined): the
           hop-2 reduce on the float32, bfloat16, e4m3 and e5m2 table, three times each.  Expected: 0.25x the float32
           bytes for float8.
  knn      a 10 M x 128 table, k = 20: the exact search with 64 and 4,096 queries and the IVF-Flat search (nlist 4,096,
           nprobe 8 and 32) per table type, with recall@20 of each type's answer against the float32 table's.

Usage: python scripts/r29/fp8_features_probe.py [reduce|pmc|knn] > profiles/r29/fp8_features.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import glx  # noqa: E402

TYPES = [("float32", None), ("bfloat16", torch.bfloat16), ("float8_e4m3fn", torch.float8_e4m3fn),
         ("float8_e5m2", torch.float8_e5m2)]
REPS, ROUNDS = 10, 3
dev = torch.device("cuda", 0)


def say(*a):
    print(*a)
    sys.stdout.flush()


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_of(fn, reps=REPS):
    return float(np.median([once(fn) for _ in range(reps)]))


def tables(X):
    return {name: glx.Features(X, dtype=None if tdt is None else name) for name, tdt in TYPES}


def reduce_mode(mode):
    import synth
    V, E, B0, k1, k2, GS = 10_000_000, 100_000_000, 65536, 25, 10, 4
    src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=True)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, w)
    del src, dst, w
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    seeds = pool[torch.randint(0, pool.shape[0], (B0,), generator=gen, device=dev)]
    n1, _ = g.sample("EdgeWeightSampler", seeds, k1, seed=42, call_counter=0)
    n2, _ = g.sample("EdgeWeightSampler", n1.view(-1), k2, seed=42, call_counter=1)
    streams = {"rmat": n2.view(-1).contiguous(),
               "uniform": torch.randint(0, V, (B0 * k1 * k2,), generator=gen, device=dev)}
    del g
    Sg = B0 * k1
    for D, agg, what in ((256, "MaxAggregator", "c3 hop-2"), (128, "MeanAggregator", "c2 shape")):
        X = synth.features_torch(V, D, GS + 1, dev)
        tabs = tables(X)
        emb = torch.empty((Sg, D), dtype=torch.float32, device=dev)
        cnt = torch.empty(Sg, dtype=torch.int32, device=dev)
        if mode == "pmc":
            if D != 256:
                break
            del X
            for _ in range(3):
                for name, _t in TYPES:
                    tabs[name].aggregate(agg, streams["rmat"], None, Sg, out=(emb, cnt))
            torch.cuda.synchronize()
            say("launch order: (%s) hop-2 reduce x 3 -- after the setup's sampling launches" % ", ".join(n for n, _ in TYPES))
            return
        # correctness first: every narrow table == the float32 table of its upcast values, for every setting timed
        for name, tdt in TYPES[1:]:
            up = glx.Features(X.to(tdt).float())
            for ld16 in (2, 1, 0):
                glx.tune("agg_half_ld16", 0)
                e, c = up.aggregate(agg, streams["rmat"], None, Sg)
                glx.tune("agg_half_ld16", ld16)
                e8, c8 = tabs[name].aggregate(agg, streams["rmat"], None, Sg, out=(emb, cnt))
                torch.cuda.synchronize()
                assert torch.equal(e.view(torch.int32), e8.view(torch.int32)) and torch.equal(c, c8), (name, ld16)
            del up, e, c
        del X
        torch.cuda.empty_cache()
        glx.tune("agg_half_ld16", 0)
        say("# %s: %d ids in %d segments of %d, D = %d, %s; device-event ms, median of %d, %d rounds: median (min .. max)"
            % (what, Sg * k2, Sg, k2, D, agg, REPS, ROUNDS))
        say("# narrow outputs verified bit-identical to the float32 table of the upcast values (both lane maps and the default)")
        say("%-8s %-8s %-14s %-9s %s" % ("ids", "launch", "table", "cols/lane", "ms"))
        look = torch.empty((1 << 20, D), dtype=torch.float32, device=dev)
        for sname, ids in streams.items():
            cfgs = [(name, ld16) for name, tdt in TYPES for ld16 in ((0,) if tdt is None else (2, 1))]
            res = {c: [] for c in cfgs}
            for c in cfgs:  # warm-up
                glx.tune("agg_half_ld16", c[1])
                tabs[c[0]].aggregate(agg, ids, None, Sg, out=(emb, cnt))
            for rnd in range(ROUNDS):
                for c in (cfgs if rnd % 2 == 0 else cfgs[::-1]):
                    glx.tune("agg_half_ld16", c[1])
                    res[c].append(median_of(lambda: tabs[c[0]].aggregate(agg, ids, None, Sg, out=(emb, cnt))))
            glx.tune("agg_half_ld16", 0)
            for c in cfgs:
                say("%-8s %-8s %-14s %-9d %.4f (%.4f .. %.4f)" % (sname, "reduce", c[0], 8 if c[1] == 1 else 4,
                                                                  np.median(res[c]), min(res[c]), max(res[c])))
            ids1m = ids[:1 << 20]
            for name, _t in TYPES:  # the lookup of the first 2^20 ids of the stream (its output is 4 D bytes per id)
                lib, h = glx.lib(), tabs[name]._h
                fn = lambda: glx._check(lib.glx_lookup(h, ids1m.data_ptr(), ids1m.shape[0], 0.0, look.data_ptr(),  # noqa: E731
                                                       glx.PTR_DEVICE, None))
                fn()
                r = [median_of(fn) for _ in range(ROUNDS)]
                say("%-8s %-8s %-14s %-9s %.4f (%.4f .. %.4f)" % (sname, "lookup", name, "-", np.median(r), min(r), max(r)))
        for t in tabs.values():
            t.close()
        del tabs, emb, cnt, look
        torch.cuda.empty_cache()


def knn_mode():
    N, D, K, nlist = 10_000_000, 128, 20, 4096
    torch.manual_seed(0)
    centres = torch.randn(1000, D, device=dev)

    def rows(n):
        return torch.randn(n, D, device=dev).mul_(0.3).add_(centres[torch.randint(0, 1000, (n,), device=dev)])

    X = rows(N)
    queries = {nq: rows(nq) for nq in (64, 4096)}
    say("# KNN: table %d x %d (mixture of 1,000 centres), k = %d; medians of %d; recall@%d against the float32 table's ids"
        % (N, D, K, REPS, K))
    say("%-14s %-6s %5s %3s %6s | %10s | %s" % ("table", "search", "nq", "m", "nprobe", "ms", "recall"))
    want = {}
    for name, tdt in TYPES:
        f = glx.Features(X, dtype=None if tdt is None else name)
        ix = f.build_ivf(nlist)
        for nq, q in queries.items():
            for metric in ("l2", "ip"):
                for nprobe in (0, 8, 32):  # 0: the exact search
                    fn = (lambda: f.search(q, K, metric)) if nprobe == 0 else (lambda: ix.search(q, K, metric, nprobe=nprobe))
                    ids, _ = fn()
                    ms = median_of(fn)
                    key = (nq, metric, nprobe)
                    want.setdefault(key, ids)
                    rec = float(((ids[:, :, None] == want[key][:, None, :]) & (want[key][:, None, :] >= 0)).any(1).float().mean())
                    say("%-14s %-6s %5d %3s %6s | %10.2f | %.4f" % (name, "exact" if nprobe == 0 else "ivf", nq, metric,
                                                                    "-" if nprobe == 0 else nprobe, ms, rec))
        ix.close()
        f.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "reduce"
    say("FP8 feature probe (%s), device %s" % (mode, torch.cuda.get_device_name(0)))
    if mode == "knn":
        knn_mode()
    else:
        reduce_mode(mode)
