"""A first measurement of the IVF-PQ index (glx_knn_ivfpq_*, glx.KnnIvf.build_pq / glx.KnnIvfPq.search) next to the
IVF-Flat index (glx.KnnIvf.search) and the exact search (glx.Features.search) on the same owned table in the same run.

  table    10 M x 128 (the shape of profiles/r24/knn_ivf.txt), float32 and bfloat16, two data sets:
           "mixture"  rows = one of 1,000 centres ~ N(0, I) + 0.3 * N(0, I); queries drawn the same way
           "gauss"    rows and queries ~ N(0, I): nothing to cluster, the index's worst case
  index    nlist = 4,096, niter = 10, the default samples; m = 8, 16 and 32 sub-quantisers on the same lists
  search   64 and 4,096 queries; k = 20 and 100; both metrics; nprobe = 1, 8, 32 and 128; refine = 0, 128 and 1,024

Reported: build time and index bytes of both layers, the codes and the codebooks apart; per shape the IVF-Flat index's
time and the exact search's time in the same run, and for every refine the coded index's time and its recall@k against
the exact answer (the share of the exact search's ids it returned; the IVF-Flat index's recall stands next to it: the
coded index probes the same lists and cannot find more).  A coded search slower than the IVF-Flat search of the same
shape is marked "<ivf", one slower than the exact search "<exact"; the marks are counted at the end of every table.

The driver (no arguments beyond the sizes) runs one child process per (data set, table type), each under its own time
limit, and stops at the first child that fails.  A child: one process, HIP events, 2 warm-up + 10 timed repetitions,
medians; a call that takes longer than 2 s is timed once (marked "x1").
Nothing here is a requirement of the test suite, and no ratio is promised.
Usage: python scripts/r26/knn_ivfpq_probe.py [--rows N] [--nlist L] [--kinds mixture,gauss] [--dtypes float32,bfloat16]
                                             [--metrics l2,ip] > profiles/r26/knn_ivfpq.txt"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

WARMUP, REPS = 2, 10
DIM = 128
SLOW_MS = 2000.0
CHILD_LIMIT_S = 1100
MS, REFINES, NPROBES = (8, 16, 32), (0, 128, 1024), (1, 8, 32, 128)


def say(*a):
    print(*a)
    sys.stdout.flush()


def child(a, kind, name):
    import torch
    import glx

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        """(median ms, runs timed)"""
        first = once(fn)
        if first > SLOW_MS:
            return first, 1
        for _ in range(WARMUP - 1):
            once(fn)
        t = sorted(once(fn) for _ in range(REPS))
        return t[len(t) // 2], REPS

    def recall(got, want):
        hit = (got[:, :, None] == want[:, None, :]) & (want[:, None, :] >= 0)
        return float(hit.any(1).float().mean())

    def rows_of(n, centres):
        out = torch.randn(n, DIM, device="cuda")
        if kind == "mixture":
            out.mul_(0.3).add_(centres[torch.randint(0, centres.shape[0], (n,), device="cuda")])
        return out

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    torch.manual_seed(0 if kind == "mixture" else 1)
    centres = torch.randn(1000, DIM, device="cuda")
    X32 = rows_of(a.rows, centres)
    queries = {nq: rows_of(nq, centres) for nq in (64, 4096)}
    f = glx.Features(X32, dtype=None if name == "float32" else name)
    del X32
    ix, build_s = wall(lambda: f.build_ivf(a.nlist))
    say("\n%s %s: table %.1f MB; ivf build %.2f s, %.1f MB" % (kind, name, a.rows * DIM * (4 if name == "float32" else 2) / 1e6,
                                                             build_s, ix.info()["device_bytes"] / 1e6))
    coded = {}
    for m in MS:
        coded[m], build_s = wall(lambda: ix.build_pq(m))
        say("%s %s: ivfpq m %2d build %.2f s, codes %.1f MB + codebooks and norms %.2f MB" % (
            kind, name, m, build_s, a.rows * m / 1e6, (coded[m].info()["device_bytes"] - a.rows * m) / 1e6))
    say("%-8s %-9s %5s %4s %3s %6s %3s | %9s %9s %7s |%s" % (
        "data", "table", "nq", "k", "met", "nprobe", "m", "exact ms", "ivf ms", "ivf rec",
        "".join(" %9s %7s %-10s|" % ("r%d ms" % r, "recall", "") for r in REFINES)))
    slower_ivf = slower_exact = shapes = 0
    for nq in (64, 4096):
        q = queries[nq]
        for k in (20, 100):
            for metric in a.metrics:
                want = (torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                        torch.empty((nq, k), dtype=torch.float32, device="cuda"))
                got = (torch.empty_like(want[0]), torch.empty_like(want[1]))
                exact_ms, _ = timed(lambda: f.search(q, k, metric, out=want))
                for nprobe in NPROBES:
                    ivf_ms, _ = timed(lambda: ix.search(q, k, metric, nprobe=nprobe, out=got))
                    ivf_rec = recall(got[0], want[0])
                    for m in MS:
                        cells = ""
                        for refine in REFINES:
                            ms, runs = timed(lambda: coded[m].search(q, k, metric, nprobe=nprobe, refine=refine, out=got))
                            marks = ("<ivf " if ms > ivf_ms else "") + ("<exact" if ms > exact_ms else "")
                            shapes += 1
                            slower_ivf += ms > ivf_ms
                            slower_exact += ms > exact_ms
                            cells += " %9.2f %7.4f %-10s|" % (ms, recall(got[0], want[0]), marks + ("x1" if runs == 1 else ""))
                        say("%-8s %-9s %5d %4d %3s %6d %3d | %9.2f %9.2f %7.4f |%s" % (
                            kind, name, nq, k, metric, nprobe, m, exact_ms, ivf_ms, ivf_rec, cells))
    say("%s %s: of %d coded shapes %d are slower than the IVF-Flat search of the same shape, %d slower than the exact "
        "search" % (kind, name, shapes, slower_ivf, slower_exact))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--kinds", default="mixture,gauss")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--metrics", default="l2,ip")
    ap.add_argument("--step", default=None, help="kind:dtype -- run that table in this process")
    a = ap.parse_args()
    a.metrics = a.metrics.split(",")
    if a.step:
        child(a, *a.step.split(":"))
        return 0
    say("KNN IVF-PQ probe: table %d x %d, nlist %d, m %s, refine %s, metrics %s, medians of %d" % (
        a.rows, DIM, a.nlist, MS, REFINES, ",".join(a.metrics), REPS))
    for kind in a.kinds.split(","):
        for name in a.dtypes.split(","):
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--rows", str(a.rows),
                   "--nlist", str(a.nlist), "--metrics", ",".join(a.metrics), "--step", "%s:%s" % (kind, name)]
            rc = subprocess.call(cmd)
            if rc != 0:  # a fault, an abort or the time limit: nothing more is started on the device
                say("%s %s: the step ended with status %d; stopping" % (kind, name, rc))
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
