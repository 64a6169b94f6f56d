"""A first measurement of the IVF-Flat index (glx_knn_ivf_*, glx.Features.build_ivf / glx.KnnIvf.search) next to the
exact search (glx.Features.search) on the same owned table in the same run.

  table    10 M x 128 (the shape of profiles/r20/knn.txt), float32 and bfloat16, two data sets:
           "mixture"  rows = one of 1,000 centres ~ N(0, I) + 0.3 * N(0, I); queries drawn the same way
           "gauss"    rows and queries ~ N(0, I): nothing to cluster, the index's worst case
  index    nlist = 4,096, niter = 10, the default sample (256 * nlist rows)
  search   64 and 4,096 queries; k = 20 and 100; both metrics; nprobe = 1, 8, 32, 128 and nlist

Reported: build time, index bytes, list lengths (min / median / longest); per shape the index's time, the exact search's
time in the same run, their ratio (above 1: the index is faster) and recall@k against the exact answer (the share of the
exact search's ids the index returned).  With nprobe = nlist the ids must equal the exact search's: "recall" 1.0000.

One process, HIP events, 2 warm-up + 10 timed repetitions, medians; a call that takes longer than 2 s is timed once
(marked "x1").  4,096 queries with nprobe = nlist re-read the table once per query: measured for k = 20 only.
Nothing here is a requirement of the test suite, and no ratio is promised.
Usage: python scripts/r24/knn_ivf_probe.py [rows] [nlist] > profiles/r24/knn_ivf.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

WARMUP, REPS = 2, 10
DIM = 128
SLOW_MS = 2000.0


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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


def rows_of(kind, n, centres):
    out = torch.randn(n, DIM, device="cuda")
    if kind == "mixture":
        out.mul_(0.3).add_(centres[torch.randint(0, centres.shape[0], (n,), device="cuda")])
    return out


def say(*a):
    print(*a)
    sys.stdout.flush()


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    nlist = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    torch.manual_seed(0)
    say("KNN IVF probe: table %d x %d, nlist %d, medians of %d, device %s" % (rows, DIM, nlist, REPS,
                                                                          torch.cuda.get_device_name(0)))
    for kind in ("mixture", "gauss"):
        centres = torch.randn(1000, DIM, device="cuda")
        X32 = rows_of(kind, rows, centres)
        queries = {nq: rows_of(kind, nq, centres) for nq in (64, 4096)}
        for name in ("float32", "bfloat16"):
            f = glx.Features(X32, dtype=None if name == "float32" else name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix = f.build_ivf(nlist)
            torch.cuda.synchronize()
            build_s = time.perf_counter() - t0
            ptr, _ = ix.lists()
            sizes = sorted((ptr[1:] - ptr[:-1]).tolist())
            info = ix.info()
            say("\n%s %s: build %.2f s, index %.1f MB (table %.1f MB), lists min %d / median %d / longest %d" % (
                kind, name, build_s, info["device_bytes"] / 1e6, rows * DIM * (4 if name == "float32" else 2) / 1e6,
                sizes[0], sizes[len(sizes) // 2], info["longest_list"]))
            say("%-8s %-9s %5s %4s %3s %6s | %10s %4s %10s %7s | %s" % ("data", "table", "nq", "k", "m", "nprobe", "ivf ms",
                                                                      "runs", "exact ms", "ratio", "recall@k"))
            for nq in (64, 4096):
                q = queries[nq]
                for k in (20, 100):
                    for metric in ("l2", "ip"):
                        want = (torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                                torch.empty((nq, k), dtype=torch.float32, device="cuda"))
                        got = (torch.empty_like(want[0]), torch.empty_like(want[1]))
                        exact_ms, _ = timed(lambda: f.search(q, k, metric, out=want))
                        for nprobe in (1, 8, 32, 128, nlist):
                            if nprobe > nlist or (nprobe == nlist and nq == 4096 and k != 20):
                                continue
                            ms, runs = timed(lambda: ix.search(q, k, metric, nprobe=nprobe, out=got))
                            say("%-8s %-9s %5d %4d %3s %6d | %10.2f %4s %10.2f %7.2f | %.4f" % (
                                kind, name, nq, k, metric, nprobe, ms, "x%d" % runs, exact_ms, exact_ms / ms,
                                recall(got[0], want[0])))
            ix.close()
            f.close()
        del X32


if __name__ == "__main__":
    main()
