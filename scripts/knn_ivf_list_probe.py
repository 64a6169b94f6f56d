"""The list-major schedule of the IVF-Flat search (KnnIvf.search(schedule="list"), glx_knn_ivf_search_ex) next to the
query-major schedule and the exact search (glx.Features.search), on the shapes of profiles/r24/knn_ivf.txt.

  table    owned 10 M x 128, float32 and bfloat16, two data sets:
           "mixture"  rows = one of 1,000 centres ~ N(0, I) + 0.3 * N(0, I); queries drawn the same way
           "gauss"    rows and queries ~ N(0, I): nothing to cluster
  index    nlist = 4,096, niter = 10, the default sample
  search   64 and 4,096 queries; nprobe = 1, 8, 32, 128; k = 20 and 100; both metrics
  legs     schedule="query", schedule="list", Features.search -- one process, the three legs interleaved repetition
           by repetition, device events around the whole call, 3 warm-ups of every leg, then 10 timed repetitions:
           the median and min .. max of each leg

Per shape the two schedules must return equal bits (asserted).  "redo" is the number of queries that took the overflow
path of the list-major schedule.  The engine keeps its flags in its workspace and exports none, so the count is
recomputed here after the timed runs from the rule the engine applies -- a query overflows when more rows of its probe
ranks >= 1 score at least as well as the k-th best row of its best list than the candidate buffer holds per query -- with
scores from a torch matmul: a score within rounding of the threshold may be counted differently.

No ratio is promised.  Usage: python scripts/knn_ivf_list_probe.py [rows] [nlist] > profiles/knn_ivf_list/probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

WARMUP, REPS = 3, 10
DIM = 128
BUDGET_KEYS = (256 << 20) // 8


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(legs):
    """[(median, min, max) ms per leg]: every repetition runs each leg once, in turn"""
    for _ in range(WARMUP):
        for fn in legs:
            once(fn)
    t = [[] for _ in legs]
    for _ in range(REPS):
        for i, fn in enumerate(legs):
            t[i].append(once(fn))
    return [(sorted(x)[len(x) // 2], min(x), max(x)) for x in t]


def rows_of(kind, n, centres):
    out = torch.randn(n, DIM, device="cuda")
    if kind == "mixture":
        out.mul_(0.3).add_(centres[torch.randint(0, centres.shape[0], (n,), device="cuda")])
    return out


def redone(f, ix, cents, assign, X32, q, k, metric, nprobe):
    """queries whose survivors of probe ranks >= 1 exceed the candidate buffer (see the module's text)"""
    nq, rows = q.shape[0], X32.shape[0]
    if nprobe == 1:
        return 0
    KP = 1 << (k - 1).bit_length()
    qb = min(max(BUDGET_KEYS // (nprobe * KP), 1), nq)
    cap = min(BUDGET_KEYS // qb, rows)
    lists = cents.search(q, nprobe, metric)[0][:, 1:]
    member = torch.zeros((nq, ix.nlist), dtype=torch.bool, device="cuda")
    member.scatter_(1, lists, True)
    ids, dist = ix.search(q, k, metric, nprobe=1)
    thr = dist[:, k - 1:k]
    open_thr = ids[:, k - 1:k] < 0  # the best list held fewer than k rows: everything passes
    count = torch.zeros(nq, dtype=torch.int64, device="cuda")
    qn = (q * q).sum(1, keepdim=True)
    for r0 in range(0, rows, 1 << 16):
        x = X32[r0:r0 + (1 << 16)].float()
        s = q @ x.T
        if metric == "l2":
            ok = (qn + (x * x).sum(1)[None, :] - 2 * s).clamp_(min=0) <= thr
        else:
            ok = s >= thr
        count += ((ok | open_thr) & member[:, assign[r0:r0 + (1 << 16)]]).sum(1)
    return int((count > cap).sum())


def say(*a):
    print(*a)
    sys.stdout.flush()


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    nlist = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    torch.manual_seed(0)
    say("KNN IVF list-major probe: table %d x %d, nlist %d, legs interleaved, %d warm-ups, medians of %d (min .. max), "
        "device %s" % (rows, DIM, nlist, WARMUP, REPS, torch.cuda.get_device_name(0)))
    for kind in ("mixture", "gauss"):
        centres = torch.randn(1000, DIM, device="cuda")
        X32 = rows_of(kind, rows, centres)
        queries = {nq: rows_of(kind, nq, centres) for nq in (64, 4096)}
        for name in ("float32", "bfloat16"):
            f = glx.Features(X32, dtype=None if name == "float32" else name)
            ix = f.build_ivf(nlist)
            cents = glx.Features(torch.from_numpy(ix.centroids()).cuda())
            ptr, list_rows = ix.lists()
            assign = torch.empty(rows, dtype=torch.int64)
            assign[torch.from_numpy(list_rows)] = torch.repeat_interleave(
                torch.arange(nlist), torch.from_numpy(ptr[1:] - ptr[:-1]))
            assign = assign.cuda()
            Xs = X32 if name == "float32" else X32.to(torch.bfloat16)
            say("\n%-8s %-9s %5s %4s %3s %6s | %28s | %28s | %28s | %7s %7s | %s" % (
                "data", "table", "nq", "k", "m", "nprobe", "query ms (min .. max)", "list ms (min .. max)",
                "exact ms (min .. max)", "q / l", "e / l", "redo"))
            for nq in (64, 4096):
                q = queries[nq]
                for k in (20, 100):
                    for metric in ("l2", "ip"):
                        outs = [(torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                                 torch.empty((nq, k), dtype=torch.float32, device="cuda")) for _ in range(3)]
                        for nprobe in (1, 8, 32, 128):
                            if nprobe > nlist:
                                continue
                            t = interleaved([
                                lambda: ix.search(q, k, metric, nprobe=nprobe, out=outs[0], schedule="query"),
                                lambda: ix.search(q, k, metric, nprobe=nprobe, out=outs[1], schedule="list"),
                                lambda: f.search(q, k, metric, out=outs[2])])
                            assert torch.equal(outs[0][0], outs[1][0]), (kind, name, nq, k, metric, nprobe)
                            assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
                            cell = ["%8.2f (%8.2f .. %8.2f)" % x for x in t]
                            say("%-8s %-9s %5d %4d %3s %6d | %s | %s | %s | %7.2f %7.2f | %d" % (
                                kind, name, nq, k, metric, nprobe, cell[0], cell[1], cell[2], t[0][0] / t[1][0],
                                t[2][0] / t[1][0], redone(f, ix, cents, assign, Xs, q, k, metric, nprobe)))
            cents.close()
            ix.close()
            f.close()
        del X32


if __name__ == "__main__":
    main()
