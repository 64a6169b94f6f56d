"""The half-precision list-major IVF-Flat search (KnnIvf.search(schedule="list", precision="half"),
glx_knn_ivf_search_prec) next to the float32 list-major and query-major schedules on the same table and index.

  table    owned 10 M x 128, bfloat16 and float8_e4m3fn; rows = one of 1,000 centres ~ N(0, I) + 0.3 * N(0, I), queries
           drawn the same way
  index    nlist = 4,096, niter = 10, the default sample
  search   128, 1,024 and 8,192 queries; nprobe = 8, 32, 128; k = 20; inner product
  legs     float32 query-major (the default), float32 list-major, half list-major with refine 0 and 100 -- one process,
           the legs interleaved repetition by repetition, device events around the whole engine call, 3 warm-ups of
           every leg, then 10 timed repetitions: the median of each leg and the default leg's min .. max
  recall   recall@20 of every leg against the float32 flat answer (Features.search) on the same table
  rounds   R and the rounds per search, recomputed here from the engine's rule (glx_knn_ivf_half.hip): blocks of up to
           8,192 queries shrunk until cap = 2^25 / block >= the longest list, R = max(1, cap / longest), rounds =
           1 + ceil((nprobe - 1) / R)

No ratio is promised; it is reported whichever way it falls.
Usage: python scripts/knn_ivf_half_probe.py [rows] [nlist] > profiles/knn_ivf_half/probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

WARMUP, REPS = 3, 10
DIM, K = 128, 20
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


def rounds(nq, nprobe, longest, rows):
    qb = min(nq, 8192)
    if BUDGET_KEYS // qb < longest:
        qb = BUDGET_KEYS // longest
    R = max(1, min(BUDGET_KEYS // qb, rows) // longest)
    return R, 1 + -(-(nprobe - 1) // R)


def recall(ids, want):
    return ((ids[:, :, None] == want[:, None, :]) & (want[:, None, :] >= 0)).any(1).float().mean().item()


def say(*a):
    print(*a)
    sys.stdout.flush()


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    nlist = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    torch.manual_seed(0)
    say("KNN IVF half list-major probe: table %d x %d, nlist %d, k %d, ip, legs interleaved, %d warm-ups, medians of %d, "
        "device %s" % (rows, DIM, nlist, K, WARMUP, REPS, torch.cuda.get_device_name(0)))
    centres = torch.randn(1000, DIM, device="cuda")

    def draw(n):
        return torch.randn(n, DIM, device="cuda").mul_(0.3).add_(centres[torch.randint(0, 1000, (n,), device="cuda")])

    X32 = draw(rows)
    queries = {nq: draw(nq) for nq in (128, 1024, 8192)}
    for name in ("bfloat16", "float8_e4m3fn"):
        f = glx.Features(X32, dtype=name)
        ix = f.build_ivf(nlist)
        longest = ix.info()["longest_list"]
        say("\ntable %s, longest list %d rows" % (name, longest))
        say("%5s %6s | %30s | %9s %9s %9s | %7s %7s | %6s %6s %6s %6s | %4s %6s" % (
            "nq", "nprobe", "f32 query ms (min .. max)", "f32 list", "half", "half r100", "q / h", "l / h",
            "rc q", "rc l", "rc h", "rc h100", "R", "rounds"))
        for nq, q in queries.items():
            want = f.search(q, K, "ip")[0]
            outs = [(torch.empty((nq, K), dtype=torch.int64, device="cuda"),
                     torch.empty((nq, K), dtype=torch.float32, device="cuda")) for _ in range(4)]
            for nprobe in (8, 32, 128):
                if nprobe > nlist:
                    continue
                t = interleaved([
                    lambda: ix.search(q, K, "ip", nprobe=nprobe, out=outs[0], schedule="query"),
                    lambda: ix.search(q, K, "ip", nprobe=nprobe, out=outs[1], schedule="list"),
                    lambda: ix.search(q, K, "ip", nprobe=nprobe, out=outs[2], schedule="list", precision="half"),
                    lambda: ix.search(q, K, "ip", nprobe=nprobe, out=outs[3], schedule="list", precision="half",
                                      refine=100)])
                R, n_rounds = rounds(nq, nprobe, longest, rows)
                say("%5d %6d | %9.2f (%8.2f .. %8.2f) | %9.2f %9.2f %9.2f | %7.2f %7.2f | %6.4f %6.4f %6.4f %6.4f | %4d %6d" % (
                    nq, nprobe, t[0][0], t[0][1], t[0][2], t[1][0], t[2][0], t[3][0], t[0][0] / t[2][0],
                    t[1][0] / t[2][0], recall(outs[0][0], want), recall(outs[1][0], want), recall(outs[2][0], want),
                    recall(outs[3][0], want), R, n_rounds))
        ix.close()
        f.close()


if __name__ == "__main__":
    main()
