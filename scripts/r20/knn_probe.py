"""A first measurement of the exact KNN search (glx_knn_search, glx.Features.search): the k best rows of a device
feature table for a batch of queries, against the same request as chunked torch.topk(q @ X.T) under the same workspace
budget (256 MiB of scores at a time, the running k best merged by a second topk), on the same machine in the same run.

  table    10 M x 128 float32, and its bfloat16 form (the torch leg multiplies the upcast float32 copy of the bfloat16
           table chunk by chunk, so both legs read 2-byte rows)
  queries  4,096 and 64;  k = 20 and 100;  both metrics

Reported per shape: the engine's time, the float32 TFLOP/s that 2 * rows * queries * dim implies -- against the 157 TF
float32 matrix peak and the 122 TF of an untuned LDS-tiled MFMA GEMM -- and the torch leg's time.  The survivors per
chunk and the select kernel's share are not reported: the search keeps no counters.

One process, HIP events, 2 warm-up + 10 timed repetitions, legs interleaved, medians.  Nothing here is a requirement of
the test suite, and no ratio is promised.
Usage: python scripts/r20/knn_probe.py [rows] > profiles/r20/knn.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

WARMUP, REPS = 2, 10
DIM = 128
BUDGET = 256 << 20
PEAK_TF, GEMM_TF = 157.0, 122.0


def timed(legs):
    times = {k: [] for k in legs}
    for rep in range(WARMUP + REPS):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= WARMUP:
                times[name].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def torch_topk(X, q, k, metric, xn):
    """chunked topk(q @ X.T) with the running k best merged chunk by chunk; X float32 or bfloat16 (upcast per chunk)"""
    nq = q.shape[0]
    chunk = max(1024, BUDGET // (4 * nq))
    best_d = best_i = None
    qn = (q * q).sum(1, keepdim=True) if metric == "l2" else None
    for r0 in range(0, X.shape[0], chunk):
        Xc = X[r0:r0 + chunk].float()
        s = q @ Xc.T
        if metric == "l2":
            s = (qn + xn[r0:r0 + chunk][None, :] - 2 * s).clamp_(min=0)
        d, i = torch.topk(s, min(k, s.shape[1]), dim=1, largest=metric == "ip")
        i = i + r0
        if best_d is not None:
            d, i = torch.cat([best_d, d], 1), torch.cat([best_i, i], 1)
            d, sel = torch.topk(d, k, dim=1, largest=metric == "ip")
            i = torch.gather(i, 1, sel)
        best_d, best_i = d, i
    return best_i, best_d


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    torch.manual_seed(0)
    X32 = torch.randn(rows, DIM, device="cuda")
    X16 = X32.to(torch.bfloat16)
    print("KNN probe: table %d x %d, medians of %d, device %s" % (rows, DIM, REPS, torch.cuda.get_device_name(0)))
    print("%-9s %6s %4s %3s | %10s %8s %7s %7s | %10s %7s | %s" % ("table", "nq", "k", "m", "glx ms", "TFLOP/s", "/157",
                                                               "/122", "torch ms", "ratio", "ids equal"))
    for name, X in (("float32", X32), ("bfloat16", X16)):
        f = glx.Features(X, view=True)
        xn = (X.float() ** 2).sum(1) if rows <= 20_000_000 else None
        for nq in (4096, 64):
            q = torch.randn(nq, DIM, device="cuda")
            for k in (20, 100):
                for metric in ("ip", "l2"):
                    out = (torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                           torch.empty((nq, k), dtype=torch.float32, device="cuda"))
                    t = timed({"glx": lambda: f.search(q, k, metric, out=out),
                               "torch": lambda: torch_topk(X, q, k, metric, xn)})
                    ti, _ = torch_topk(X, q, k, metric, xn)
                    same = float((ti == out[0]).float().mean())
                    tf = 2.0 * rows * nq * DIM / (t["glx"] * 1e-3) / 1e12
                    print("%-9s %6d %4d %3s | %10.2f %8.2f %7.3f %7.3f | %10.2f %7.2f | %.4f" % (
                        name, nq, k, metric, t["glx"], tf, tf / PEAK_TF, tf / GEMM_TF, t["torch"], t["torch"] / t["glx"],
                        same))
                    sys.stdout.flush()
        del f


if __name__ == "__main__":
    main()
