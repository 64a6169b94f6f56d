"""Probe of the split KNN scan (glx.Features.search(..., split=True)) on the shapes of scripts/knn_half_probe.py: one
owned 10 M x 128 float32 Gaussian table, 4,096 and 64 queries, k = 20 and 100, IP and L2.  Per shape the default search,
the split scan and the split scan with refine=1024 are interleaved in one process: medians (and min..max) of --reps
timed calls after --warmup, device events around the engine call; recall@k of the split answers against the default
answer; the largest |ip - float64| / bound over the returned IP scores (float64 over the float32 operands; the bound is
the contract's formula in include/glx.h).  A measurement, not a test.
Usage: python scripts/knn_split_probe.py [--rows 10000000] [--dim 128] [--reps 10] [--warmup 3] [--out profiles/knn_split/probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

MODES = (("default", {}), ("split", {"split": True}), ("split+refine1024", {"split": True, "refine": 1024}))


def timed(f, q, k, metric, kw):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = f.search(q, k, metric, **kw)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def ip_error(X, q, ids, ip, dim):
    """largest |ip - float64| / bound over the returned (query, row) pairs, a block of queries at a time"""
    worst = 0.0
    for q0 in range(0, q.shape[0], 64):
        qb = q[q0:q0 + 64].double()[:, None, :]
        xb = X[ids[q0:q0 + 64]].double()
        exact, terms = (qb * xb).sum(2), (qb * xb).abs().sum(2)
        bound = (6.2 * dim + 2) * 2.0 ** -23 * terms + 2.0 ** -133 * (qb.abs() + xb.abs()).sum(2) + 6 * dim * 2.0 ** -126
        worst = max(worst, ((ip[q0:q0 + 64].double() - exact).abs() / bound).max().item())
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_split", "probe.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("knn_split_probe: %s, %d x %d float32 table, medians of %d after %d warm-ups, ms [min..max]"
        % (torch.cuda.get_device_name(0), a.rows, a.dim, a.reps, a.warmup))
    gen = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((a.rows, a.dim), generator=gen, device="cuda", dtype=torch.float32)
    f = glx.Features(X)
    for nq in (4096, 64):
        q = torch.randn((nq, a.dim), generator=gen, device="cuda", dtype=torch.float32)
        for k in (20, 100):
            for metric in ("ip", "l2"):
                ms, ans = {m: [] for m, _ in MODES}, {}
                for rep in range(a.warmup + a.reps):
                    for mode, kw in MODES:
                        t, ans[mode] = timed(f, q, k, metric, kw)
                        if rep >= a.warmup:
                            ms[mode].append(t)
                med = {m: statistics.median(v) for m, v in ms.items()}
                text = "nq %d k %d %s:" % (nq, k, metric)
                for mode, _ in MODES:
                    text += "  %s %.2f [%.2f..%.2f]" % (mode, med[mode], min(ms[mode]), max(ms[mode]))
                    if mode != "default":
                        hit = (ans[mode][0][:, :, None] == ans["default"][0][:, None, :]).any(2).float().mean().item()
                        text += " x%.2f recall@%d %.4f" % (med["default"] / med[mode], k, hit)
                text += "  default's spread %.2f" % (max(ms["default"]) - min(ms["default"]))
                if metric == "ip":
                    text += "  largest |ip - float64| / bound %.4f" % ip_error(X, q, ans["split"][0], ans["split"][1], a.dim)
                say(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
