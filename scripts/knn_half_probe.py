"""Probe of the half-precision KNN scan (glx.Features.search(..., precision="half")) on the shapes of
profiles/r20/knn.txt: owned 10 M x 128 bfloat16 and float16 tables, 4,096 and 64 queries, k = 20 and 100, IP and L2.
Per shape the default search, the half scan and the half scan with refine=1024 are interleaved in one process: medians
(and min..max) of --reps timed calls after --warmup, device events around the engine call; recall@k of the half
answers against the default answer.  Then, per dtype, the largest |ip - exact| / bound seen on a Gaussian sample (float64
over the rounded operands; bound = dim * 2^-23 * sum|terms|, the contract's) and whether a subnormal operand contributed
to a score.  A measurement, not a test.  float8 tables: scripts/knn_half_fp8_probe.py, whose legs span two tables.
Usage: python scripts/knn_half_probe.py [--rows 10000000] [--dim 128] [--reps 10] [--warmup 3] [--out profiles/knn_half/probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

MODES = (("default", {}), ("half", {"precision": "half"}), ("half+refine1024", {"precision": "half", "refine": 1024}))


def timed(f, q, k, metric, kw):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = f.search(q, k, metric, **kw)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_half", "probe.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("knn_half_probe: %s, %d x %d table, medians of %d after %d warm-ups, ms [min..max]"
        % (torch.cuda.get_device_name(0), a.rows, a.dim, a.reps, a.warmup))
    gen = torch.Generator(device="cuda").manual_seed(0)
    for dtype in (torch.bfloat16, torch.float16):
        name = str(dtype).replace("torch.", "")
        X = torch.randn((a.rows, a.dim), generator=gen, device="cuda", dtype=torch.float32).to(dtype)
        f = glx.Features(X)
        del X
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
                    text = "%s nq %d k %d %s:" % (name, nq, k, metric)
                    for mode, _ in MODES:
                        text += "  %s %.2f [%.2f..%.2f]" % (mode, med[mode], min(ms[mode]), max(ms[mode]))
                        if mode != "default":
                            hit = (ans[mode][0][:, :, None] == ans["default"][0][:, None, :]).any(2).float().mean().item()
                            text += " x%.2f recall@%d %.4f" % (med["default"] / med[mode], k, hit)
                    spread = max(ms["default"]) - min(ms["default"])
                    text += "  default - half %.2f vs default's spread %.2f" % (med["default"] - med["half"], spread)
                    say(text)
        # error against the contract's bound: every score of a small Gaussian table (k = num_rows returns them all)
        Xs = torch.randn((1024, a.dim), generator=gen, device="cuda", dtype=torch.float32).to(dtype)
        qs = torch.randn((256, a.dim), generator=gen, device="cuda", dtype=torch.float32)
        ids, ip = glx.Features(Xs).search(qs, 1024, "ip", precision="half")
        qr, xr = qs.to(dtype).double(), Xs.double()
        exact = torch.gather(qr @ xr.T, 1, ids)
        bound = a.dim * 2.0 ** -23 * torch.gather(qr.abs() @ xr.abs().T, 1, ids)
        say("%s largest |ip - exact| / bound on 256 x 1024 Gaussian scores: %.4f"
            % (name, ((ip.double() - exact).abs() / bound).max().item()))
        # a subnormal table element times a query that brings the product into the normal range
        tiny = 2.0 ** -130 if dtype == torch.bfloat16 else 2.0 ** -20
        scale = 2.0 ** 100 if dtype == torch.bfloat16 else 1.0
        Xt = torch.zeros((1, 16), device="cuda", dtype=dtype)
        Xt[0, 0] = tiny
        qt = torch.zeros((1, 16), device="cuda", dtype=torch.float32)
        qt[0, 0] = scale
        got = glx.Features(Xt).search(qt, 1, "ip", precision="half")[1].item()
        say("%s subnormal operand %g x %g: score %g (%s)" % (name, tiny, scale, got,
            "contributed" if got == tiny * scale else "flushed to zero" if got == 0 else "unexpected"))
        del f
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
