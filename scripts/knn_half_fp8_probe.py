"""Probe of the half-precision KNN scan over float8 tables (glx.Features.search(..., precision="half") on a float8_e4m3fn /
float8_e5m2 table) on the table of profiles/knn_half/probe.txt: owned 10 M x 128, 4,096 and 64 queries, k = 20 and 100,
IP and L2, refine 0 and 1,024.  Per shape three legs are interleaved in one process: the default search on the float8
table (what there was for this table before), the half scan on the float8 table, and the half scan on the bfloat16 table
of the same values.  Medians (and min..max) of --reps timed calls after --warmup, device events around the engine call.
The second and third legs must return equal bits (asserted per shape); recall@k is the scan's ids against the default
answer on the same float8 table.  A measurement, not a test.
Usage: python scripts/knn_half_fp8_probe.py [--rows 10000000] [--dim 128] [--reps 10] [--warmup 3]
                                            [--dtype float8_e4m3fn float8_e5m2] [--out profiles/knn_half_fp8/probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
from knn_half_probe import timed  # noqa: E402

LEGS = ("default", "half", "bf16 half")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", choices=sorted(glx.FP8_FEATURE_DTYPES), default=sorted(glx.FP8_FEATURE_DTYPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_half_fp8", "probe.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("knn_half_fp8_probe: %s, %d x %d table, medians of %d after %d warm-ups, ms [min..max]"
        % (torch.cuda.get_device_name(0), a.rows, a.dim, a.reps, a.warmup))
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name in a.dtype:
        X = torch.randn((a.rows, a.dim), generator=gen, device="cuda", dtype=torch.float32)
        f8 = glx.Features(X, dtype=name)  # rounded on the device
        del X
        up = f8.lookup(torch.arange(a.rows, device="cuda"))  # the table's values, upcast exactly
        f16 = glx.Features(up, dtype="bfloat16")  # every float8 number is a bfloat16 number: nothing is rounded
        del up
        torch.cuda.empty_cache()
        for nq in (4096, 64):
            q = torch.randn((nq, a.dim), generator=gen, device="cuda", dtype=torch.float32)
            for k in (20, 100):
                for metric in ("ip", "l2"):
                    for refine in (0, 1024):
                        half = {"precision": "half", "refine": refine}
                        legs = (("default", f8, {}), ("half", f8, half), ("bf16 half", f16, half))
                        ms, ans = {leg: [] for leg in LEGS}, {}
                        for rep in range(a.warmup + a.reps):
                            for leg, f, kw in legs:
                                t, ans[leg] = timed(f, q, k, metric, kw)
                                if rep >= a.warmup:
                                    ms[leg].append(t)
                        (ids8, dist8), (ids16, dist16) = ans["half"], ans["bf16 half"]
                        same = torch.equal(ids8, ids16) and torch.equal(dist8.view(torch.int32), dist16.view(torch.int32))
                        assert same, "%s nq %d k %d %s refine %d: the float8 scan and the bfloat16 scan differ" % (
                            name, nq, k, metric, refine)
                        med = {leg: statistics.median(v) for leg, v in ms.items()}
                        hit = (ans["half"][0][:, :, None] == ans["default"][0][:, None, :]).any(2).float().mean().item()
                        text = "%s nq %d k %d %s refine %d:" % (name, nq, k, metric, refine)
                        for leg in LEGS:
                            text += "  %s %.2f [%.2f..%.2f]" % (leg, med[leg], min(ms[leg]), max(ms[leg]))
                        text += "  default / half x%.2f  half / bf16 half x%.2f  recall@%d %.4f  bits equal" % (
                            med["default"] / med["half"], med["half"] / med["bf16 half"], k, hit)
                        say(text)
        del f8, f16
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
