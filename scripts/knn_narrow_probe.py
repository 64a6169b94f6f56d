"""Probe of the narrow KNN tile (glx.Features.search(..., tile="narrow")) at the few-queries end: an owned 10 M x 128
Gaussian table, 1 to 512 queries, k = 20 and 100, IP and L2.  Per shape five legs are interleaved in one process: the
wide and the narrow tile at precision="float32" on the float32 table, the wide and the narrow tile at precision="half"
on the bfloat16 table, and chunked torch.topk(q @ X.T) on the float32 table under the same 256 MiB of scores at a time
(scripts/r20/knn_probe.py's comparator).  Medians (and min..max) of --reps timed calls after --warmup, device events
around the whole engine call.  The narrow answer must equal the wide answer bit for bit on every shape (asserted).  A
narrow - wide difference counts only beyond the wide leg's own min..max spread, which is printed next to it.  The floor:
a device-to-device copy of each table's bytes (one read and one write of them), timed the same way in the same run.
A measurement, not a test.
Usage: python scripts/knn_narrow_probe.py [--rows 10000000] [--dim 128] [--reps 10] [--warmup 3] [--out profiles/knn_narrow/probe.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402

BUDGET = 256 << 20


def timed(call):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def torch_topk(X, q, k, metric, xn):
    """chunked topk(q @ X.T) with the running k best merged chunk by chunk"""
    chunk = max(1024, BUDGET // (4 * q.shape[0]))
    best_d = best_i = None
    qn = (q * q).sum(1, keepdim=True) if metric == "l2" else None
    for r0 in range(0, X.shape[0], chunk):
        s = q @ X[r0:r0 + chunk].T
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


def same_bits(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_narrow", "probe.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("knn_narrow_probe: %s, %d x %d table, medians of %d after %d warm-ups, ms [min..max]"
        % (torch.cuda.get_device_name(0), a.rows, a.dim, a.reps, a.warmup))
    gen = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((a.rows, a.dim), generator=gen, device="cuda", dtype=torch.float32)
    xn = (X * X).sum(1)
    f32, f16 = glx.Features(X), glx.Features(X.to(torch.bfloat16))
    for name, src in (("float32", X), ("bfloat16", X.to(torch.bfloat16))):
        dst = torch.empty_like(src)
        ms = [timed(lambda: dst.copy_(src))[0] for _ in range(a.warmup + a.reps)][a.warmup:]
        say("floor: device copy of the %s table's %.2f GB (read + write): %.2f [%.2f..%.2f]"
            % (name, src.numel() * src.element_size() / 1e9, statistics.median(ms), min(ms), max(ms)))
        del dst, src
    torch.cuda.empty_cache()
    for metric in ("ip", "l2"):
        for k in (20, 100):
            for nq in (1, 8, 32, 64, 128, 512):
                q = torch.randn((nq, a.dim), generator=gen, device="cuda", dtype=torch.float32)
                legs = (("f32 wide", lambda: f32.search(q, k, metric)),
                        ("f32 narrow", lambda: f32.search(q, k, metric, tile="narrow")),
                        ("half wide", lambda: f16.search(q, k, metric, precision="half")),
                        ("half narrow", lambda: f16.search(q, k, metric, precision="half", tile="narrow")),
                        ("torch", lambda: torch_topk(X, q, k, metric, xn)))
                ms, ans = {m: [] for m, _ in legs}, {}
                for rep in range(a.warmup + a.reps):
                    for leg, call in legs:
                        t, ans[leg] = timed(call)
                        if rep >= a.warmup:
                            ms[leg].append(t)
                med = {m: statistics.median(v) for m, v in ms.items()}
                text = "%s k %d nq %d:" % (metric, k, nq)
                for leg, _ in legs:
                    text += "  %s %.2f [%.2f..%.2f]" % (leg, med[leg], min(ms[leg]), max(ms[leg]))
                for p in ("f32", "half"):
                    wide, narrow = p + " wide", p + " narrow"
                    equal = same_bits(ans[wide], ans[narrow])
                    text += "  %s: wide - narrow %.2f vs wide's spread %.2f (x%.2f) bit-equal %s" % (
                        p, med[wide] - med[narrow], max(ms[wide]) - min(ms[wide]), med[wide] / med[narrow], equal)
                    assert equal, text
                say(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
