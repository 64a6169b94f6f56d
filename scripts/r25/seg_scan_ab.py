"""Round 25: the streaming segment scan against the launches it replaces, in one process.

The five request shapes of scripts/r06/seg_ragged_probe.py at the headline's size (16,384,000 ids, 1,638,400 segments,
256 columns), plus the same with a violation in the middle (level 2: the capped fix-up has work), each timed as a whole
aggregate call (HIP events on the current stream, median of 7 behind a warm-up call) with glx_tune("seg_scan_parent", 1)
and 0 in six alternations.  Prints per shape and setting the median of the six medians and their range, and the embeddings'
equality between the two settings.  A second table sweeps glx_tune("seg_scan_wgs", cap) on the dense shape.

usage: python scripts/r25/seg_scan_ab.py [alternations]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import glx  # noqa: E402
import synth  # noqa: E402

ALTS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
dev = torch.device("cuda", 0)
V, D, Sg, f = 10_000_000, 256, 1_638_400, 10
n = Sg * f
feats = glx.Features(synth.features_torch(V, D, 5, dev))
gen = torch.Generator(device=dev)
gen.manual_seed(1)
ids = torch.randint(0, V, (n,), generator=gen, device=dev)
dense = (torch.arange(n, device=dev) // f).to(torch.int32)
ragged_div = torch.sort(torch.randint(0, Sg, (n,), generator=gen, device=dev)).values.to(torch.int32)
ragged = ragged_div[: n - 3].contiguous()
swapped = dense.clone()
swapped[f - 1] = 1
violation = dense.clone()
violation[n // 2] = 0
emb = torch.empty((Sg, D), dtype=torch.float32, device=dev)
cnt = torch.empty(Sg, dtype=torch.int32, device=dev)
SHAPES = (("none", None, n), ("dense", dense, n), ("swapped", swapped, n), ("ragged_div", ragged_div, n),
          ("ragged", ragged, n - 3), ("violation", violation, n))


def timed(seg, m):
    r = []
    for _ in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        feats.aggregate("SumAggregator", ids[:m], seg, Sg, out=(emb, cnt))
        b.record()
        torch.cuda.synchronize()
        r.append(a.elapsed_time(b))
    return float(np.median(r[1:]))


def say(s):
    print(s, flush=True)


say("# whole aggregate call, ms: median of %d alternations (min .. max); V = %d, D = %d, %d ids, %d segments" % (ALTS, V, D, n, Sg))
say("# shape  seg_scan_parent=1  seg_scan_parent=0  difference  outputs equal")
for name, seg, m in SHAPES:
    got = {0: [], 1: []}
    keep = {}
    for alt in range(ALTS):
        for parent in ((1, 0) if alt % 2 == 0 else (0, 1)):
            glx.tune("seg_scan_parent", parent)
            got[parent].append(timed(seg, m))
            if alt == 0:
                keep[parent] = (emb.clone(), cnt.clone())
    same = torch.equal(keep[0][0], keep[1][0]) and torch.equal(keep[0][1], keep[1][1])
    med = {k: float(np.median(v)) for k, v in got.items()}
    say("%-11s %.4f (%.4f .. %.4f)  %.4f (%.4f .. %.4f)  %+.4f  %s" % (
        name, med[1], min(got[1]), max(got[1]), med[0], min(got[0]), max(got[0]), med[0] - med[1], same))
glx.tune("seg_scan_parent", 0)
say("# dense, seg_scan_wgs = cap on the scan's workgroups (0 = the default grid)")
for cap in (0, 256, 512, 1024, 1280, 1536, 2048):
    glx.tune("seg_scan_wgs", cap)
    t = [timed(dense, n) for _ in range(3)]
    say("wgs %-5d %.4f (%.4f .. %.4f)" % (cap, float(np.median(t)), min(t), max(t)))
glx.tune("seg_scan_wgs", 0)
