"""Driver of l2_stripe_sim.cc: build it (g++, into build/), and simulate the per-XCD L2 line fetches of the grouped
reduce over a hop-2 id stream under today's mapping, the XCD-stripe mapping and the sorted-by-hop-1 order.

  python scripts/l2_stripe_sim.py HOP2_IDS [--hop1 HOP1_IDS] [--fanout 10] [--dim 256] [--rows 10000000]

Id files: .npy (int32 / int64) or .u24 (raw 24-bit little-endian ids).  With --hop1 (one hop-1 vertex per hop-2
segment) the sorted-by-hop-1 order is simulated too."""
import argparse, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(os.path.dirname(HERE), "build")


def build():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "l2_stripe_sim")
    src = os.path.join(HERE, "l2_stripe_sim.cc")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, src])
    return exe


def load_ids(path):
    if path.endswith(".u24"):
        b = np.fromfile(path, np.uint8).reshape(-1, 3).astype(np.int32)
        return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.load(path)


def run(ids, mappings, fanout, dim, rows, order=None, resident=None):
    exe = build()
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "ids.npy")
        np.save(p, np.ascontiguousarray(ids, dtype=np.int32 if ids.max(initial=0) < 2**31 else np.int64))
        maps = list(mappings)
        if order is not None:
            q = os.path.join(tmp, "order.npy")
            np.save(q, np.ascontiguousarray(order, dtype=np.int32))
            maps = [m.replace("@ORDER", q) for m in maps]
        extra = ["resident=%d" % resident] if resident else []
        return subprocess.run([exe, p, str(fanout), str(dim), str(rows)] + maps + extra, check=True,
                              stdout=subprocess.PIPE, text=True).stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("hop2")
    ap.add_argument("--hop1")
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--resident", type=int, default=0)
    args = ap.parse_args()
    ids = load_ids(args.hop2)
    maps = ["rr:1", "rr:2", "rr:4"]
    for n in (1, 2, 4):
        maps += ["stripe:%d:%d" % (n, c) for c in (4, 16, 64, 256)]
    order = None
    if args.hop1:
        h1 = load_ids(args.hop1)
        order = np.argsort(h1, kind="stable")
        maps += ["perm:1:@ORDER", "perm:2:@ORDER"]
    sys.stdout.write(run(ids, maps, args.fanout, args.dim, args.rows, order, args.resident or None))


if __name__ == "__main__":
    main()
