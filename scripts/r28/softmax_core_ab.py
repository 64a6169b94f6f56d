"""Parent against result for the softmax core under glx_segment_softmax, glx_gat_attention and glx_dot_attention: the
same bits, and the same speed.  Every figure comes from a fresh child process whose GLX_LIB names the library; each
child runs under its own time limit, and the first one that fails ends the run.

    python scripts/r28/softmax_core_ab.py build-parent [REV]   libglx.so of REV (default HEAD~1) into build/parent/
    python scripts/r28/softmax_core_ab.py bits                 > profiles/r28/softmax_core_bits.txt
    python scripts/r28/softmax_core_ab.py speed                > profiles/r28/softmax_core_speed.txt

bits   the requests that the three GPU test files build (_lengths_request for heads 1, 2, 3, 4, 6, 8, pad 0 and 10,000,
       cut and uncut, drop_p 0 and 0.1; the dot test's lengths_request for its dim / heads grid, with and without
       edge, aligned (float4 where the shape allows) and one float off) through all six entry points, one checksum of
       the bits of every output.  The parent's list and the result's must be identical; both are printed.
speed  forward and backward of the three operators on C3-like segments of 10 at heads 4, with and without dropout,
       and on segments of 4,000 positions (the workgroup walk; in the dot kernel the group's spill loop): medians of 10
       HIP-event timings after 2 warm-ups.  Children: parent1 result1 .. parent5 result5, then parent against parent
       aa1a aa1b .. aa5a aa5b.  spread = the largest |a - b| of the five parent-against-parent pairs; a call passes
       when the result's five figures lie inside [min(parent) - spread, max(parent) + spread]."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "graph-learn_amd")
PARENT = os.path.join(ROOT, "build", "parent")
LIBS = {"parent": os.path.join(PARENT, "graph-learn_amd", "lib", "libglx.so"),
        "result": os.path.join(PKG, "lib", "libglx.so")}
CHILD_LIMIT = 240  # seconds; a child needs 10 .. 40
WARMUP, REPS = 2, 10


def build_parent(rev):
    os.makedirs(PARENT, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "graph-learn_amd/csrc", "graph-learn_amd/Makefile", "include"],
                         stdout=subprocess.PIPE, check=True).stdout
    subprocess.run(["tar", "-x", "-C", PARENT], input=tar, check=True)
    subprocess.run(["make", "-j16", "-C", os.path.join(PARENT, "graph-learn_amd"), LIBS["parent"]], check=True)


def child(mode, side):
    """the stdout lines of one fresh process on the library of `side`; any failure ends the run"""
    env = dict(os.environ, GLX_LIB=LIBS[side])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child-" + mode], env=env, stdout=subprocess.PIPE,
                       text=True, timeout=CHILD_LIMIT)
    if r.returncode != 0:
        sys.exit("the %s child on %s ended with status %d: nothing further is started" % (mode, side, r.returncode))
    return r.stdout.splitlines()


def _imports():
    for p in (os.path.join(ROOT, "tests"), os.path.join(PKG, "python"), PKG):
        sys.path.insert(0, p)


# ---- bits -----------------------------------------------------------------------------------------------------------
def child_bits():
    _imports()
    import numpy as np
    import test_gpu_dot_attention as tdot
    import test_gpu_gat_attention as tgat
    import test_gpu_segment_softmax as tsm

    def show(case, names, outs):
        for name, a in zip(names, outs):
            if a is not None:
                print("%-44s %-9s %s" % (case, name, hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]))

    for heads in tsm.HEADS:
        for pad in (0, 10000):
            for cut in (False, True):
                case = "heads %d pad %d %s" % (heads, pad, "cut" if cut else "uncut")
                e, cnt, g = tsm._lengths_request(heads, pad, cut, seed=heads + pad)
                alpha = tsm.gpu_forward(e, cnt, len(cnt))[0]
                show("softmax " + case, ["alpha", "grad_e"], [alpha, tsm.gpu_backward(alpha, g, cnt, len(cnt))[0]])
                s, t, rows, g, cnt = tgat._lengths_request(heads, pad, cut, seed=heads + pad)
                for p in (0.0, 0.1):
                    kw = dict(drop_p=p, seed=11, call=3)
                    alpha, soft = tgat.gpu_forward(s, t, rows, cnt, **kw)
                    show("gat %s drop %.1f" % (case, p), ["alpha", "soft", "grad_e", "grad_s", "grad_t"],
                         [alpha, soft] + list(tgat.gpu_backward(soft, g, s, t, rows, cnt, **kw)))
    for dim, heads in tdot.SHAPES:
        for with_edge in (False, True):
            for cut in (False, True):
                r = tdot.lengths_request(dim, heads, with_edge, seed=dim + heads, cut=cut)
                for offset in (False, True):
                    for p in (0.0, 0.1):
                        kw = dict(drop_p=p, seed=11, call=3)
                        case = "dot %d/%d %s %s %s drop %.1f" % (dim, heads, "edge" if with_edge else "plain",
                                                                "cut" if cut else "uncut", "off" if offset else "al", p)
                        out, soft, logit = tdot.gpu_forward(r, offset=offset, **kw)
                        show(case, ["out", "soft", "logit", "grad_e", "grad_q", "grad_k", "grad_v", "grad_edge"],
                             [out, soft, logit] + list(tdot.gpu_backward(r, soft, offset=offset, **kw)))


def run_bits():
    lists = {}
    for side in ("parent", "result"):
        lists[side] = child("bits", side)
        with open(LIBS[side], "rb") as f:
            print("%s (libglx.so %s): %d checksums" % (side, hashlib.sha1(f.read()).hexdigest()[:16], len(lists[side])))
        print("\n".join("  " + x for x in lists[side]))
    differ = [a for a, b in zip(lists["parent"], lists["result"]) if a != b]
    same = len(lists["parent"]) == len(lists["result"]) and not differ and len(lists["parent"]) > 0
    print("the two lists are identical: %s" % ("yes" if same else "NO\n" + "\n".join(differ)))
    return 0 if same else 1


# ---- speed ----------------------------------------------------------------------------------------------------------
def child_speed():
    _imports()
    import torch
    import glx
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    H, D, M = 4, 256, 1 << 20
    n = 65536 * 25 * 10
    calls = {}

    def add(tag, length):  # a function: every closure keeps the buffers of its own request
        S = n // length
        cnt = torch.full((S,), length, dtype=torch.int32, device=dev)
        rows = torch.randint(0, M, (n,), device=dev, generator=gen)
        e = torch.randn(n, H, device=dev, generator=gen) * 3
        g = torch.randn(n, H, device=dev, generator=gen)
        out, out2 = torch.empty_like(e), torch.empty_like(e)
        alpha = glx.segment_softmax(e, S, cnt=cnt).clone()
        calls["sm_fwd_" + tag] = lambda e=e, S=S, cnt=cnt: glx.segment_softmax(e, S, cnt=cnt, out=out)
        calls["sm_bwd_" + tag] = lambda a=alpha, g=g, S=S, cnt=cnt: glx.segment_softmax_backward(a, g, cnt, S, out=out)
        s = torch.randn(S, H, device=dev, generator=gen) * 2
        t = torch.randn(M, H, device=dev, generator=gen) * 2
        out_s, out_t = torch.empty_like(s), torch.empty_like(t)
        q = torch.randn(S, D, device=dev, generator=gen) * 0.25
        k = torch.randn(M, D, device=dev, generator=gen) * 0.25
        v = torch.randn(M, D, device=dev, generator=gen) * 0.25
        go = torch.randn(S, D, device=dev, generator=gen)
        oq, ok, ov, oo = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(q)
        for p in ((0.0, 0.4) if tag == "c3" else (0.0,)):
            kw = dict(drop_p=p, seed=11, call=3)
            soft = glx.gat_attention(s, t, rows, cnt=cnt, **kw)[1].clone()
            name = "%s_p%d" % (tag, round(p * 10))
            calls["gat_fwd_" + name] = lambda s=s, t=t, rows=rows, cnt=cnt, kw=kw: glx.gat_attention(
                s, t, rows, cnt=cnt, out=out, soft_out=out2, **kw)
            calls["gat_bwd_" + name] = lambda soft=soft, g=g, s=s, t=t, rows=rows, cnt=cnt, kw=kw: \
                glx.gat_attention_backward(soft, g, s, t, rows, cnt=cnt, out=out, out_s=out_s, out_t=out_t, **kw)
        for p in ((0.0, 0.1) if tag == "c3" else (0.0,)):
            kw = dict(heads=H, drop_p=p, seed=11, call=3)
            soft = glx.dot_attention(q, k, v, rows, cnt=cnt, **kw)[1].clone()
            name = "%s_p%d" % (tag, round(p * 10))
            calls["dot_fwd_" + name] = lambda q=q, k=k, v=v, rows=rows, cnt=cnt, kw=kw, oo=oo: glx.dot_attention(
                q, k, v, rows, cnt=cnt, out=oo, soft_out=out, **kw)
            calls["dot_bwd_" + name] = lambda soft=soft, go=go, q=q, k=k, v=v, rows=rows, cnt=cnt, kw=kw, oq=oq, ok=ok, \
                ov=ov: glx.dot_attention_backward(soft, go, q, k, v, rows, cnt=cnt, out=out2, out_q=oq, out_k=ok, out_v=ov,
                                                  **kw)

    add("c3", 10)
    add("long", 4000)
    res = {}
    for name, fn in calls.items():
        ts = []
        for rep in range(WARMUP + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        res[name] = sorted(ts[WARMUP:])[REPS // 2]
    print(json.dumps(res))


def run_speed():
    def one(side):
        return json.loads(child("speed", side)[-1])

    ab = [(one("parent"), one("result")) for _ in range(5)]
    aa = [(one("parent"), one("parent")) for _ in range(5)]
    print(__doc__.split("\nspeed  ", 1)[1].replace("\n       ", "\n").strip())
    print("One MI355X, one session.  ratio = median(result) / median(parent).  All times in ms.\n")
    worst, failed = ("", 0.0), []
    for name in ab[0][0]:
        par, res = [p[name] for p, _ in ab], [r[name] for _, r in ab]
        spread = max(abs(a[name] - b[name]) for a, b in aa)
        lo, hi = min(par) - spread, max(par) + spread
        ratio = sorted(res)[2] / sorted(par)[2]
        ok = all(lo <= x <= hi for x in res)
        verdict = "pass" if ok else "OUTSIDE, slower" if max(res) > hi else "OUTSIDE, faster"
        print(name)
        print("  parent  " + " ".join("%10.3f" % x for x in par))
        print("  result  " + " ".join("%10.3f" % x for x in res))
        print("  A/A     " + " ".join("%9.3f/%-9.3f" % (a[name], b[name]) for a, b in aa))
        print("  spread %.3f  allowed [%.3f, %.3f]  ratio %.4f  %s" % (spread, lo, hi, ratio, verdict))
        if ratio > worst[1]:
            worst = (name, ratio)
        if not ok:
            failed.append("%s (%s)" % (name, verdict.split(", ")[1]))
    print("\nworst ratio: %s %.4f" % worst)
    print("calls outside their band: %s" % (", ".join(failed) if failed else "none"))
    return 1 if failed else 0


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "build-parent":
        build_parent(sys.argv[2] if len(sys.argv) > 2 else "HEAD~1")
    elif cmd == "child-bits":
        child_bits()
    elif cmd == "child-speed":
        child_speed()
    elif cmd in ("bits", "speed"):
        sys.exit(run_bits() if cmd == "bits" else run_speed())
    else:
        sys.exit(__doc__)
