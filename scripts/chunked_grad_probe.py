"""The chunked order of the row gradients (K5-bwd-chunked) against the default ascending-position order, at engine level
(glx.aggregate_backward / glx.aggregate_weighted_backward_x with chunked=False / True), dim = 256, on three streams:

  (a) hop 2 of a real C3 step (RMAT 10 M / 100 M, EdgeWeight [25, 10], 65,536 seeds), deduplicated (glx.unique):
      16.4 M positions into 1.64 M segments of 10 over the distinct nodes
  (b) the same positions with every list capped at 256 entries: the entries of a list from the 257th on are moved to
      rows drawn uniformly, until no list exceeds 256 -- no long row, so the chunked mode adds its directory pass only
  (c) synthetic: 262,140 positions over 100,000 rows, one row takes half of them, the rest are uniform (kept this
      small because the default mode gives the hub's 131,070 entries to one lane group: tens of milliseconds a call)

for Mean, Max and the weighted Sum at heads 1 and 4, each with a float32 and a bfloat16 grad_x.  One process, the two
modes interleaved (their order alternating), 3 warm-up + 10 timed repetitions, device events around the whole call,
medians with min and max.  The transpose is reported apart: the same call at dim = 1 is the stable sort, the row
offsets and (chunked) the directory, with a reduce that moves almost nothing; `reduce` is the dim-256 median minus it.
Read the default mode's dim-1 figure with care: its reduce still walks the longest list with ONE lane group, entry by
entry, so on a stream with a hub it is that walk's latency and not the sort -- the sort and the offsets alone are what
stream (b) and the chunked mode show at dim 1.

Three statements are checked against the DEFAULT mode of the same run and printed as CHECK lines: on (b) the chunked
median lies within the default's own min .. max; on (c) the chunked mode is faster; on (a) nothing is promised.
Nothing here is a requirement of the test suite.
Usage: python scripts/chunked_grad_probe.py [nodes] [edges] [batch] > profiles/chunked_grad/probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402

WARMUP, REPS = 3, 10
FANOUTS = [25, 10]
D, CHUNK = 256, glx.COALESCE_CHUNK
MODES = (False, True)
HUB_N, HUB_ROWS = 262_140, 100_000  # stream (c): the default mode walks the hub's 131,070 entries with ONE lane group


def median(v):
    return sorted(v)[len(v) // 2]


def list_ranks(index):
    """for every position its rank in its row's list (ascending position), and the list lengths"""
    order = torch.sort(index, stable=True).indices
    srt = index[order]
    first = torch.searchsorted(srt, srt, right=False)
    rank = torch.empty_like(index)
    rank[order] = torch.arange(index.numel(), device=index.device) - first
    return rank


def capped(index, M, gen):
    """stream (b): no list longer than CHUNK"""
    index = index.clone()
    for _ in range(20):
        over = list_ranks(index) >= CHUNK
        k = int(over.sum())
        if k == 0:
            return index
        index[over] = torch.randint(0, M, (k,), device=index.device, generator=gen)
    raise RuntimeError("could not cap the lists")


def describe(name, index, M):
    lengths = torch.bincount(index, minlength=M)
    long_rows = lengths > CHUNK
    share = float(lengths[long_rows].sum()) / index.numel()
    chunks = int(((lengths[long_rows] + CHUNK - 1) // CHUNK).sum())
    print("\nstream %s: %d positions over %d rows; longest list %d; rows above %d entries: %d, holding %.4f of the "
          "positions in %d chunks" % (name, index.numel(), M, int(lengths.max()), CHUNK, int(long_rows.sum()), share,
                                      chunks), flush=True)


def timed(call, out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    call(out)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def measure(calls, outs):
    """calls[mode](out): medians, mins and maxs per mode, the modes interleaved and their order alternating"""
    times = {m: [] for m in MODES}
    for rep in range(WARMUP + REPS):
        for m in (MODES if rep % 2 == 0 else MODES[::-1]):
            t = timed(calls[m], outs[m])
            if rep >= WARMUP:
                times[m].append(t)
    return {m: (median(times[m]), min(times[m]), max(times[m])) for m in MODES}


def probe(stream, name, make_call, index, M, S, gen, verdicts):
    """make_call(dim, grad_out, chunked) -> call(out); one line per (grad_x dtype, mode)"""
    go = {D: torch.randn(S, D, device=index.device, generator=gen), 1: torch.randn(S, 1, device=index.device, generator=gen)}
    for dtype in (torch.float32, torch.bfloat16):
        res = {}
        for dim in (D, 1):
            outs = {m: torch.empty(M, dim, dtype=dtype, device=index.device) for m in MODES}
            calls = {m: make_call(dim, go[dim], m) for m in MODES}
            res[dim] = measure(calls, outs)
            if dim == D and dtype == torch.float32:  # the two orders agree wherever a list has at most one chunk
                short = torch.bincount(index, minlength=M) <= CHUNK
                same = bool(torch.equal(outs[False][short].view(torch.int32), outs[True][short].view(torch.int32)))
                print("  %s: rows of at most %d entries get the default bits: %s" % (name, CHUNK, same), flush=True)
            del outs, calls
        tag = "%s, grad_x %s" % (name, str(dtype).replace("torch.", ""))
        for m in MODES:
            whole, tr = res[D][m], res[1][m]
            print("  %-34s %-8s whole median %8.3f ms (min %8.3f max %8.3f)   transpose (dim 1) %7.3f ms   "
                  "reduce (whole - transpose) %8.3f ms" % (tag, "chunked" if m else "default", whole[0], whole[1],
                                                          whole[2], tr[0], whole[0] - tr[0]), flush=True)
        d, c = res[D][False], res[D][True]
        print("  %-34s chunked / default: whole %.3f" % (tag, c[0] / d[0]), flush=True)
        if stream == "b":
            verdicts.append(("(b) %s: chunked median %.3f ms within the default's min .. max [%.3f, %.3f]"
                             % (tag, c[0], d[1], d[2]), d[1] <= c[0] <= d[2]))
        elif stream == "c":
            verdicts.append(("(c) %s: chunked median %.3f ms below the default's %.3f ms" % (tag, c[0], d[0]), c[0] < d[0]))
    del go
    torch.cuda.empty_cache()


def run_stream(stream, label, index, M, S, f, gen, verdicts):
    describe(label, index, M)
    n, dev = int(index.numel()), index.device
    for op_name, op in (("mean", glx.MEAN), ("max", glx.MAX)):
        arg = {}
        if op == glx.MAX:  # any position of the segment is a valid argument
            for dim in (D, 1):
                arg[dim] = (torch.arange(S, device=dev, dtype=torch.int32)[:, None] * f +
                            torch.randint(0, f, (S, dim), device=dev, generator=gen, dtype=torch.int32)).contiguous()
        probe(stream, "aggregate_backward %s" % op_name,
              lambda dim, go, m, o=op, a=arg: (lambda out: glx.aggregate_backward(o, index, None, go, M, arg=a.get(dim),
                                                                                 out=out, chunked=m)),
              index, M, S, gen, verdicts)
        del arg
    for heads in (1, 4):
        wts = torch.softmax(torch.randn(S, f, heads, device=dev, generator=gen), dim=1).reshape(n, heads).contiguous()
        w1 = wts[:, :1].contiguous()  # dim 1 has one head
        probe(stream, "weighted_backward_x sum, heads %d" % heads,
              lambda dim, go, m, wt=wts, w_1=w1: (lambda out: glx.aggregate_weighted_backward_x(
                  glx.SUM, index, wt if dim == D else w_1, None, go, M, out=out, chunked=m)),
              index, M, S, gen, verdicts)
        del wts, w1


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    dev = torch.device("cuda", 0)
    print("device: %s   graph: RMAT %d vertices / %d edges   EdgeWeight %s   %d seeds   dim %d   chunk %d"
          % (torch.cuda.get_device_name(0), V, E, FANOUTS, B, D, CHUNK), flush=True)
    src, dst, w = synth.rmat_edges_torch(V, E, 1, dev, weighted=True)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, w)
    del src, dst, w
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    hops = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, FANOUTS, seed=42, call_counter=0)
    nodes, inverse, _ = glx.unique([seeds, hops[0][0], hops[1][0]])
    index = inverse[2].reshape(-1).contiguous()
    n, M, f = int(index.numel()), int(nodes.shape[0]), FANOUTS[1]
    S = n // f
    del g, hops, nodes, inverse
    torch.cuda.empty_cache()
    print("hop 2: %d positions into %d segments of %d over %d distinct nodes" % (n, S, f, M), flush=True)
    print("modes: default = ascending request position, one lane group per row; chunked = chunks of %d list entries, "
          "one lane group per chunk of a long row, partial sums added in chunk order" % CHUNK, flush=True)
    verdicts = []
    run_stream("a", "(a) C3 hop 2, deduplicated", index, M, S, f, gen, verdicts)
    run_stream("b", "(b) the same, lists capped at %d" % CHUNK, capped(index, M, gen), M, S, f, gen, verdicts)
    hub = torch.randint(0, HUB_ROWS, (HUB_N,), device=dev, generator=gen)
    hub[torch.randperm(HUB_N, device=dev, generator=gen)[:HUB_N // 2]] = HUB_ROWS // 2
    run_stream("c", "(c) synthetic, one row holds half the positions", hub, HUB_ROWS, HUB_N // f, f, gen, verdicts)
    print("\nchecks against the default mode of this run:", flush=True)
    for text, ok in verdicts:
        print("  CHECK %s: %s" % ("holds" if ok else "DOES NOT HOLD", text), flush=True)


if __name__ == "__main__":
    main()
