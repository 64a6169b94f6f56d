"""The chunked order of pair_dot's backward (K5-dot-chunked) and of gat_attention's grad_t (K5-gat-chunked) against the
default ascending order, at engine level (glx.pair_dot_backward / glx.gat_attention_backward with chunked=False / True).

pair_dot backward, both sides, float32 and bfloat16 tables, dim 256, heads 1:
  (a) examples/train_sage_unsup.py's stream at C3 size: 65,536 source vertices of the RMAT 10 M / 100 M graph, K = 5
      negatives each from glx.Negative.from_graph(g, by_in_degree=True), rows deduplicated by glx.unique
  (b) the same pairs with every candidate-side run capped at 256 (entries past the 256th of a row moved to rows drawn
      uniformly): no long run, so the chunked order adds its directory and its idle launches only
  (c) synthetic: 262,140 pairs over 100,000 rows, one row holds half of them (K = 1 for side 1; the same index as the
      source side with K = 5 gives side 0 runs five times as long)
grad_t, heads 1 and 4: the FullSampler hop over 65,536 RMAT seeds of scripts/r18/gat_attention_probe.py.

One process on one MI355X, the two orders interleaved (their order alternating), device events around the whole engine
call, medians of 10 after 3 warm-ups.  Equal bits between the legs are asserted wherever the contract says so.  CHECK
lines compare with the default leg of the same run: on (b) whether the chunked median lies within the default's own
min .. max, on (c) whether it is faster; on (a) and on grad_t nothing is promised.  Not a requirement of the suite.
Usage: timeout 900 python scripts/pair_dot_chunked_probe.py [nodes] [edges] [batch] > profiles/pair_dot_chunked/probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402
from chunked_grad_probe import CHUNK, HUB_N, HUB_ROWS, MODES, capped, measure  # noqa: E402

D, K = 256, 5


def describe(name, own, rep, M):
    runs = torch.bincount(own[(own >= 0) & (own < M)], minlength=M) * rep
    long_runs = runs > CHUNK
    print("  %s: %d runs above %d pairs, the longest %d, holding %.4f of the %d pairs" % (
        name, int(long_runs.sum()), CHUNK, int(runs.max()), float(runs[long_runs].sum()) / (own.numel() * rep),
        own.numel() * rep), flush=True)
    return runs


def pair_stream(stream, label, ia, ib, repeat, M, gen, verdicts):
    n, dev = int(ib.numel()), ib.device
    print("\nstream %s: %d pairs, repeat %d, over %d rows" % (label, n, repeat, M), flush=True)
    g = torch.randn(n, 1, device=dev, generator=gen)
    z32 = torch.randn(M, D, device=dev, generator=gen)
    for side in (0, 1):
        runs = describe("side %d" % side, ia if side == 0 else ib, repeat if side == 0 else 1, M)
        for z in (z32, z32.bfloat16()):
            outs = {m: torch.empty_like(z) for m in MODES}
            calls = {m: (lambda out, m=m: glx.pair_dot_backward(side, ia, ib, g, z, M, repeat=repeat, out=out, chunked=m))
                     for m in MODES}
            res = measure(calls, outs)
            short = runs <= CHUNK
            assert torch.equal(outs[False][short], outs[True][short]), "short runs must keep the default bits"
            tag = "side %d, %s" % (side, str(z.dtype).replace("torch.", ""))
            for m in MODES:
                print("  %-22s %-8s median %8.3f ms (min %8.3f max %8.3f)" % ((tag, "chunked" if m else "default") + res[m]),
                      flush=True)
            d, c = res[False], res[True]
            print("  %-22s chunked / default: %.3f" % (tag, c[0] / d[0]), flush=True)
            if stream == "b":
                verdicts.append(("(b) %s: chunked median %.3f ms within the default's min .. max [%.3f, %.3f]"
                                 % (tag, c[0], d[1], d[2]), d[1] <= c[0] <= d[2]))
            elif stream == "c":
                verdicts.append(("(c) %s: chunked median %.3f ms below the default's %.3f ms" % (tag, c[0], d[0]), c[0] < d[0]))
            del outs
    torch.cuda.empty_cache()


def grad_t_stream(seed_local, local, deg, M, gen, verdicts):
    n, S, dev = int(local.numel()), int(deg.numel()), local.device
    lists = torch.bincount(local, minlength=M)
    print("\ngrad_t on the FullSampler hop: %d positions in %d segments over %d rows; rows named above %d times: %d, the "
          "most %d" % (n, S, M, CHUNK, int((lists > CHUNK).sum()), int(lists.max())), flush=True)
    for heads in (1, 4):
        s = torch.randn(S, heads, device=dev, generator=gen)
        t = torch.randn(M, heads, device=dev, generator=gen)
        ga = torch.randn(n, heads, device=dev, generator=gen)
        _, soft = glx.gat_attention(s, t, local, cnt=deg)
        outs = {m: tuple(torch.empty(k, heads, device=dev) for k in (n, S, M)) for m in MODES}
        calls = {m: (lambda o, m=m: glx.gat_attention_backward(soft, ga, s, t, local, cnt=deg, out=o[0], out_s=o[1],
                                                                out_t=o[2], chunked=m)) for m in MODES}
        res = measure(calls, outs)
        assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])
        assert torch.equal(outs[False][2][lists <= CHUNK], outs[True][2][lists <= CHUNK])
        for m in MODES:
            print("  heads %d %-8s whole backward median %8.3f ms (min %8.3f max %8.3f)"
                  % ((heads, "chunked" if m else "default") + res[m]), flush=True)
        print("  heads %d chunked / default: %.3f" % (heads, res[True][0] / res[False][0]), flush=True)
        del outs


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    dev = torch.device("cuda", 0)
    print("device: %s   graph: RMAT %d vertices / %d edges   %d sources   K %d   dim %d   chunk %d"
          % (torch.cuda.get_device_name(0), V, E, B, K, D, CHUNK), flush=True)
    src, dst, _ = synth.rmat_edges_torch(V, E, 1, dev, weighted=False)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, sort_by_weight=False)
    del src, dst
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    verdicts = []

    neg = glx.Negative.from_graph(g, by_in_degree=True).sample(seeds, K, seed=42, call_counter=0)
    nodes, (l_src, l_neg), _ = glx.unique([seeds, neg])
    M = int(nodes.numel())
    l_src, l_neg = l_src.reshape(-1).contiguous(), l_neg.reshape(-1).contiguous()
    pair_stream("a", "(a) in-degree negatives, deduplicated", l_src, l_neg, K, M, gen, verdicts)
    pair_stream("b", "(b) the same, candidate runs capped at %d" % CHUNK, l_src, capped(l_neg, M, gen), K, M, gen, verdicts)
    hub = torch.randint(0, HUB_ROWS, (HUB_N,), device=dev, generator=gen)
    hub[torch.randperm(HUB_N, device=dev, generator=gen)[:HUB_N // 2]] = HUB_ROWS // 2
    pair_stream("c", "(c) synthetic, one row holds half the pairs", hub[:HUB_N // K].contiguous(),
                hub[:HUB_N // K * K].contiguous(), K, HUB_ROWS, gen, verdicts)

    deg, nbr, _ = g.sample_full(seeds, 0)
    nodes, (local0, local), _ = glx.unique([seeds, nbr])
    M = int(nodes.numel())
    del g, nbr, nodes
    torch.cuda.empty_cache()
    grad_t_stream(local0, local.reshape(-1).contiguous(), deg, M, gen, verdicts)

    print("\nchecks against the default leg of this run:", flush=True)
    for text, ok in verdicts:
        print("  CHECK %s: %s" % ("holds" if ok else "DOES NOT HOLD", text), flush=True)


if __name__ == "__main__":
    main()
