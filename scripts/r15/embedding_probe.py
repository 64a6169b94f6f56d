"""Trainable embedding tables at the headline graph's size: a 10 M x 128 float32 table, one node2vec-sized batch of
4,096 walks x 20 positions plus 10 negatives per position (901,120 ids; walk positions uniform over the table, negatives
skewed towards low ids the way in-degree negatives are).

  1. lookup + backward + Adam step through SparseEmbedding / SparseAdam against torch.nn.Embedding(sparse=True) +
     torch.optim.SparseAdam on the same ids and the same output gradient, in the same process, legs interleaved;
  2. glx_rows_coalesce and glx_embedding_update (Adam) apart, each with the bytes it must move;
  3. the categorical case: 1.9 M positions over 1,000 Zipf-distributed values at D = 16 and D = 64 -- the longest list's
     length and the coalesce time (chunks of GLX_COALESCE_CHUNK entries, partial sums added in order);
  4. one coalesce request at num_rows = 10^4 and at num_rows = 2 * 10^9: nothing may scale with the table (the radix
     sort runs over the bits num_rows needs, so the second sorts 31 bits where the first sorts 14).

The parent of this change has no such entry point, so torch is the only baseline.  One process, HIP events, 3 warm-up +
10 timed repetitions, medians.  Nothing here is a requirement of the test suite.
Usage: python scripts/r15/embedding_probe.py [rows] > profiles/r15/embedding.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
from graphlearn.nn.pytorch import SparseAdam, SparseEmbedding  # noqa: E402

WARMUP, REPS = 3, 10
D = 128
WALKS, WALK_LEN, NEGATIVES = 4096, 20, 10


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
    return {k: sorted(v) for k, v in times.items()}


def show(name, ts):
    med = ts[len(ts) // 2]
    print("  %-66s median %9.3f ms  min %9.3f  max %9.3f" % (name, med, ts[0], ts[-1]), flush=True)
    return med


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    pos = WALKS * WALK_LEN
    walk_ids = torch.randint(0, V, (pos,), device=dev, generator=gen)
    neg_ids = (torch.rand(pos * NEGATIVES, device=dev, generator=gen).double() ** 3 * V).long().clamp_(0, V - 1)
    ids = torch.cat([walk_ids, neg_ids]).contiguous()
    n = int(ids.numel())
    grad_out = torch.randn(n, D, device=dev, generator=gen)
    print("device: %s   table: %d x %d float32 (%.2f GB)   %d ids (%d walk positions + %d negatives), %d distinct"
          % (torch.cuda.get_device_name(0), V, D, V * D * 4 / 1e9, n, pos, pos * NEGATIVES,
             int(torch.unique(ids).numel())), flush=True)

    emb = SparseEmbedding(V, D, seed=1)
    opt = SparseAdam(emb, lr=0.01)
    ref = torch.nn.Embedding(V, D, sparse=True, device=dev)
    with torch.no_grad():
        ref.weight.copy_(emb.weight)
    ref_opt = torch.optim.SparseAdam(ref.parameters(), lr=0.01)

    def engine():
        emb(ids).backward(grad_out)
        opt.step()

    def plain():
        ref_opt.zero_grad(set_to_none=True)
        ref(ids).backward(grad_out)
        ref_opt.step()

    print("\n[1] lookup + backward + Adam step, %d ids" % n, flush=True)
    t = timed({"engine": engine, "torch": plain})
    e_ms = show("SparseEmbedding + SparseAdam (gather, coalesce, fused update)", t["engine"])
    t_ms = show("nn.Embedding(sparse=True) + torch.optim.SparseAdam", t["torch"])
    print("  torch / engine: %.2f" % (t_ms / e_ms), flush=True)
    steps = WARMUP + REPS
    diff = float((emb.weight - ref.weight.detach()).abs().max())
    print("  largest |engine - torch| over the table after %d steps each: %.3e" % (steps, diff), flush=True)
    for name, fn in (("engine", engine), ("torch", plain)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        print("  %-6s peak memory above what the leg keeps: %7.3f GB" % (name, (torch.cuda.max_memory_allocated() - base) / 1e9),
              flush=True)
    del ref, ref_opt
    torch.cuda.empty_cache()

    print("\n[2] the entry points apart", flush=True)
    urows, ug, count = glx.rows_coalesce(ids, grad_out, V)
    U = int(count)
    m, v = opt.state[0]["state1"], opt.state[0]["state2"]
    t = timed({
        "coalesce": lambda: glx.rows_coalesce(ids, grad_out, V, out_rows=urows, out_g=ug),
        "update": lambda: glx.embedding_update(glx.EMB_ADAM, emb.weight, urows, ug, state1=m, state2=v, alpha=1e-3, eps=1e-8,
                                               beta1=0.9, c1=0.1, beta2=0.999, c2=0.001),
    })
    row = D * 4
    for key, name, nbytes in (
            ("coalesce", "glx_rows_coalesce (%d positions -> %d rows)" % (n, U), n * (8 + row) + U * (8 + row)),
            ("update", "glx_embedding_update, Adam (%d entries, %d in the table)" % (n, U), n * 8 + U * (row + 6 * row))):
        ms = show(name, t[key])
        print("    at least %.3f GB by the shapes -> %.1f GB/s" % (nbytes / 1e9, nbytes / max(ms, 1e-6) / 1e6), flush=True)
    del emb, opt, m, v, urows, ug
    torch.cuda.empty_cache()

    print("\n[3] categorical columns: 1.9 M positions over 1,000 Zipf-distributed values", flush=True)
    npos, values = 1_900_000, 1000
    weights = 1.0 / torch.arange(1, values + 1, device=dev, dtype=torch.float64)
    cat = torch.multinomial(weights, npos, replacement=True, generator=gen).contiguous()
    longest = int(torch.bincount(cat, minlength=values).max())
    for d in (16, 64):
        g = torch.randn(npos, d, device=dev, generator=gen)
        t = timed({"coalesce": lambda: glx.rows_coalesce(cat, g, values)})
        ms = show("glx_rows_coalesce D = %d (longest list %d = %d chunks)"
                  % (d, longest, -(-longest // glx.COALESCE_CHUNK)), t["coalesce"])
        nbytes = npos * (8 + d * 4)
        print("    at least %.3f GB by the shapes -> %.1f GB/s" % (nbytes / 1e9, nbytes / max(ms, 1e-6) / 1e6), flush=True)
        a = glx.rows_coalesce(cat, g, values)[1][:values].clone()
        b = glx.rows_coalesce(cat, g, values)[1][:values]
        print("    two calls give the same bits: %s" % bool(torch.equal(a.view(torch.int32), b.view(torch.int32))), flush=True)
        del g, a, b

    print("\n[4] one request (%d positions, rows below 10^4, D = %d) against two table sizes" % (n, D), flush=True)
    small = (ids % 10_000).contiguous()
    t = timed({"1e4": lambda: glx.rows_coalesce(small, grad_out, 10_000),
               "2e9": lambda: glx.rows_coalesce(small, grad_out, 2_000_000_000)})
    a_ms = show("num_rows = 10^4      (14 key bits)", t["1e4"])
    b_ms = show("num_rows = 2 * 10^9  (31 key bits)", t["2e9"])
    print("  ratio %.2f; run-to-run spread of each leg: %.1f %% and %.1f %%"
          % (b_ms / a_ms, 100 * (t["1e4"][-1] - t["1e4"][0]) / a_ms, 100 * (t["2e9"][-1] - t["2e9"][0]) / b_ms), flush=True)


if __name__ == "__main__":
    main()
