"""Lines and sectors the C3 hop-2 EdgeWeight sampling launch touches under four record layouts, predicted on the host
from the live request before any kernel is written (issue: 20-byte draw records, step 1).

  python scripts/r17/ew_lines_model.py dump [OUT.npz]     on the GPU, once: the live hop-2 request of one C3 step
  python scripts/r17/ew_lines_model.py model [IN.npz] [OUT.txt]     host only, numpy

dump builds the C3 store (RMAT 10 M / 100 M, weighted), draws hop 1 as the bench does and saves, for the 1,638,400
rows of the hop-2 request: the request ids, row_ptr[row] and the degree of each, and per draw the row-local alias
index when the draw takes its alias (-1 when it keeps its own slot; layout (d) needs it).  The slot index ix of every
draw is RECOMPUTED from the Philox contract exactly as kSlotEdgeWeightPacked does (draw_ix below); dump first checks
that restatement against the kernel on a small graph whose neighbour ids are its slot numbers.

model counts the distinct 128-byte lines and 64-byte sectors of the record table the launch touches under
  (a) 32-byte records (slot g at 32 g);
  (b) 24-byte records (slot g at 24 g; one in four straddles a 64-byte boundary);
  (c) 20-byte records, three to a 64-byte sector (slot g at (g // 3) * 64 + (g % 3) * 20);
  (d) 16-byte {prob, nbr_self, eid_self, alias_ix} records and a second gather when the alias is taken,
then runs the same stream, in launch order, through the L2 model of scripts/l2_stripe_sim.cc: 8 private L2s of 4 MiB,
128-byte lines, LRU, workgroup b on XCD b mod 8.  The LRU here is fully associative (l2_stripe_sim.cc: 16 ways)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEFAULT_NPZ = os.path.join(ROOT, "build", "r17", "hop2_request.npz")
DEFAULT_TXT = os.path.join(ROOT, "profiles", "r17", "ew_lines_model.txt")
V, E, B0, K1, K2, GS = 10_000_000, 100_000_000, 65536, 25, 10, 4
SEED, CC_HOP2 = 42, 1
XCDS, L2_LINES, LINE, SECTOR, BLOCK = 8, (4 << 20) // 128, 128, 64, 256

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
LOW = np.uint64(0xFFFFFFFF)


def philox_block(blk, row, seed, cc):
    """Philox4x32-10, key = (seed lo, seed hi), counter = (blk, row, cc lo, cc hi) -> four uint32 arrays."""
    c0, c1 = blk.astype(np.uint32), row.astype(np.uint32)
    c2 = np.full(c0.shape, cc & 0xFFFFFFFF, np.uint32)
    c3 = np.full(c0.shape, cc >> 32, np.uint32)
    k0, k1 = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            n0 = (p1 >> np.uint64(32)).astype(np.uint32) ^ c1 ^ k0
            n2 = (p0 >> np.uint64(32)).astype(np.uint32) ^ c3 ^ k1
            c0, c1, c2, c3 = n0, (p1 & LOW).astype(np.uint32), n2, (p0 & LOW).astype(np.uint32)
            k0, k1 = np.uint32(k0 + W0), np.uint32(k1 + W1)
    return c0, c1, c2, c3


def draw_ix(deg, k, seed, cc, rng_rows=None):
    """-> (ix[batch, k] int32, frac[batch, k] float32): the slot of every draw and the variate the record's prob is
    compared with, as glx_sample_slots_kernel<kSlotEdgeWeightPacked> computes them.  Rows of degree 0 give ix = 0."""
    batch = deg.shape[0]
    kpairs = (k + 1) // 2
    rows = np.arange(batch, dtype=np.uint32) if rng_rows is None else rng_rows.astype(np.uint32)
    w = philox_block(np.tile(np.arange(kpairs, dtype=np.uint32), batch), np.repeat(rows, kpairs), seed, cc)
    u = np.empty((batch * kpairs, 2), np.uint64)
    u[:, 0] = (w[1].astype(np.uint64) << np.uint64(32)) | w[0].astype(np.uint64)
    u[:, 1] = (w[3].astype(np.uint64) << np.uint64(32)) | w[2].astype(np.uint64)
    u = u.reshape(batch, 2 * kpairs)[:, :k]
    rd = ((u >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) * np.maximum(deg.astype(np.float64) - 1.0, 0.0)[:, None]
    rnd = rd.astype(np.float32)
    ix = rnd.astype(np.int32)
    return ix, rnd - ix.astype(np.float32)


# ------------------------------------------------------------------------------------------------------- dump ---
def check_restatement(glx):
    """draw_ix against the kernel: a graph whose neighbour ids are its slot numbers tells which slot each draw took."""
    rng = np.random.default_rng(3)
    deg = np.array([4, 1, 30, 0, 2, 130, 7, 3, 97, 96, 5, 2000], np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    n = int(rp[-1])
    w = (rng.random(n) * 0.99 + 0.01).astype(np.float32)
    g = glx.Graph(rp, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), w)
    prob, alias = g.export_alias()
    q = np.resize(np.arange(deg.shape[0], dtype=np.int64), 500)
    for k, cc in ((10, 1), (25, 0), (7, 5)):
        nbr, _ = g.sample("EdgeWeightSampler", q, k, seed=SEED, call_counter=cc)
        ix, frac = draw_ix(deg[q], k, SEED, cc)
        slot = rp[q][:, None] + ix
        take = prob[np.minimum(slot, n - 1)] <= frac
        want = np.where(take, rp[q][:, None] + alias[np.minimum(slot, n - 1)], slot)
        live = (deg[q] > 0)[:, None] & np.ones_like(take)
        assert np.array_equal(nbr[live], want[live]), "the Philox restatement disagrees with the kernel"
    g.close()


def dump(out):
    sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
    import torch
    import glx
    import synth
    check_restatement(glx)
    dev = torch.device("cuda", 0)
    src, dst, w = synth.rmat_edges_torch(V, E, GS, dev, weighted=True)
    uniq, counts = torch.unique(src, return_counts=True)  # rows are the distinct sources, ascending (glx_build.hip)
    g = glx.Graph.from_edges(src, dst, w)
    del src, dst, w
    assert g.num_rows == uniq.shape[0]
    row_ptr = torch.zeros(uniq.shape[0] + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(counts, 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    seeds = uniq[torch.randint(0, uniq.shape[0], (B0,), generator=gen, device=dev)]
    n1, _ = g.sample("EdgeWeightSampler", seeds, K1, seed=SEED, call_counter=0)
    ids = n1.view(-1).contiguous()
    row = torch.searchsorted(uniq, ids).clamp_(max=uniq.shape[0] - 1)
    known = uniq[row] == ids
    start = torch.where(known, row_ptr[row], torch.zeros_like(row))
    deg = torch.where(known, counts[row], torch.zeros_like(row))
    assert torch.equal(deg, g.degrees(ids)), "row_ptr as rebuilt here is not the graph's"
    h_start, h_deg = start.cpu().numpy(), deg.cpu().numpy().astype(np.int32)
    ix, frac = draw_ix(h_deg, K2, SEED, CC_HOP2)
    # which draws take their alias, and which row-local slot that is
    prob = torch.empty(E, dtype=torch.float32, device=dev)
    alias = torch.empty(E, dtype=torch.int32, device=dev)
    rc = glx.lib().glx_graph_export_alias(g._h, prob.data_ptr(), alias.data_ptr(), glx.PTR_DEVICE, None)
    assert rc == 0
    torch.cuda.synchronize()
    slot = torch.from_numpy(h_start[:, None] + ix).to(dev)
    take = prob[slot] <= torch.from_numpy(frac).to(dev)
    alias_ix = torch.where(take, alias[slot], torch.full_like(alias[slot], -1))
    alias_ix[torch.from_numpy(h_deg == 0).to(dev)] = -1
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, ids=ids.cpu().numpy(), start=h_start, deg=h_deg, alias_ix=alias_ix.cpu().numpy())
    print("dumped %d rows, %d draws, %.1f %% take their alias -> %s" % (
        ids.shape[0], ix.size, 100.0 * float(take.float().mean()), out))


# ------------------------------------------------------------------------------------------------------ model ---
def lru_misses(lines, xcd):
    """Misses of XCDS private LRU caches of L2_LINES lines each; lines / xcd in launch order."""
    from collections import OrderedDict
    misses = 0
    for x in range(XCDS):
        lru = OrderedDict()
        for line in lines[xcd == x].tolist():
            if line in lru:
                lru.move_to_end(line)
            else:
                misses += 1
                lru[line] = None
                if len(lru) > L2_LINES:
                    lru.popitem(last=False)
    return misses


def model(path, out):
    z = np.load(path)
    start, deg, alias_ix = z["start"], z["deg"], z["alias_ix"]
    batch = start.shape[0]
    ix, _ = draw_ix(deg, K2, SEED, CC_HOP2)
    live = np.repeat(deg > 0, K2).reshape(batch, K2)
    g = (start[:, None] + ix).astype(np.int64)
    kpairs = (K2 + 1) // 2
    thread = np.arange(batch, dtype=np.int64)[:, None] * kpairs + np.arange(K2)[None, :] // 2
    xcd_of = ((thread // BLOCK) % XCDS).astype(np.int8)
    g, xcd_of, alias_g = g[live], xcd_of[live], (start[:, None] + np.maximum(alias_ix, 0))[live]
    taken = (alias_ix >= 0)[live]
    n = g.shape[0]
    lines_out = []

    def say(s):
        print(s, flush=True)
        lines_out.append(s)

    say("# C3 hop-2 EdgeWeight sampling request: %d rows (%d of degree 0), %d live draws, %.1f %% take their alias"
        % (batch, int((deg == 0).sum()), n, 100.0 * taken.mean()))
    say("# distinct slots drawn: %d" % np.unique(g).shape[0])

    def spans(first, last, unit):
        """the units [first // unit, last // unit] of every access, in access order: (units, access index)"""
        lo, hi = first // unit, last // unit
        two = hi > lo
        idx = np.concatenate([np.arange(first.shape[0]), np.nonzero(two)[0]])
        u = np.concatenate([lo, hi[two]])
        o = np.argsort(idx, kind="stable")
        return u[o], idx[o]

    layouts = {
        "(a) 32-byte": (g * 32, g * 32 + 31, None),
        "(b) 24-byte": (g * 24, g * 24 + 23, None),
        "(c) 20-byte, 3 per sector": ((g // 3) * 64 + (g % 3) * 20, (g // 3) * 64 + (g % 3) * 20 + 19, None),
        "(d) 16-byte + alias gather": (g * 16, g * 16 + 15, alias_g[taken] * 16),
    }
    say("# layout  table GB  distinct 128 B lines  distinct 64 B sectors  lines per draw  modelled L2 line fetches (8 x 4 MiB LRU)  fetched MB  vs (a)")
    base = None
    for name, (first, last, second) in layouts.items():
        bytes_per = {"(a)": 32.0, "(b)": 24.0, "(c)": 64.0 / 3, "(d)": 16.0}[name[:3]]
        acc_first, acc_last, acc_idx = first, last, np.arange(n)
        if second is not None:  # the alias gather follows its draw's own record
            t = np.nonzero(taken)[0]
            acc_idx = np.concatenate([np.arange(n), t])
            o = np.argsort(acc_idx, kind="stable")
            acc_first = np.concatenate([first, second])[o]
            acc_last = np.concatenate([last, second + 15])[o]
            acc_idx = acc_idx[o]
        ln, li = spans(acc_first, acc_last, LINE)
        sc, _ = spans(acc_first, acc_last, SECTOR)
        miss = lru_misses(ln, xcd_of[acc_idx[li]])
        if base is None:
            base = miss
        say("%-28s %.2f  %d  %d  %.3f  %d  %.1f  %+.1f %%" % (
            name, bytes_per * E / 1e9, np.unique(ln).shape[0], np.unique(sc).shape[0], np.unique(ln).shape[0] / n, miss,
            miss * LINE / 1e6, 100.0 * (miss - base) / base))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines_out) + "\n")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "model"
    if mode == "dump":
        dump(sys.argv[2] if len(sys.argv) > 2 else DEFAULT_NPZ)
    else:
        model(sys.argv[2] if len(sys.argv) > 2 else DEFAULT_NPZ, sys.argv[3] if len(sys.argv) > 3 else DEFAULT_TXT)
