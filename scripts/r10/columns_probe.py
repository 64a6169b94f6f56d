"""Device-resident label / int-attribute columns on the hop-2 id stream of a real C3 step (RMAT 10 M / 100 M, EdgeWeight
[25, 10], 65,536 seeds: 1.64 M ids), int_attrs of i_num = 8 plus labels (72 B of fields, 80-byte records):

  1. glx.Columns.lookup(ids, ("labels", "int_attrs")) on the device, in ms, with the algorithmic bytes per id;
  2. the same answer through the host operators (LookupNodes over the host columns) plus a .to(device) -- the path the
     device table replaces.  The host operators are untouched by the device table, so this leg times the same code the
     parent commit runs.  It goes through a gl.Graph loaded from a TSV source of `host_nodes` vertices (the stream's
     ids are folded into that range): a smaller host index than C3's 10 M vertices flatters the host path if anything;
  3. the GATHER32 probe rate of the same run (glx_probe_bandwidth): random 32-byte records of a table of the same size,
     the line-gather ceiling the lookup kernel is to be read against;
  4. NeighborLoader ms per batch with node_columns=() and with ("labels", "int_attrs"), same process, interleaved
     (A/B of the plain path: "default arguments" against a loader object that never heard of columns is the same code).

One process, HIP events, 3 warm-up + 20 timed repetitions, legs interleaved.
Usage: python scripts/r10/columns_probe.py [nodes] [edges] [batch] [host_nodes] > profiles/r10/columns.txt"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import torch  # noqa: E402
import glx  # noqa: E402
import synth  # noqa: E402

WARMUP, REPS = 3, 20
FANOUTS = [25, 10]
I_NUM = 8
WANT = ("labels", "int_attrs")


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


def show(name, ts, n):
    med = ts[len(ts) // 2]
    print("  %-52s median %8.3f ms  min %8.3f  max %8.3f   %6.2f ns/id" % (name, med, ts[0], ts[-1], med * 1e6 / n),
          flush=True)
    return med


class _Sampler(object):
    def __init__(self, g, fanouts):
        self.g, self.fanouts = g, fanouts

    def get_device(self, seeds, seed=None, call_counter=0):
        return glx.sample_hops([self.g] * len(self.fanouts), "EdgeWeightSampler", seeds, self.fanouts, seed=42,
                               call_counter=call_counter)


class _Graph(object):
    """What NeighborLoader asks of a gl.Graph, over glx handles built from tensors."""

    def __init__(self, g, feats, cols):
        self.g, self.feats, self.cols = g, feats, cols

    def neighbor_sampler(self, meta_path, fanouts, strategy="random"):
        return _Sampler(self.g, list(fanouts))

    def get_topology(self):
        return self

    def get_dst_type(self, edge_type):
        return "v"

    def device_features(self, node_type):
        return self.feats

    def device_columns(self, node_type):
        return self.cols


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    VH = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
    D = 256
    dev = torch.device("cuda", 0)
    print("device: %s   graph: RMAT %d vertices / %d edges   EdgeWeight %s   %d seeds   i_num %d + labels"
          % (torch.cuda.get_device_name(0), V, E, FANOUTS, B, I_NUM), flush=True)
    src, dst, w = synth.rmat_edges_torch(V, E, 1, dev, weighted=True)
    pool = torch.unique(src)
    g = glx.Graph.from_edges(src, dst, w)
    del src, dst, w
    feats = glx.Features(synth.features_torch(V, D, 2, dev))
    rows = torch.arange(V, device=dev, dtype=torch.int64)
    labels = (rows % 47).to(torch.int32)
    ia = (rows[:, None] * 1000003 + torch.arange(I_NUM, device=dev)) % 1000
    cols = glx.Columns(V, labels=labels, int_attrs=ia, map_of=feats)
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    seeds = pool[torch.randperm(pool.shape[0], generator=gen, device=dev)[:B]].contiguous()
    hops = glx.sample_hops([g, g], "EdgeWeightSampler", seeds, FANOUTS, seed=42, call_counter=0)
    ids = hops[0][0].reshape(-1).contiguous()  # frontier 1: the ids hop 2 is sampled for
    n = int(ids.numel())
    rec = cols.record_bytes
    out_bytes = 4 + 8 * I_NUM

    # ---- 1. the device lookup
    print("\n[1] glx.Columns.lookup on n = %d ids, records of %d B in a %.2f GB table" % (n, rec, V * rec / 1e9), flush=True)
    t = timed({"device: glx_columns_lookup(labels, int_attrs)": lambda: cols.lookup(ids, WANT)})
    dev_ms = show("device: glx_columns_lookup(labels, int_attrs)", t["device: glx_columns_lookup(labels, int_attrs)"], n)
    per_id = 8 + rec + out_bytes
    print("  algorithmic bytes per id: 8 (id) + %d (record) + %d (outputs) = %d  ->  %.1f GB/s"
          % (rec, out_bytes, per_id, n * per_id / dev_ms / 1e6), flush=True)
    got = cols.lookup(ids, WANT)
    ok = bool(torch.equal(got["labels"], labels[ids]) and torch.equal(got["int_attrs"], ia[ids]))
    print("  equals the torch gather of the source columns: %s" % ok, flush=True)

    # ---- 3. the line-gather ceiling of this run
    pr = glx.probe_bandwidth("gather32", V * rec, units=n, reps=20)
    print("\n[3] GATHER32 probe, %d random 32-byte records of a %.2f GB table: %.3f ms  (%.1f G records/s, %.1f GB/s moved)"
          % (n, V * rec / 1e9, pr["ms"], n / pr["ms"] / 1e6, pr["gbps"]), flush=True)
    print("  lookup / probe time: %.2f  (an 80-byte record spans up to 2 128-byte lines and 3 32-byte sectors; the probe"
          " reads one sector and writes 16 B per unit, the lookup writes %d B)" % (dev_ms / pr["ms"], out_bytes), flush=True)

    # ---- 2. the host operators + .to(device)
    import graphlearn as gl
    d = tempfile.mkdtemp(prefix="columns_probe_")
    path = os.path.join(d, "nodes")
    t0 = time.time()
    with open(path, "w") as fo:
        fo.write("id:int64\tlabel:int64\tfeature:string\n")
        for lo in range(0, VH, 100000):
            r = np.arange(lo, min(VH, lo + 100000), dtype=np.int64)
            a = (r[:, None] * 1000003 + np.arange(I_NUM)) % 1000
            fo.write("".join("%d\t%d\t%s\n" % (v, v % 47, ":".join(map(str, row))) for v, row in zip(r.tolist(), a.tolist())))
    hg = gl.Graph().node(path, "v", gl.Decoder(labeled=True, attr_types=["int"] * I_NUM)).init()
    print("\n[2] host operators: gl.Graph with %d nodes loaded in %.1f s" % (VH, time.time() - t0), flush=True)
    ids_h = (ids % VH).cpu().numpy()

    def host_leg():
        v = hg.lookup_nodes("v", ids_h)
        return torch.from_numpy(v.labels).to(dev), torch.from_numpy(v.int_attrs).to(dev)

    t = timed({"host: LookupNodes(labels, int_attrs) + .to(device)": host_leg})
    host_ms = show("host: LookupNodes(labels, int_attrs) + .to(device)",
                   t["host: LookupNodes(labels, int_attrs) + .to(device)"], n)
    hl, hi = host_leg()
    ok = bool(torch.equal(hl, labels[ids % VH]) and torch.equal(hi.reshape(n, I_NUM), ia[ids % VH]))
    print("  equals the device columns for the folded ids: %s     host / device time: %.0f x" % (ok, host_ms / dev_ms),
          flush=True)
    hg.close()

    # ---- 4. the loader
    shim = _Graph(g, feats, cols)
    seed_ids = pool.cpu().numpy()

    def batches(**kw):
        loader = gl.NeighborLoader(shim, "v", ["e", "e"], FANOUTS, batch_size=B, strategy="edge_weight", seed_ids=seed_ids,
                                   **kw)
        while True:
            for batch in loader:
                yield batch

    a0, a1, b0 = batches(), batches(node_columns=()), batches(node_columns=WANT)
    total = B * (1 + FANOUTS[0] + FANOUTS[0] * FANOUTS[1])
    print("\n[4] NeighborLoader, ms per batch (2 hops + features at dim %d; %d frontier rows)" % (D, total), flush=True)
    t = timed({"default arguments (A)": lambda: next(a0),
               "node_columns=() (B, the same path)": lambda: next(a1),
               'node_columns=("labels", "int_attrs")': lambda: next(b0)})
    med = {k: show(k, v, total) for k, v in t.items()}
    print("  A / B: %.3f   columns on / off: %.3f" % (med["default arguments (A)"] / med["node_columns=() (B, the same path)"],
                                                    med['node_columns=("labels", "int_attrs")'] / med["default arguments (A)"]),
          flush=True)


if __name__ == "__main__":
    main()
