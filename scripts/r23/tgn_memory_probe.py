"""A first measurement of the device-resident TGN memory (graphlearn.nn.pytorch.TGNMemory over glx_tgn_store_update,
glx_tgn_message, glx_tgn_message_backward, glx_tgn_memory_write): one training-mode cycle, forward(n_id) +
update_state(src, dst, t, raw_msg), against two other ways to the same state on the same machine in the same run.

  shapes   M = T = 100, R = 172 (the reference's memory_dim, time_dim, msg_dim), N = 10^6 nodes
  batches  B = 200 (the reference's batch size) and B = 65,536; n_id = the distinct ids of (src, dst, one negative)
  module   TGNMemory
  dict     torch_geometric's algorithm: two dicts of per-node tensors keyed by node id, walked with .tolist() on every
           forward and every update_state, LastAggregator by scatter-argmax, on the GPU
  torch    a vectorised composite: stable sorts of the 2B candidates by (node, t, seq), a segment-last pick, scatters
           into the same six buffers; index_select and cat for the message
The three share one GRUCell; the GRU is part of every cycle.  Also reported: the four entry points apart (HIP events
around one call each), Et and Es (the largest ulp error of torch.cos / torch.sin on this GPU over the tolerance tests'
arguments, against float64), and glx_tgn_store_update on a batch in which one hub is an end point of every event
against a batch without one.

One process, HIP events, 2 warm-up + 10 timed repetitions, legs interleaved, medians (the dict leg at B = 65,536: 1 + 3,
it takes seconds).  Nothing here is a requirement of the test suite, and no ratio is promised.
Usage: python scripts/r23/tgn_memory_probe.py > profiles/r23/tgn_memory.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import glx  # noqa: E402
import tgn_memory_ref as tref  # noqa: E402
from graphlearn.nn.pytorch import TGNMemory  # noqa: E402

WARMUP, REPS = 2, 10
N, M, R, T = 10 ** 6, 100, 172, 100
I64_MIN = -2 ** 63


def timed(legs, warmup=WARMUP, reps=REPS):
    times = {k: [] for k in legs}
    for rep in range(warmup + reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


class DictMemory:
    """torch_geometric's TGNMemory (IdentityMessage, LastAggregator), its stores and loops as they are there"""

    def __init__(self, gru, time_w, time_b):
        self.gru, self.w, self.b = gru, time_w, time_b
        self.memory = torch.zeros(N, M, device="cuda")
        self.last_update = torch.zeros(N, dtype=torch.int64, device="cuda")
        self.msg_s, self.msg_d = {}, {}
        i, f = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, R, device="cuda")
        self.empty = (i, i, i, f)
        self.assoc = torch.empty(N, dtype=torch.int64, device="cuda")

    def _update_store(self, src, dst, t, raw, store):
        n_id, perm = src.sort()
        n_id, count = n_id.unique_consecutive(return_counts=True)
        for i, idx in zip(n_id.tolist(), perm.split(count.tolist())):
            store[i] = (src[idx], dst[idx], t[idx], raw[idx])

    def _compute_msg(self, n_id, store):
        data = [store.get(i, self.empty) for i in n_id.tolist()]
        src, dst, t, raw = (torch.cat(x, 0) for x in zip(*data))
        t_rel = t - self.last_update[src]
        enc = torch.cos(t_rel.float()[:, None] * self.w + self.b)
        return torch.cat([self.memory[src], self.memory[dst], raw, enc], -1), t, src

    def updated(self, n_id):
        self.assoc[n_id] = torch.arange(n_id.numel(), device="cuda")
        ms, ts, ss = self._compute_msg(n_id, self.msg_s)
        md, td, sd = self._compute_msg(n_id, self.msg_d)
        idx, msg, t = torch.cat([ss, sd]), torch.cat([ms, md]), torch.cat([ts, td])
        local = self.assoc[idx]
        aggr = msg.new_zeros(n_id.numel(), msg.shape[1])
        if idx.numel():  # LastAggregator: the arg-max of t per node
            best = torch.full((n_id.numel(),), I64_MIN, dtype=torch.int64, device="cuda").scatter_reduce(0, local, t, "amax")
            pick = (t == best[local]).nonzero().reshape(-1)
            aggr[local[pick]] = msg[pick]
        memory = self.gru(aggr, self.memory[n_id])
        last = self.last_update.scatter(0, idx, t)[n_id]
        return memory, last

    def forward(self, n_id):
        return self.updated(n_id)

    def update_state(self, src, dst, t, raw):
        n_id = torch.cat([src, dst]).unique()
        with torch.no_grad():
            memory, last = self.updated(n_id)
        self.memory[n_id], self.last_update[n_id] = memory, last
        self._update_store(src, dst, t, raw, self.msg_s)
        self._update_store(dst, src, t, raw, self.msg_d)


class TorchMemory:
    """the six buffers of the module, kept with sorts, scatters, index_select and cat"""

    def __init__(self, gru, time_w, time_b):
        self.gru, self.w, self.b = gru, time_w, time_b
        self.memory = torch.zeros(N, M, device="cuda")
        self.last_update = torch.zeros(N, dtype=torch.int64, device="cuda")
        self.pend_t = torch.full((N,), I64_MIN, dtype=torch.int64, device="cuda")
        self.pend_seq = torch.full((N,), -1, dtype=torch.int64, device="cuda")
        self.pend_other = torch.full((N,), -1, dtype=torch.int64, device="cuda")
        self.pend_raw = torch.zeros(N, R, device="cuda")
        self.seq_base = 0

    def updated(self, n_id):
        has = self.pend_seq[n_id] >= 0
        t = self.pend_t[n_id]
        dt = torch.where(has, t - self.last_update[n_id], torch.zeros_like(t)).float()
        h = self.memory.index_select(0, n_id)
        other = self.memory.index_select(0, self.pend_other[n_id].clamp(min=0))
        msg = torch.cat([h, other, self.pend_raw.index_select(0, n_id), torch.cos(dt[:, None] * self.w + self.b)], 1)
        msg = torch.where(has[:, None], msg, torch.zeros_like(msg))
        return self.gru(msg, h), torch.where(has, t, self.last_update[n_id])

    def forward(self, n_id):
        return self.updated(n_id)

    def update_state(self, src, dst, t, raw):
        B = src.numel()
        u = torch.cat([src, dst]).unique()
        with torch.no_grad():
            memory, last = self.updated(u)
        self.memory[u], self.last_update[u] = memory, last
        own, other, tt = torch.cat([src, dst]), torch.cat([dst, src]), torch.cat([t, t])
        pos = torch.arange(B, device="cuda").repeat(2)
        order = torch.sort(pos, stable=True)[1]
        order = order[torch.sort(tt[order], stable=True)[1]]
        order = order[torch.sort(own[order], stable=True)[1]]  # by (node, t, seq)
        own_s = own[order]
        last_of = torch.ones_like(own_s, dtype=torch.bool)
        last_of[:-1] = own_s[1:] != own_s[:-1]
        win = order[last_of]
        v, tv = own[win], tt[win]
        keep = tv >= self.pend_t[v]  # every stored seq is below seq_base
        v, win = v[keep], win[keep]
        self.pend_t[v], self.pend_seq[v], self.pend_other[v] = tt[win], self.seq_base + pos[win], other[win]
        self.pend_raw[v] = raw[pos[win]]
        self.seq_base += B


def batch_of(gen, B, step, hub=False):
    src = torch.randint(0, N, (B,), device="cuda", generator=gen)
    dst = torch.randint(0, N, (B,), device="cuda", generator=gen)
    if hub:
        src = torch.where(torch.arange(B, device="cuda") % 2 == 0, torch.full_like(src, 5), src)
        dst = torch.where(torch.arange(B, device="cuda") % 2 == 1, torch.full_like(dst, 5), dst)
    neg = torch.randint(0, N, (B,), device="cuda", generator=gen)
    t = step * 1000 + torch.sort(torch.randint(0, 1000, (B,), device="cuda", generator=gen))[0]
    raw = torch.randn(B, R, device="cuda", generator=gen)
    return src, dst, t, raw, torch.cat([src, dst, neg]).unique()


def ulps():
    rng = np.random.default_rng(0)
    w, b, dt = tref.time_recipe(rng, 20000, T)
    x = tref.fma32(w[None, :], dt.astype(np.float32)[:, None], b[None, :]).reshape(-1)
    xd = torch.from_numpy(x).cuda()
    x64 = x.astype(np.float64)
    return (tref.ulp_error(torch.cos(xd).cpu().numpy(), np.cos(x64)), tref.ulp_error(torch.sin(xd).cpu().numpy(), np.sin(x64)))


def main():
    sys.stdout.reconfigure(line_buffering=True)
    print("device: %s" % torch.cuda.get_device_name(0))
    print("N %d, M %d, R %d, T %d; medians of %d after %d warm-up (the dict form at B = 65,536: of 3 after 1), ms" % (
        N, M, R, T, REPS, WARMUP))
    Et, Es = ulps()
    print("largest ulp error over the tolerance recipe's arguments (2,000,000 of them): torch.cos Et = %.3f, "
          "torch.sin Es = %.3f" % (Et, Es))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    torch.manual_seed(0)
    mod = TGNMemory(N, R, M, T).cuda()
    mod.train()
    w, b = mod.time_enc.weight.detach(), mod.time_enc.bias.detach()
    for B in (200, 65536):
        paths = {"module": mod, "dict": DictMemory(mod.gru, w, b), "torch": TorchMemory(mod.gru, w, b)}
        mod.reset_state()
        steps = {k: 0 for k in paths}
        batches = [batch_of(gen, B, s) for s in range(WARMUP + REPS + 1)]

        def cycle(name):
            def run():
                src, dst, t, raw, n_id = batches[steps[name] % len(batches)]
                steps[name] += 1
                with torch.no_grad():
                    paths[name].forward(n_id)
                paths[name].update_state(src, dst, t, raw)
            return run

        slow = B > 10000
        fast = timed({k: cycle(k) for k in ("module", "torch")})
        fast.update(timed({"dict": cycle("dict")}, *((1, 3) if slow else (WARMUP, REPS))))
        n_ids = int(np.mean([x[4].numel() for x in batches]))
        print("B %6d (about %d ids per forward): one cycle  module %.3f   dict-form %.3f   torch composite %.3f" % (
            B, n_ids, fast["module"], fast["dict"], fast["torch"]))
        # the four entry points apart, on the module's state
        src, dst, t, raw, n_id = batches[-1]
        bufs = (mod.memory, mod.last_update, mod.pend_t, mod.pend_seq, mod.pend_other, mod.pend_raw)
        msg, h, dt, t_out, has = glx.tgn_message(*bufs, w, b, n_id)
        grad = torch.randn_like(msg)
        new = torch.randn(n_id.numel(), M, device="cuda")
        hub = batch_of(gen, B, WARMUP + REPS + 2, hub=True)
        seq = [mod.seq_base]

        def store(ev):
            def run():
                glx.tgn_store_update(ev[0], ev[1], ev[2], ev[3], seq[0], *bufs[2:])
                seq[0] += B
            return run

        k = timed({"store_update": store((src, dst, t, raw)), "store_update_hub": store(hub),
                   "message": lambda: glx.tgn_message(*bufs, w, b, n_id),
                   "message_backward": lambda: glx.tgn_message_backward(grad, dt, has, w, b, 2 * M + R),
                   "memory_write": lambda: glx.tgn_memory_write(mod.memory, mod.last_update, n_id, new, t_out)})
        print("B %6d entry points: store_update %.3f   message (n %d) %.3f   message_backward %.3f   memory_write %.3f" % (
            B, k["store_update"], n_id.numel(), k["message"], k["message_backward"], k["memory_write"]))
        print("B %6d store_update with one hub in every event %.3f against %.3f without: %.2f x" % (
            B, k["store_update_hub"], k["store_update"], k["store_update_hub"] / k["store_update"]))
        del paths, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
