"""Restatement of the TGN memory (include/glx.h, "TGN memory") in torch_geometric's own form, in numpy -- plus a torch
module around it for the tests of graphlearn.nn.pytorch.TGNMemory.

DictStore is TGNMemory's message store as torch_geometric writes it: two stores per node, one per role, that an
update_state OVERWRITES per role with the call's events of that node; the message of a node is computed from the union
of both stores; "last" picks by (t, seq), which fixes what LastAggregator's scatter_argmax leaves open.  Nothing in it
knows of the one-slot-per-node layout of the device store.  latest_events is the contract's own sentence -- the event
with the largest (t, seq) among ALL events that ever named the node -- computed from the full event log; on a
time-ordered stream the two agree (test_tgn_memory_cpu.py), on any other stream latest_events is the contract.
"""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min


class DictStore:
    """msg_s[v] / msg_d[v]: the events (other end point, t, raw row, seq) of the LAST update call that named v as src /
    as dst."""

    def __init__(self, num_nodes, raw_dim):
        self.N, self.R = int(num_nodes), int(raw_dim)
        self.reset()

    def reset(self):
        self.msg_s, self.msg_d, self.seq_base = {}, {}, 0

    def _update_role(self, store, own, other, t, raw):
        for v in sorted(set(int(x) for x in own)):  # torch_geometric: sort, unique_consecutive, one entry per node
            if 0 <= v < self.N:
                idx = np.flatnonzero(own == v)
                store[v] = (other[idx].copy(), t[idx].copy(), raw[idx].copy(), self.seq_base + idx.astype(np.int64))

    def update(self, src, dst, t, raw):
        src, dst, t = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(t, np.int64)
        raw = np.asarray(raw, np.float32).reshape(len(src), self.R)
        self._update_role(self.msg_s, src, dst, t, raw)
        self._update_role(self.msg_d, dst, src, t, raw)
        self.seq_base += len(src)

    def last(self, v):
        """(t, seq, other, raw row) of the last message of v over both roles, or None"""
        best = None
        for store in (self.msg_s, self.msg_d):
            if v in store:
                other, t, raw, seq = store[v]
                for k in range(len(t)):
                    key = (int(t[k]), int(seq[k]))
                    if best is None or key > best[0]:
                        best = (key, int(other[k]), raw[k])
        return None if best is None else (best[0][0], best[0][1], best[1], best[2])

    def arrays(self):
        """the store as the four pend_* arrays of the contract"""
        return slot_arrays({v: self.last(v) for v in range(self.N)}, self.N, self.R)


def slot_arrays(last_of, N, R):
    pend_t = np.full(N, INT64_MIN, np.int64)
    pend_seq = np.full(N, -1, np.int64)
    pend_other = np.full(N, -1, np.int64)
    pend_raw = np.zeros((N, R), np.float32)
    for v, m in last_of.items():
        if m is not None:
            pend_t[v], pend_seq[v], pend_other[v] = m[0], m[1], m[2]
            pend_raw[v] = m[3]
    return pend_t, pend_seq, pend_other, pend_raw


class EventLog:
    """every event of every update call; latest_events() applies the contract's sentence to the whole log"""

    def __init__(self, num_nodes, raw_dim):
        self.N, self.R = int(num_nodes), int(raw_dim)
        self.src, self.dst, self.t = (np.zeros(0, np.int64) for _ in range(3))
        self.raw = np.zeros((0, self.R), np.float32)

    def update(self, src, dst, t, raw):
        self.src = np.concatenate([self.src, np.asarray(src, np.int64)])
        self.dst = np.concatenate([self.dst, np.asarray(dst, np.int64)])
        self.t = np.concatenate([self.t, np.asarray(t, np.int64)])
        self.raw = np.concatenate([self.raw, np.asarray(raw, np.float32).reshape(len(self.src) - len(self.raw), self.R)])

    def arrays(self):
        E = len(self.src)
        seq = np.arange(E, dtype=np.int64)
        own = np.concatenate([self.src, self.dst])
        other = np.concatenate([self.dst, self.src])
        ev = np.concatenate([seq, seq])
        ok = (own >= 0) & (own < self.N)
        own, other, ev = own[ok], other[ok], ev[ok]
        order = np.lexsort((ev, self.t[ev], own))  # by node, then t, then seq
        own, other, ev = own[order], other[order], ev[order]
        is_last = np.ones(len(own), bool)
        is_last[:-1] = own[1:] != own[:-1]
        pend_t, pend_seq, pend_other, pend_raw = slot_arrays({}, self.N, self.R)
        v = own[is_last]
        pend_t[v], pend_seq[v], pend_other[v] = self.t[ev[is_last]], ev[is_last], other[is_last]
        pend_raw[v] = self.raw[ev[is_last]]
        return pend_t, pend_seq, pend_other, pend_raw


# ---- the message ---------------------------------------------------------------------------------------------------
def fma32(w, dt, b):
    """fmaf(w, dt, b) of float32 operands as a float64 emulation: the product of two float32 is exact in float64, the
    sum is rounded to float64 and then to float32 -- twice, so it may differ from the one rounding of fmaf by one
    ulp32 of the result (the tolerance's ulp32(x) term)."""
    return (np.asarray(w, np.float32).astype(np.float64) * np.asarray(dt, np.float32).astype(np.float64)
            + np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def message(memory, last_update, pend, time_w, time_b, n_id):
    """glx_tgn_message's outputs; the time encoding in float64: (h, has, t_out, dt, copied [n, 2M + R], x [n, T] float32,
    enc [n, T] float64 -- cos of the float32 x)"""
    pend_t, pend_seq, pend_other, pend_raw = pend
    N, M = memory.shape
    R, T, n = pend_raw.shape[1], len(time_w), len(n_id)
    h = np.zeros((n, M), np.float32)
    has = np.zeros(n, np.int32)
    t_out = np.zeros(n, np.int64)
    dt = np.zeros(n, np.float32)
    copied = np.zeros((n, 2 * M + R), np.float32)
    for i, v in enumerate(int(x) for x in n_id):
        if not 0 <= v < N:
            continue
        h[i] = memory[v]
        t_out[i] = last_update[v]
        if pend_seq[v] >= 0:
            has[i] = 1
            t_out[i] = pend_t[v]
            dt[i] = np.float32(int(pend_t[v]) - int(last_update[v]))  # exact integer difference, one rounding
            o = int(pend_other[v])
            copied[i, :M] = memory[v]
            if 0 <= o < N:
                copied[i, M:2 * M] = memory[o]
            copied[i, 2 * M:] = pend_raw[v]
    x = fma32(np.asarray(time_w, np.float32)[None, :], dt[:, None], np.asarray(time_b, np.float32)[None, :])
    enc = np.where(has[:, None] != 0, np.cos(x.astype(np.float64)), 0.0)
    return h, has, t_out, dt, copied, x, enc


def time_gradients(g, dt, has, time_w, time_b):
    """float64 (grad_w, grad_b, sum_i |g| max(|dt|, 1) [T], sum_i |term_w| [T], sum_i |term_b| [T], x [n, T]) of the
    contract's sums, from the float32 x and dt"""
    x = fma32(np.asarray(time_w, np.float32)[None, :], np.asarray(dt, np.float32)[:, None],
              np.asarray(time_b, np.float32)[None, :])
    live = (np.asarray(has) != 0)[:, None]
    g64 = np.where(live, np.asarray(g, np.float32).astype(np.float64), 0.0)
    dt64 = np.asarray(dt, np.float32).astype(np.float64)[:, None]
    term_b = np.where(live, g64 * -np.sin(x.astype(np.float64)), 0.0)
    term_w = term_b * dt64
    scale = np.abs(g64) * np.maximum(np.abs(dt64), 1.0)
    return term_w.sum(0), term_b.sum(0), scale, np.abs(term_w).sum(0), np.abs(term_b).sum(0), x


def backward_bound(scale, x, has, abs_terms, Es, D):
    """sum_i |g_i| max(|dt_i|, 1) (ulp32(x_i) + (2 Es + 2) 2^-24) + D 2^-24 sum_i |term_i|, per column"""
    live = (np.asarray(has) != 0)[:, None]
    per = np.where(live, scale * (ulp32(x) + (2 * Es + 2) * 2.0 ** -24), 0.0)
    return per.sum(0) + D * 2.0 ** -24 * abs_terms


def ulp_error(got32, want64):
    """the largest error of float32 results in ulps of the float64 answer rounded to float32"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    return float(np.max(np.abs(np.asarray(got32, np.float32).astype(np.float64) - want64) / ulp)) if got32.size else 0.0


def time_recipe(rng, n, T):
    """The inputs of the time-encoding tolerance test: w = 10^-linspace(0, 3, T), |b| <= 1; dt in [0, 4096] for 95 % of
    the nodes (|x| < 8192: the bound stays below 2^-10) and up to 2^40 for 5 % (where the bound is vacuous for the
    large w).  -> (w [T], b [T], dt [n] int64)"""
    w = (10.0 ** -np.linspace(0.0, 3.0, T)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, T).astype(np.float32)
    dt = rng.integers(0, 4097, n).astype(np.int64)
    far = rng.permutation(n)[:n // 20]
    dt[far] = rng.integers(0, 2 ** 40, len(far), dtype=np.int64)
    return w, b, dt


def encoding_bound(x, Et):
    """ulp32(x) + (2 Et + 1) 2^-24"""
    return ulp32(x) + (2 * Et + 1) * 2.0 ** -24


# ---- the module ----------------------------------------------------------------------------------------------------
class DictTGNMemory:
    """torch_geometric's TGNMemory (IdentityMessage, LastAggregator) over DictStore, with a given GRUCell and time
    encoder parameters, on their device: the host loops and .tolist() walks of the original, tensors for the GRU."""

    def __init__(self, num_nodes, raw_dim, mem_dim, gru, time_w, time_b):
        import torch
        self.torch = torch
        self.N, self.R, self.M = num_nodes, raw_dim, mem_dim
        self.gru, self.time_w, self.time_b = gru, time_w, time_b
        self.store = DictStore(num_nodes, raw_dim)
        self.training = True
        self.reset_state()

    def reset_state(self):
        self.store.reset()
        self.memory = np.zeros((self.N, self.M), np.float32)
        self.last_update = np.zeros(self.N, np.int64)

    def _updated(self, n_id):
        """gru(message, memory) and the message times of n_id (an id outside the table: a zero row, as a node without a
        message) -> (tensor [n, M], int64 [n], the message tensor)"""
        torch = self.torch
        dev = self.time_w.device
        h, has, t_out, dt, copied, _, _ = message(self.memory, self.last_update, self.store.arrays(),
                                                  np.zeros(0, np.float32), np.zeros(0, np.float32), n_id)
        dt_t = torch.from_numpy(dt).to(dev)
        live = torch.from_numpy(has != 0).to(dev)
        # x = fmaf(w, dt, b) as the contract has it: the product is exact in float64, one more rounding to float32
        x = (dt_t.double()[:, None] * self.time_w.double() + self.time_b.double()).float()
        enc = torch.cos(x)
        enc = torch.where(live[:, None], enc, torch.zeros_like(enc))
        msg = torch.cat([torch.from_numpy(copied).to(dev), enc], 1)
        return self.gru(msg, torch.from_numpy(h).to(dev)), t_out, msg

    def forward(self, n_id):
        n_id = np.asarray(n_id, np.int64)
        if self.training:
            out, t_out, self.last_msg = self._updated(n_id)
            return out, t_out
        return self.memory[n_id], self.last_update[n_id]

    def _write_memory(self, src, dst):
        both = np.concatenate([src, dst])
        _, first = np.unique(both, return_index=True)
        u = both[np.sort(first)]  # the distinct ids in order of first occurrence ...
        padded = np.concatenate([u, np.full(len(both) - len(u), -1, np.int64)])  # ... at the length the module runs the GRU at
        with self.torch.no_grad():
            new, t_new, _ = self._updated(padded)
        new = new.cpu().numpy()
        for i, v in enumerate(int(x) for x in u):
            if 0 <= v < self.N:
                self.memory[v], self.last_update[v] = new[i], t_new[i]

    def update_state(self, src, dst, t, raw):
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        if self.training:
            self._write_memory(src, dst)
            self.store.update(src, dst, t, raw)
        else:
            self.store.update(src, dst, t, raw)
            self._write_memory(src, dst)
