"""glx_tgn_store_update, glx_tgn_message, glx_tgn_message_backward and glx_tgn_memory_write against the restatement
(tgn_memory_ref.py): bit for bit, except the time encoding and its gradients, which have the bounds of the contract."""
import numpy as np
import pytest

import glx
import tgn_memory_ref as tref

pytestmark = pytest.mark.gpu

N = 97  # small enough that the ids of a batch collide
I64 = np.iinfo(np.int64)
BATCHES = [0, 1, 63, 64, 65, 257, 1000]
GUARD = 32


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Guarded:
    """a device array with GUARD canary words behind it"""

    def __init__(self, torch, a, shift=0):
        a = np.ascontiguousarray(a)
        self.size, self.shift = a.size, shift
        canary = -7.25 if a.dtype == np.float32 else 0x5A5A5A5A5A5A5A5A
        full = np.full(shift + a.size + GUARD, canary, a.dtype)
        full[shift:shift + a.size] = a.reshape(-1)
        self.full = torch.from_numpy(full).cuda()
        self.canary = full[shift + a.size:].copy()
        self.t = self.full[shift:shift + a.size].view(a.shape)

    def host(self):
        got = self.full.cpu().numpy()
        assert np.array_equal(got[self.shift + self.size:], self.canary), "a write behind the buffer"
        return got[self.shift:self.shift + self.size].reshape(tuple(self.t.shape))


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), what


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the store -----------------------------------------------------------------------------------------------------
def _events(rng, B, call, t_lo):
    """B events from time t_lo on, ascending with runs of ties: self loops, ids outside the table, and in the odd calls
    a hub (node 5) that is an end point of every event"""
    src, dst = rng.integers(0, N, B).astype(np.int64), rng.integers(0, N, B).astype(np.int64)
    loops = rng.random(B) < 0.1
    dst[loops] = src[loops]
    if call % 2 == 1:
        as_src = rng.random(B) < 0.5
        src[as_src] = 5
        dst[~as_src] = 5
    for bad in (-1, N, I64.min, I64.max):
        for side in (src, dst):
            if B > 8:
                side[rng.integers(0, B)] = bad
    t = t_lo + np.sort(rng.integers(0, max(B // 8, 2), B)).astype(np.int64)
    return src, dst, t


@pytest.mark.parametrize("R", [0, 1, 3, 4, 172, 257])
@pytest.mark.parametrize("first", range(len(BATCHES)))
def test_store_update_five_calls(torch, R, first):
    rng = np.random.default_rng(1000 * R + first)
    log = tref.EventLog(N, R)
    bufs = [Guarded(torch, a) for a in tref.slot_arrays({}, N, R)]
    seq_base, t_lo = 0, -40  # the stream starts below zero and, with the larger batches, crosses it
    for call in range(5):
        B = BATCHES[(first + call) % len(BATCHES)]
        # the third call's timestamps lie below the second's: the stream is not time-ordered there
        src, dst, t = _events(rng, B, call, t_lo - 200 if call == 2 else t_lo)
        t_lo = int(t[-1]) if B and call != 2 else t_lo
        raw = rng.standard_normal((B, R)).astype(np.float32)
        log.update(src, dst, t, raw)
        glx.tgn_store_update(_cuda(torch, src), _cuda(torch, dst), _cuda(torch, t), _cuda(torch, raw), seq_base,
                             *[b.t for b in bufs])
        seq_base += B
        for b, want, name in zip(bufs, log.arrays(), ("pend_t", "pend_seq", "pend_other", "pend_raw")):
            _same(b.host(), want, "%s after call %d (B = %d)" % (name, call, B))


def test_store_update_same_bits_on_a_second_run_and_a_tie_only_batch(torch):
    """every event of the batch has ONE timestamp and two hubs meet in every event: the largest position wins"""
    B, R = 1000, 3
    rng = np.random.default_rng(3)
    src, dst, t = np.full(B, 5, np.int64), np.full(B, 9, np.int64), np.full(B, 77, np.int64)
    raw = rng.standard_normal((B, R)).astype(np.float32)
    outs = []
    for _ in range(2):
        bufs = [Guarded(torch, a) for a in tref.slot_arrays({}, N, R)]
        glx.tgn_store_update(_cuda(torch, src), _cuda(torch, dst), _cuda(torch, t), _cuda(torch, raw), 10, *[b.t for b in bufs])
        outs.append([b.host() for b in bufs])
    for a, b in zip(*outs):
        _same(a, b)
    pt, ps, po, pr = outs[0]
    assert pt[5] == 77 and ps[5] == 10 + B - 1 and po[5] == 9 and po[9] == 5
    _same(pr[5], raw[-1])
    _same(pr[9], raw[-1])
    assert (ps >= 0).sum() == 2


# ---- the message ---------------------------------------------------------------------------------------------------
def _state(rng, M, R, T, nodes=N, empty=0.25):
    """a memory with -0.0 and NaN elements and a store in which some nodes have no message and some messages name an
    other end point outside the table; last_update = pend_t - (the recipe's dt)"""
    memory = rng.standard_normal((nodes, M)).astype(np.float32)
    flat = memory.reshape(-1)
    flat[rng.integers(0, flat.size, max(flat.size // 16, 1))] = -0.0
    flat.view(np.uint32)[rng.integers(0, flat.size, max(flat.size // 16, 1))] = 0x7FC12345  # a NaN with a payload
    w, b, dt = tref.time_recipe(rng, nodes, T)
    pend_t, pend_seq, pend_other, pend_raw = tref.slot_arrays({}, nodes, R)
    live = rng.random(nodes) >= empty
    pend_t[live] = rng.integers(-10 ** 6, 10 ** 6, int(live.sum()))
    pend_seq[live] = rng.integers(0, 10 ** 6, int(live.sum()))
    pend_other[live] = rng.integers(-1, nodes + 1, int(live.sum()))  # -1 and `nodes` are outside
    pend_raw[live] = rng.standard_normal((int(live.sum()), R)).astype(np.float32)
    last_update = np.where(live, pend_t - dt, rng.integers(0, 100, nodes)).astype(np.int64)
    return memory, last_update, (pend_t, pend_seq, pend_other, pend_raw), w, b


def _ulps(torch, fn, x, want64):
    """the largest ulp error of torch's fn on the GPU over the float32 arguments x, floored at 1"""
    if x.size == 0:
        return 1.0
    got = fn(_cuda(torch, x.reshape(-1))).cpu().numpy()
    return max(tref.ulp_error(got, want64.reshape(-1)), 1.0)


def _run_message(torch, memory, last_update, pend, w, b, n_id, shift=0):
    dev = [Guarded(torch, a, shift) for a in (memory, last_update, *pend, w, b, n_id)]
    out = glx.tgn_message(*[d.t for d in dev])
    for d, a in zip(dev, (memory, last_update, *pend, w, b, n_id)):
        _same(d.host(), np.ascontiguousarray(a), "an input changed")
    return [o.cpu().numpy() for o in out]


def _check_message(torch, memory, last_update, pend, w, b, n_id, shift=0):
    M, R, T = memory.shape[1], pend[3].shape[1], len(w)
    msg, h, dt, t_out, has = _run_message(torch, memory, last_update, pend, w, b, n_id, shift)
    rh, rhas, rt, rdt, rcopied, x, enc = tref.message(memory, last_update, pend, w, b, n_id)
    _same(h, rh, "h_out")
    _same(has, rhas, "has_out")
    _same(t_out, rt, "t_out")
    _same(dt, rdt, "dt_out")
    assert msg.shape == (len(n_id), 2 * M + R + T)
    _same(np.ascontiguousarray(msg[:, :2 * M + R]), rcopied, "the three copied parts")
    got = msg[:, 2 * M + R:]
    absent = rhas == 0
    assert not got[absent].view(np.uint32).any(), "the time columns of a row without a message must be +0.0"
    live = ~absent
    Et = _ulps(torch, torch.cos, x[live], np.cos(x[live].astype(np.float64)))
    bound = tref.encoding_bound(x[live], Et)
    err = np.abs(got[live].astype(np.float64) - enc[live])
    print("message M %d R %d T %d n %d: Et %.2f, worst error / bound %.3f" % (M, R, T, len(n_id), Et,
                                                                            float((err / bound).max()) if err.size else 0.0))
    assert np.all(err <= bound)
    return bound


@pytest.mark.parametrize("M,R,T", [(1, 0, 1), (4, 3, 8), (100, 172, 100), (256, 257, 7)])
@pytest.mark.parametrize("n", [0, 1, 63, 65, 300])
def test_message(torch, M, R, T, n):
    rng = np.random.default_rng(M * 1000 + n)
    memory, last_update, pend, w, b = _state(rng, M, R, T)
    n_id = rng.integers(0, N, n).astype(np.int64)  # repeats, nodes with and without a message
    if n > 8:
        n_id[rng.permutation(n)[:4]] = [-1, N, I64.min, I64.max]
    _check_message(torch, memory, last_update, pend, w, b, n_id)


def test_message_on_buffers_that_are_not_16_byte_aligned(torch):
    """M, R and T are multiples of 4, every base pointer is 8 bytes (int64) or 4 bytes (float32) past a 16-byte line"""
    rng = np.random.default_rng(11)
    memory, last_update, pend, w, b = _state(rng, 8, 4, 4)
    _check_message(torch, memory, last_update, pend, w, b, rng.integers(-1, N + 1, 70).astype(np.int64), shift=1)


@pytest.mark.parametrize("T", [100, 8, 7])
def test_time_encoding_tolerance(torch, T):
    """every node of a 300-node table has a message, dt by the recipe: each element within
    ulp32(x) + (2 Et + 1) 2^-24 of the float64 cosine of x, and at least 90 % of the bounds at most 2^-10"""
    nodes = 300
    rng = np.random.default_rng(T)
    memory, last_update, pend, w, b = _state(rng, 4, 3, T, nodes=nodes, empty=0.0)
    bound = _check_message(torch, memory, last_update, pend, w, b, np.arange(nodes, dtype=np.int64))
    assert bound.shape == (nodes, T)
    assert np.mean(bound <= 2.0 ** -10) >= 0.9


# ---- the gradient of the time encoder --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(0, 7), (1, 1), (255, 7), (257, 100), (1030, 100), (64 * 256 + 300, 7)])
@pytest.mark.parametrize("far", [True, False])
def test_message_backward(torch, n, T, far):
    """far: the recipe as it is, whose 5 % of dt up to 2^40 dominate the bound; not far: every dt in [0, 4096], where the
    bound is tight enough to see a wrong term"""
    rng = np.random.default_rng(n + T)
    off, width = 5, 5 + T + 3
    w, b, dt_int = tref.time_recipe(rng, n, T)
    dt = (dt_int if far else dt_int % 4097).astype(np.float32)
    has = (rng.random(n) < 0.7).astype(np.int32)
    g = rng.standard_normal((n, width)).astype(np.float32)
    g[has == 0] = np.nan  # a row without a message contributes nothing, whatever its gradient holds
    dev = [_cuda(torch, a) for a in (g, dt, has, w, b)]
    gw, gb = glx.tgn_message_backward(*dev, off)
    gw2, gb2 = glx.tgn_message_backward(*dev, off)
    gw, gb, gw2, gb2 = (a.cpu().numpy() for a in (gw, gb, gw2, gb2))
    _same(gw, gw2, "two calls, grad_w")
    _same(gb, gb2, "two calls, grad_b")
    want_w, want_b, scale, abs_w, abs_b, x = tref.time_gradients(g[:, off:off + T], dt, has, w, b)
    live = has != 0
    Es = _ulps(torch, torch.sin, x[live], np.sin(x[live].astype(np.float64)))
    D = glx.tgn_backward_depth(n)
    for got, want, abs_terms, name in ((gw, want_w, abs_w, "grad_w"), (gb, want_b, abs_b, "grad_b")):
        bound = tref.backward_bound(scale, x, has, abs_terms, Es, D)
        err = np.abs(got.astype(np.float64) - want)
        print("backward n %d T %d %s: Es %.2f D %d, worst error / bound %.3g" % (
            n, T, name, Es, D, float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(np.isfinite(got)) and np.all(err <= bound), name
    if n == 0 or not live.any():
        assert not gw.view(np.uint32).any() and not gb.view(np.uint32).any()  # +0.0


# ---- the memory write ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4, 100, 257])
@pytest.mark.parametrize("n", [0, 1, 65])
def test_memory_write(torch, M, n):
    rng = np.random.default_rng(M + n)
    memory = rng.standard_normal((N, M)).astype(np.float32)
    memory.reshape(-1).view(np.uint32)[::7] = 0x7FC12345  # untouched rows keep even these bits
    last_update = rng.integers(-100, 100, N).astype(np.int64)
    n_id = rng.permutation(N)[:n].astype(np.int64)  # distinct
    if n > 8:
        n_id[[3, 20, 40, 60]] = [-1, N, I64.min, I64.max]
    new = rng.standard_normal((n, M)).astype(np.float32)
    t_new = rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64)
    dm, dl = Guarded(torch, memory), Guarded(torch, last_update)
    glx.tgn_memory_write(dm.t, dl.t, _cuda(torch, n_id), _cuda(torch, new), _cuda(torch, t_new))
    ok = (n_id >= 0) & (n_id < N)
    memory[n_id[ok]], last_update[n_id[ok]] = new[ok], t_new[ok]
    _same(dm.host(), memory, "memory")
    _same(dl.host(), last_update, "last_update")
