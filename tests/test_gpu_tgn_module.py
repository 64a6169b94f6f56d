"""graphlearn.nn.pytorch.TGNMemory against torch_geometric's algorithm restated over dict stores
(tgn_memory_ref.DictTGNMemory), with the same GRUCell on the same device; examples/train_tgn.py."""
import copy
import os
import sys

import numpy as np
import pytest

import glx
import tgn_memory_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

NODES, RAW, MEM, TIME = 40, 5, 12, 6
BATCHES, EVENTS = 8, 50


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def thg():
    import graphlearn.nn.pytorch as m
    return m


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    """eight batches of 50 events over 40 nodes, time-ordered with ties inside and across the batches"""
    rng = np.random.default_rng(2)
    t = np.sort(rng.integers(0, BATCHES * EVENTS // 3, BATCHES * EVENTS)).astype(np.int64)
    out = []
    for k in range(BATCHES):
        src, dst = rng.integers(0, NODES, EVENTS).astype(np.int64), rng.integers(0, NODES, EVENTS).astype(np.int64)
        dst[:3] = src[:3]  # self loops
        out.append((src, dst, t[k * EVENTS:(k + 1) * EVENTS], rng.standard_normal((EVENTS, RAW)).astype(np.float32)))
    return out


def _module(torch, thg, zero_time):
    torch.manual_seed(0)
    mod = thg.TGNMemory(NODES, RAW, MEM, TIME).cuda()
    if zero_time:  # the encoding is exactly 1 in the module (fmaf) and in the restatement (a product and a sum)
        with torch.no_grad():
            mod.time_enc.weight.zero_()
            mod.time_enc.bias.zero_()
    return mod


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_state(mod, ref, what):
    assert np.array_equal(_bits(mod.memory), _bits(ref.memory)), what + ": memory"
    assert np.array_equal(_bits(mod.last_update), _bits(ref.last_update)), what + ": last_update"


def _same_forward(torch, mod, ref, n_id, what):
    with torch.no_grad():
        z, lu = mod(_cuda(torch, n_id))
        rz, rlu = ref.forward(n_id)
    assert np.array_equal(_bits(z), _bits(rz)), what + ": forward()[0]"
    assert np.array_equal(_bits(lu), _bits(rlu)), what + ": forward()[1]"


def test_bit_equal_run(torch, thg):
    mod = _module(torch, thg, zero_time=True)
    ref = tref.DictTGNMemory(NODES, RAW, MEM, mod.gru, mod.time_enc.weight, mod.time_enc.bias)
    rng = np.random.default_rng(4)
    stream = _stream()

    def run(training, batches, tag):
        mod.train(training)
        ref.training = training
        for k, (src, dst, t, raw) in enumerate(batches):
            n_id = np.concatenate([src, dst, rng.integers(0, NODES, 7)])  # with repeats, and nodes not in the batch
            _same_forward(torch, mod, ref, n_id, "%s batch %d" % (tag, k))
            mod.update_state(_cuda(torch, src), _cuda(torch, dst), _cuda(torch, t), _cuda(torch, raw))
            ref.update_state(src, dst, t, raw)
            mod.detach()
            _same_state(mod, ref, "%s batch %d" % (tag, k))
            assert np.array_equal(_bits(mod.pend_seq), ref.store.arrays()[1])

    run(True, stream[:5], "train")
    assert mod.seq_base == 5 * EVENTS and mod.last_update.max() > 0 and mod.memory.abs().max() > 0
    run(False, stream[5:], "eval")
    mod.reset_state()
    ref.reset_state()
    _same_state(mod, ref, "reset")
    assert mod.seq_base == 0 and int((mod.pend_seq != -1).sum()) == 0 and int(mod.pend_t.max()) == tref.INT64_MIN
    assert not _bits(mod.memory).any() and not _bits(mod.pend_raw).any() and int(mod.pend_other.max()) == -1
    mod.train(True)
    ref.training = True
    _same_forward(torch, mod, ref, np.arange(NODES, dtype=np.int64), "after reset")


def test_gradients(torch, thg):
    mod = _module(torch, thg, zero_time=False)
    with torch.no_grad():  # the recipe of the kernel test: the bound stays small for dt of a few hundred
        mod.time_enc.weight.copy_(_cuda(torch, (10.0 ** -np.linspace(0, 3, TIME)).astype(np.float32)))
    gru_ref = copy.deepcopy(mod.gru)
    w_ref = mod.time_enc.weight.detach().clone().requires_grad_(True)
    b_ref = mod.time_enc.bias.detach().clone().requires_grad_(True)
    ref = tref.DictTGNMemory(NODES, RAW, MEM, gru_ref, w_ref, b_ref)
    stream = _stream()
    for src, dst, t, raw in stream[:3]:  # some state: the GRU of the reference copy gives the same memory
        mod.update_state(_cuda(torch, src), _cuda(torch, dst), _cuda(torch, t), _cuda(torch, raw))
        ref.update_state(src, dst, t, raw)
    seen = []

    def keep(_module, args):
        args[0].retain_grad()
        seen.append(args[0])

    hook = mod.gru.register_forward_pre_hook(keep)
    n_id = np.concatenate([np.arange(NODES, dtype=np.int64), [3, 3, NODES, -1]])
    z, _ = mod(_cuda(torch, n_id))
    hook.remove()
    z.sum().backward()
    rz, _ = ref.forward(n_id)
    rz.sum().backward()
    torch.testing.assert_close(z, rz)
    for (name, p), (_, q) in zip(mod.gru.named_parameters(), gru_ref.named_parameters()):
        assert p.grad is not None and float(p.grad.abs().max()) > 0, name
        torch.testing.assert_close(p.grad, q.grad, msg=lambda m, name=name: "%s: %s" % (name, m))
    # the time encoder: the kernel test's bound, from the gradient of the message that reached the kernel
    (msg,) = seen
    g = msg.grad.cpu().numpy()[:, 2 * MEM + RAW:]
    _, _, dt, _, has = [a.cpu().numpy() for a in glx.tgn_message(
        mod.memory, mod.last_update, mod.pend_t, mod.pend_seq, mod.pend_other, mod.pend_raw,
        mod.time_enc.weight.detach(), mod.time_enc.bias.detach(), _cuda(torch, n_id))]
    assert has.sum() > 10 and has[-2:].tolist() == [0, 0]
    w, b = mod.time_enc.weight.detach().cpu().numpy(), mod.time_enc.bias.detach().cpu().numpy()
    want_w, want_b, scale, abs_w, abs_b, x = tref.time_gradients(g, dt, has, w, b)
    live = has != 0
    got = torch.sin(_cuda(torch, x[live].reshape(-1))).cpu().numpy()
    Es = max(tref.ulp_error(got, np.sin(x[live].astype(np.float64)).reshape(-1)), 1.0)
    D = glx.tgn_backward_depth(len(n_id))
    for p, want, abs_terms, name in ((mod.time_enc.weight, want_w, abs_w, "weight"), (mod.time_enc.bias, want_b, abs_b, "bias")):
        bound = tref.backward_bound(scale, x, has, abs_terms, Es, D)
        err = np.abs(p.grad.cpu().numpy().astype(np.float64) - want)
        print("time_enc.%s: Es %.2f, worst error / bound %.3g" % (name, Es, float(np.max(err / bound))))
        assert np.all(err <= bound) and float(np.abs(want).max()) > 0, name


def test_no_time_gradient_is_computed_when_none_is_needed(torch, thg):
    mod = _module(torch, thg, zero_time=False)
    mod.time_enc.weight.requires_grad_(False)
    mod.time_enc.bias.requires_grad_(False)
    z, _ = mod(_cuda(torch, np.arange(5, dtype=np.int64)))
    z.sum().backward()
    assert mod.time_enc.weight.grad is None and mod.time_enc.bias.grad is None and mod.gru.weight_ih.grad is not None


def test_state_dict_round_trip(torch, thg):
    stream = _stream()
    whole = _module(torch, thg, zero_time=False)
    for src, dst, t, raw in stream[:4]:
        whole.update_state(*[_cuda(torch, a) for a in (src, dst, t, raw)])
    state = copy.deepcopy(whole.state_dict())
    assert state["_extra_state"] == {"seq_base": 4 * EVENTS}
    for name in ("memory", "last_update", "pend_t", "pend_seq", "pend_other", "pend_raw"):
        assert name in state, name
    torch.manual_seed(99)
    fresh = thg.TGNMemory(NODES, RAW, MEM, TIME).cuda()
    fresh.load_state_dict(state)
    assert fresh.seq_base == 4 * EVENTS
    for m in (whole, fresh):
        m.update_state(*[_cuda(torch, a) for a in stream[4]])
    for name, a in whole.state_dict().items():
        b = fresh.state_dict()[name]
        assert (a == b) if name == "_extra_state" else np.array_equal(_bits(a), _bits(b)), name
    assert fresh.seq_base == 5 * EVENTS


def test_eval_forward_reads_zeros_for_ids_outside_the_table(torch, thg):
    mod = _module(torch, thg, zero_time=False)
    src, dst, t, raw = _stream()[0]
    mod.update_state(*[_cuda(torch, a) for a in (src, dst, t, raw)])
    mod.update_state(*[_cuda(torch, a) for a in (src, dst, t + 1000, raw)])  # the first batch's messages reach the memory
    mod.eval()
    v = int(src[-1])  # the batch's last event is this node's latest
    z, lu = mod(_cuda(torch, np.array([-1, v, NODES, v, np.iinfo(np.int64).max], np.int64)))
    assert not _bits(z[[0, 2, 4]]).any() and lu.tolist()[0::2] == [0, 0, 0]
    assert np.array_equal(_bits(z[1]), _bits(mod.memory[v])) and np.array_equal(_bits(z[3]), _bits(mod.memory[v]))
    assert int(lu[1]) == int(mod.last_update[v]) > 0 and float(z[1].abs().max()) > 0


def test_arguments_are_checked(torch, thg):
    mod = _module(torch, thg, zero_time=True)
    ids = _cuda(torch, np.arange(4, dtype=np.int64))
    with pytest.raises(ValueError):
        mod(ids.to(torch.int32))
    with pytest.raises(ValueError):
        mod(ids.cpu())
    with pytest.raises(ValueError):
        mod.update_state(ids, ids, ids, torch.zeros(4, RAW + 1, device="cuda"))
    with pytest.raises(ValueError):
        mod.update_state(ids, ids[:3], ids, torch.zeros(4, RAW, device="cuda"))
    with pytest.raises(ValueError):
        thg.TGNMemory(10, 3, 0, 4)


def test_example_runs_twice_to_the_same_bits():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_tgn
    history, leaked, same = train_tgn.main(epochs=1, events=3000, quiet=True)
    assert leaked == 0 and same
    for run in history:
        for losses, _ in run:
            assert len(losses) > 5 and np.all(np.isfinite(losses))
