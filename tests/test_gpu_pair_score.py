"""graphlearn.nn.pytorch.pair_dot: the torch.autograd surface of glx_pair_dot and glx_pair_dot_backward."""
import os
import subprocess
import sys

import numpy as np
import pytest

import glx
import pair_dot_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

B, K, D, NA, NB = 6, 5, 8, 7, 11


@pytest.fixture(scope="module")
def thg():
    import graphlearn.nn.pytorch as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _request(heads, seed=0, k=K):
    rng = np.random.default_rng(seed)
    xa = rng.standard_normal((NA, D)).astype(np.float32)
    xb = rng.standard_normal((NB, D)).astype(np.float32)
    ia = rng.integers(0, NA, B).astype(np.int64)
    ia[1] = ia[4] = 2  # one source behind two entries
    ib = rng.integers(0, min(NA, NB), (B, k)).astype(np.int64)  # in range for either table
    ib[0, :3] = 3  # one candidate several times
    g = rng.standard_normal((B, k, heads)).astype(np.float32)
    return xa, xb, ia, ib, g


def _torch_reference(xa, xb, ia, ib, g, heads):
    """(out, xa.grad, xb.grad) of torch autograd in float64 on the CPU"""
    import torch
    ta = torch.tensor(xa, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(xb, dtype=torch.float64, requires_grad=True)
    n, repeat = ib.size, ib.size // ia.size
    out = (ta[torch.tensor(ia)].repeat_interleave(repeat, 0) * tb[torch.tensor(ib.reshape(-1))]).view(n, heads, -1).sum(-1)
    out.backward(torch.tensor(g.reshape(n, heads), dtype=torch.float64))
    return out.detach().numpy(), ta.grad.numpy(), tb.grad.numpy()


@pytest.mark.parametrize("heads", [None, 2])
def test_against_float64_autograd(thg, heads):
    """The forward inside the contract's bound of the float64 composite; the gradients relative 1e-5 of the same
    autograd over the magnitudes (at most B * K = 30 float32 terms per element: 30 * 2^-24 < 1e-5) and equal to the
    restatement bit for bit"""
    H = heads or 1
    xa, xb, ia, ib, g = _request(H)
    x_a, x_b = _cuda(xa).requires_grad_(True), _cuda(xb).requires_grad_(True)
    out = thg.pair_dot(x_a, _cuda(ia), x_b, _cuda(ib), heads=heads)
    gt = _cuda(g if heads else g[..., 0])
    out.backward(gt)
    want = _torch_reference(xa, xb, ia, ib, g, H)
    scale = _torch_reference(np.abs(xa), np.abs(xb), ia, ib, np.abs(g), H)
    ref_out, bound = pref.forward(xa, ia, xb, ib, H, K)
    got_out = out.detach().cpu().numpy().reshape(B * K, H)
    assert np.all(np.abs(ref_out - want[0]) <= 1e-12 * scale[0])  # the restatement is the composite
    assert pref.within_bound(got_out, want[0], bound)
    ga, gb = x_a.grad.cpu().numpy(), x_b.grad.cpu().numpy()
    for got, t, m, name in ((ga, want[1], scale[1], "xa.grad"), (gb, want[2], scale[2], "xb.grad")):
        assert got.shape == t.shape, name
        assert np.all(np.abs(got.astype(np.float64) - t) <= 1e-5 * m), name
    assert pref.same_bits(ga, pref.backward(0, ia, ib, g, xb, NA, K))
    assert pref.same_bits(gb, pref.backward(1, ia, ib, g, xa, NB, K))
    assert np.any(ga != 0) and np.any(gb != 0)


@pytest.mark.parametrize("heads", [None, 4])
def test_one_table_on_both_sides_adds_the_two_gradients(thg, heads):
    """xa is xb: autograd adds side 0's and side 1's gradients -- one float32 add per element of the two restatements"""
    H = heads or 1
    xa, _, ia, ib, g = _request(H, seed=3)
    z = _cuda(xa).requires_grad_(True)
    out = thg.pair_dot(z, _cuda(ia), z, _cuda(ib), heads=heads)
    out.backward(_cuda(g if heads else g[..., 0]))
    want = pref.backward(0, ia, ib, g, xa, NA, K) + pref.backward(1, ia, ib, g, xa, NA, K)  # float32 + float32
    assert want.dtype == np.float32
    assert pref.same_bits(z.grad.cpu().numpy(), want)
    ref_out, bound = pref.forward(xa, ia, xa, ib, H, K)
    assert pref.within_bound(out.detach().cpu().numpy().reshape(B * K, H), ref_out, bound)


def test_only_the_needed_side_is_computed(thg, monkeypatch):
    import torch
    xa, xb, ia, ib, g = _request(1, seed=7)
    sides = []
    real = glx.pair_dot_backward
    monkeypatch.setattr(glx, "pair_dot_backward", lambda side, *a, **k: (sides.append(side), real(side, *a, **k))[1])
    full_a, full_b = _cuda(xa).requires_grad_(True), _cuda(xb).requires_grad_(True)
    full = thg.pair_dot(full_a, _cuda(ia), full_b, _cuda(ib))
    full.backward(_cuda(g[..., 0]))
    assert sorted(sides) == [0, 1]
    # only xa
    del sides[:]
    x_a, x_b = _cuda(xa).requires_grad_(True), _cuda(xb)
    out = thg.pair_dot(x_a, _cuda(ia), x_b, _cuda(ib))
    out.backward(_cuda(g[..., 0]))
    assert sides == [0] and x_b.grad is None
    assert torch.equal(x_a.grad, full_a.grad) and torch.equal(out, full)
    # only xb
    del sides[:]
    x_a, x_b = _cuda(xa), _cuda(xb).requires_grad_(True)
    thg.pair_dot(x_a, _cuda(ia), x_b, _cuda(ib)).backward(_cuda(g[..., 0]))
    assert sides == [1] and x_a.grad is None
    assert torch.equal(x_b.grad, full_b.grad)
    # neither: no graph at all
    del sides[:]
    out = thg.pair_dot(_cuda(xa), _cuda(ia), _cuda(xb), _cuda(ib))
    assert not out.requires_grad and sides == []


def test_output_shapes(thg):
    xa, xb, ia, ib, _ = _request(1)
    x_a, x_b, i_a, i_b = _cuda(xa), _cuda(xb), _cuda(ia), _cuda(ib)
    f = thg.pair_dot
    assert tuple(f(x_a, i_a, x_b, i_b).shape) == (B, K)                       # [B] against [B, K]
    assert tuple(f(x_a, i_a, x_b, i_b, heads=2).shape) == (B, K, 2)
    assert tuple(f(x_a, i_a, x_b, i_b[:, 0].contiguous()).shape) == (B,)      # edges one to one
    assert tuple(f(x_a, i_a, x_b, i_b[:, 0].contiguous(), heads=D).shape) == (B, D)
    assert tuple(f(x_a, i_a.view(2, 3), x_b, i_b.view(2, 3, K), heads=1).shape) == (2, 3, K, 1)
    assert tuple(f(x_a, i_a[:0], x_b, i_b[:0]).shape) == (0, K)               # nothing to score
    # heads = D: every column its own head -- the elementwise product of the two rows
    got = f(x_a, i_a, x_b, i_b[:, 0].contiguous(), heads=D).cpu().numpy()
    assert np.array_equal(got, xa[ia] * xb[ib[:, 0]])


def test_indices_outside_the_tables_read_the_default_row_and_get_no_gradient(thg):
    xa, xb, ia, ib, g = _request(2, seed=11)
    ia[0], ia[5], ib[2, 1], ib[0, 0], ib[3, 4] = -1, NA, NB, -1, NB + 5
    x_a, x_b = _cuda(xa).requires_grad_(True), _cuda(xb).requires_grad_(True)
    out = thg.pair_dot(x_a, _cuda(ia), x_b, _cuda(ib), heads=2, default_attr=0.5)
    out.backward(_cuda(g))
    ref_out, bound = pref.forward(xa, ia, xb, ib, 2, K, 0.5)
    assert pref.within_bound(out.detach().cpu().numpy().reshape(B * K, 2), ref_out, bound)
    assert pref.same_bits(x_a.grad.cpu().numpy(), pref.backward(0, ia, ib, g, xb, NA, K, 0.5))
    assert pref.same_bits(x_b.grad.cpu().numpy(), pref.backward(1, ia, ib, g, xa, NB, K, 0.5))


def test_value_errors(thg):
    import torch
    xa, xb, ia, ib, _ = _request(1)
    x_a, x_b, i_a, i_b = _cuda(xa), _cuda(xb), _cuda(ia), _cuda(ib)
    f = thg.pair_dot
    bad = [
        lambda: f(xa, i_a, x_b, i_b),                                   # xa not a tensor
        lambda: f(x_a, i_a, xb, i_b),                                   # xb not a tensor
        lambda: f(x_a.double(), i_a, x_b, i_b),                         # xa not float32
        lambda: f(x_a, i_a, x_b.half(), i_b),                           # xb not float32
        lambda: f(x_a.cpu(), i_a.cpu(), x_b, i_b),                      # xa not on the GPU
        lambda: f(x_a, i_a, x_b.cpu(), i_b.cpu()),                      # xb not on the GPU
        lambda: f(x_a[:, ::2], i_a, x_b[:, :4].contiguous(), i_b),      # xa not contiguous
        lambda: f(x_a, i_a, x_b.t(), i_b),                              # xb not contiguous
        lambda: f(x_a.view(-1), i_a, x_b, i_b),                         # xa not [N, D]
        lambda: f(x_a, i_a, x_b[:, :4].contiguous(), i_b),              # different numbers of columns
        lambda: f(x_a, i_a.int(), x_b, i_b),                            # ia not int64
        lambda: f(x_a, i_a, x_b, i_b.int()),                            # ib not int64
        lambda: f(x_a, i_a.cpu(), x_b, i_b),                            # ia on another device
        lambda: f(x_a, i_a, x_b, i_b.cpu()),                            # ib on another device
        lambda: f(x_a, ia, x_b, i_b),                                   # ia not a tensor
        lambda: f(x_a, i_a[:4], x_b, i_b),                              # 4 sources do not divide 30 candidates
        lambda: f(x_a, i_a[:0], x_b, i_b),                              # no source for 30 candidates
        lambda: f(x_a, i_a, x_b, i_b, heads=3),                         # heads do not divide D
        lambda: f(x_a, i_a, x_b, i_b, heads=0),
        lambda: f(x_a, i_a, x_b, i_b, heads=-2),
        lambda: f(x_a, i_a.float().requires_grad_(True), x_b, i_b),     # an index that wants a gradient (and is float)
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case {} raised nothing".format(i))
    assert torch.cuda.is_available()


def test_double_backward_is_refused(thg):
    import torch
    xa, xb, ia, ib, g = _request(1)
    x_a, x_b = _cuda(xa).requires_grad_(True), _cuda(xb).requires_grad_(True)
    out = thg.pair_dot(x_a, _cuda(ia), x_b, _cuda(ib))
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(out, [x_a, x_b], _cuda(g[..., 0]), create_graph=True)


def test_two_backward_passes_give_the_same_bits(thg):
    xa, _, ia, ib, g = _request(2, seed=5)
    grads = []
    for _ in range(2):
        z = _cuda(xa).requires_grad_(True)
        thg.pair_dot(z, _cuda(ia), z, _cuda(ib), heads=2).backward(_cuda(g))
        grads.append(z.grad.cpu().numpy())
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32))


def test_example_trains_and_repeats_its_losses():
    """examples/train_sage_unsup.py, one short epoch twice from one seed in a process of its own: the loss falls inside
    the epoch and the two runs print the same per-batch losses bit for bit"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_sage_unsup.py"), "1", "4096"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("run ")]
    assert len(lines) == 2, r.stdout[-2000:]
    first, second = (float(v) for v in lines[0].split("loss ")[1].split(" (")[0].split(" -> "))
    assert second < first, lines[0]
    bits = [ln.split("bits ")[1] for ln in lines]
    assert bits[0] == bits[1] and len(bits[0].split(",")) == 16, lines
    assert "the two runs' losses are the same bits" in r.stdout
