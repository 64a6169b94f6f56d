"""graphlearn.nn.pytorch.weighted_segment_aggregate: the torch.autograd surface of glx_aggregate_weighted and its two
gradients."""
import os
import subprocess
import sys

import numpy as np
import pytest

import agg_weighted_ref as wref
import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

S, K, D, N = 5, 7, 8, 11


@pytest.fixture(scope="module")
def thg():
    import graphlearn.nn.pytorch as m
    return m


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _request(heads, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    index = rng.integers(0, N, S * K).astype(np.int64)
    index[:4] = 3  # one row referenced several times
    w = rng.standard_normal((S * K, heads)).astype(np.float32)
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    return X, index, w, grad_out


def _torch_reference(X, index, w, grad_out, op):
    """(out, x.grad, w.grad) of torch autograd in float64 on the CPU"""
    import torch
    x = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    C = D // w.shape[1]
    out = (x[torch.tensor(index)] * wt.repeat_interleave(C, 1)).view(S, K, D).sum(1)
    if op == "mean":
        out = out / K
    out.backward(torch.tensor(grad_out, dtype=torch.float64))
    return out.detach().numpy(), x.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("heads", [1, 2])
def test_against_float64_autograd(thg, heads, op):
    """Relative 1e-5: every element is a float32 sum of at most 64 products (7 per output, 8 or 4 per weight gradient,
    at most S * K = 35 per row gradient), whose error is below 64 * 2^-24 < 1e-5 of the sum of the terms' magnitudes
    -- which is what the same autograd computes from |x|, |w| and |grad_out|"""
    X, index, w, grad_out = _request(heads)
    x, wt = _cuda(X).requires_grad_(True), _cuda(w).requires_grad_(True)
    out = thg.weighted_segment_aggregate(x, _cuda(index).view(S, K), wt, S, op=op)
    out.backward(_cuda(grad_out))
    want = _torch_reference(X, index, w, grad_out, op)
    scale = _torch_reference(np.abs(X), index, np.abs(w), np.abs(grad_out), op)
    got = (out.detach().cpu().numpy(), x.grad.cpu().numpy(), wt.grad.cpu().numpy())
    for g, t, m, name in zip(got, want, scale, ("out", "x.grad", "w.grad")):
        assert g.shape == t.shape, name
        assert np.all(np.abs(g.astype(np.float64) - t) <= 1e-5 * m), name
    assert np.any(got[1] != 0) and np.any(got[2] != 0)
    # the engine's own restatement: bit for bit where the contract is
    assert wref.same_bits(got[0], wref.forward(wref.SUM if op == "sum" else wref.MEAN, X, index, w, None, S))


def test_one_dimensional_weights_keep_their_shape(thg):
    X, index, w, grad_out = _request(1, seed=2)
    x, wt = _cuda(X).requires_grad_(True), _cuda(w[:, 0]).requires_grad_(True)
    out = thg.weighted_segment_aggregate(x, _cuda(index), wt, S)
    out.backward(_cuda(grad_out))
    assert tuple(wt.grad.shape) == (S * K,)
    want, bound = wref.backward_w(wref.SUM, X, index, 1, None, grad_out)
    assert wref.within_bound(wt.grad.cpu().numpy()[:, None], want, bound)
    assert wref.same_bits(x.grad.cpu().numpy(), wref.backward_x(wref.SUM, index, w, None, grad_out, N))


@pytest.mark.parametrize("op", ["sum", "mean"])
def test_two_identical_calls_give_the_same_bits(thg, op):
    X, index, w, grad_out = _request(2, seed=5)
    grads = []
    for _ in range(2):
        x, wt = _cuda(X).requires_grad_(True), _cuda(w).requires_grad_(True)
        thg.weighted_segment_aggregate(x, _cuda(index), wt, S, op=op).backward(_cuda(grad_out))
        grads.append((x.grad.cpu().numpy(), wt.grad.cpu().numpy()))
    assert np.array_equal(grads[0][0].view(np.uint32), grads[1][0].view(np.uint32))
    assert np.array_equal(grads[0][1].view(np.uint32), grads[1][1].view(np.uint32))


def test_only_the_needed_gradients_are_computed(thg, monkeypatch):
    import torch
    X, index, w, grad_out = _request(2, seed=7)
    calls = []
    for name in ("aggregate_weighted_backward_x", "aggregate_weighted_backward_w"):
        real = getattr(glx, name)
        monkeypatch.setattr(glx, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    full_x, full_w = _cuda(X).requires_grad_(True), _cuda(w).requires_grad_(True)
    thg.weighted_segment_aggregate(full_x, _cuda(index), full_w, S).backward(_cuda(grad_out))
    assert sorted(calls) == ["aggregate_weighted_backward_w", "aggregate_weighted_backward_x"]
    # only x
    del calls[:]
    x, wt = _cuda(X).requires_grad_(True), _cuda(w)
    thg.weighted_segment_aggregate(x, _cuda(index), wt, S).backward(_cuda(grad_out))
    assert calls == ["aggregate_weighted_backward_x"] and wt.grad is None
    assert torch.equal(x.grad, full_x.grad)
    # only w
    del calls[:]
    x, wt = _cuda(X), _cuda(w).requires_grad_(True)
    thg.weighted_segment_aggregate(x, _cuda(index), wt, S).backward(_cuda(grad_out))
    assert calls == ["aggregate_weighted_backward_w"] and x.grad is None
    assert torch.equal(wt.grad, full_w.grad)
    # neither: no graph at all
    del calls[:]
    out = thg.weighted_segment_aggregate(_cuda(X), _cuda(index), _cuda(w), S)
    assert not out.requires_grad and calls == []


@pytest.mark.parametrize("op", ["sum", "mean"])
def test_counts_path(thg, op):
    X, index, w, grad_out = _request(2, seed=9)
    cnt = np.array([0, 10, 1, 0, 20], np.int32)  # 31 of 35 consumed
    x, wt = _cuda(X).requires_grad_(True), _cuda(w).requires_grad_(True)
    out = thg.weighted_segment_aggregate(x, _cuda(index), wt, S, op=op, counts=_cuda(cnt), default_attr=0.75)
    out.backward(_cuda(grad_out))
    o = wref.SUM if op == "sum" else wref.MEAN
    assert wref.same_bits(out.detach().cpu().numpy(), wref.forward(o, X, index, w, cnt, S, 0.75))
    assert wref.same_bits(x.grad.cpu().numpy(), wref.backward_x(o, index, w, cnt, grad_out, N))
    want, bound = wref.backward_w(o, X, index, 2, cnt, grad_out, 0.75)
    gw = wt.grad.cpu().numpy()
    assert wref.within_bound(gw, want, bound)
    assert not gw[31:].any()


def test_value_errors(thg):
    import torch
    X, index, w, _ = _request(2)
    x, idx, wt = _cuda(X), _cuda(index), _cuda(w)
    cnt = _cuda(np.full(S, K, np.int32))
    f = thg.weighted_segment_aggregate
    bad = [
        lambda: f(X, idx, wt, S),                                  # x not a tensor
        lambda: f(x.double(), idx, wt, S),                         # x not float32
        lambda: f(x.cpu(), idx.cpu(), wt.cpu(), S),                # x not on the GPU
        lambda: f(x[:, ::2], idx, wt[:, :1], S),                   # x not contiguous
        lambda: f(x, idx.int(), wt, S),                            # index not int64
        lambda: f(x, idx.cpu(), wt, S),                            # index on another device
        lambda: f(x, idx, w, S),                                   # weights not a tensor
        lambda: f(x, idx, wt.double(), S),                         # weights not float32
        lambda: f(x, idx, wt.cpu(), S),                            # weights on another device
        lambda: f(x, idx, wt[:-1], S),                             # one weight row short
        lambda: f(x, idx, wt.view(S, K, 2), S),                    # weights of three dimensions
        lambda: f(x, idx, torch.ones((S * K, 3), device="cuda"), S),  # heads do not divide D
        lambda: f(x, idx, wt, S, op="max"),
        lambda: f(x, idx, wt, S, op="min"),
        lambda: f(x, idx, wt, S, op="prod"),
        lambda: f(x, idx, wt, -1),
        lambda: f(x, idx, wt, 0),                                  # implied layout without segments
        lambda: f(x, idx, wt, 4),                                  # 35 positions do not divide into 4 segments
        lambda: f(x, idx, wt, S, counts=cnt.long()),               # counts not int32
        lambda: f(x, idx, wt, S, counts=cnt.cpu()),                # counts on another device
        lambda: f(x, idx, wt, S, counts=cnt[:-1]),                 # one count short
        lambda: f(x, idx, wt, S, counts=cnt.tolist()),             # counts not a tensor
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case {} raised nothing".format(i))


def test_double_backward_is_refused(thg):
    import torch
    X, index, w, grad_out = _request(1)
    x, wt = _cuda(X).requires_grad_(True), _cuda(w).requires_grad_(True)
    out = thg.weighted_segment_aggregate(x, _cuda(index), wt, S)
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(out, [x, wt], _cuda(grad_out), create_graph=True)


def test_example_trains_and_repeats_its_losses():
    """examples/train_gat_dedup.py, one short epoch twice from one seed in a process of its own: the loss falls inside
    the epoch and the two runs print the same per-batch losses bit for bit"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_gat_dedup.py"), "1", "4096"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("run ")]
    assert len(lines) == 2, r.stdout[-2000:]
    first, second = (float(v) for v in lines[0].split("loss ")[1].split(" (")[0].split(" -> "))
    assert second < first, lines[0]
    bits = [ln.split("bits ")[1] for ln in lines]
    assert bits[0] == bits[1] and len(bits[0].split(",")) == 8, lines
    assert "the two runs' losses are the same bits" in r.stdout
