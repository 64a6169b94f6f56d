"""graphlearn.nn.pytorch.gat_attention, the torch.autograd surface of glx_gat_attention and its gradients, and the
GATConv layer on top of it."""
import os
import sys

import numpy as np
import pytest

import gat_attention_ref as gref
import glx
from test_gat_attention_cpu import _request, magnitudes, torch_composite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def thg():
    import graphlearn.nn.pytorch as m
    return m


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("drop_p", [0.0, 0.4])
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("heads", [1, 3])
def test_against_float64_autograd(thg, heads, ragged, drop_p):
    """The coefficients inside the contract's bound of the restatement; the gradients relative 1e-5 of float64 CPU
    autograd of the composite over the magnitudes of their terms (segments of at most 40 terms: 42 * 2^-23 < 1e-5)"""
    s, t, rows, cnt, S, g = _request(heads, ragged, seed=heads)
    n, slope, seed, call = len(rows), 0.2, 11, 3
    ds, dt = _cuda(s).requires_grad_(True), _cuda(t).requires_grad_(True)
    if heads == 1:  # [S] and [M] instead of [S, 1] and [M, 1]
        ds, dt = _cuda(s[:, 0]).requires_grad_(True), _cuda(t[:, 0]).requires_grad_(True)
    alpha = thg.gat_attention(ds, dt, _cuda(rows), S, counts=_cuda(cnt), negative_slope=slope, dropout=drop_p,
                              seed=seed, call=call)
    assert tuple(alpha.shape) == (n, heads)
    alpha.backward(_cuda(g))
    keep = gref.keep_mask(n, heads, drop_p, seed, call)
    ks = np.where(keep, float(gref.scale(drop_p)), 0.0) if drop_p else np.ones((n, heads))
    want, bound, pre = gref.forward(s, t, rows, cnt, S, slope, 0.0)
    got = alpha.detach().cpu().numpy()
    assert gref.within_bound(got, want * ks, bound * ks + np.abs(want * ks) * 2.0 ** -24)
    _, _, want_gs, want_gt = torch_composite(s, t, rows, cnt, S, g, slope, 0.0, ks)
    _, ms, mt = magnitudes(want, gref.drop(g, keep, drop_p), pre, rows, cnt, S, len(t), slope)
    gs, gt = ds.grad.cpu().numpy().reshape(S, heads), dt.grad.cpu().numpy().reshape(len(t), heads)
    assert ds.grad.shape == ds.shape and dt.grad.shape == dt.shape
    assert np.all(np.abs(gs - want_gs) <= 1e-5 * ms) and np.all(np.abs(gt - want_gt) <= 1e-5 * mt)
    assert np.any(gs != 0) and np.any(gt != 0)


def test_only_the_needed_gradients_are_computed(thg, monkeypatch):
    import torch
    s, t, rows, cnt, S, g = _request(2, True)
    asked = []
    real = glx.gat_attention_backward

    def spy(*args, **kw):
        asked.append((kw["want_s"], kw["want_t"]))
        return real(*args, **kw)

    monkeypatch.setattr(glx, "gat_attention_backward", spy)
    for need_s, need_t in ((True, False), (False, True), (True, True)):
        ds, dt = _cuda(s).requires_grad_(need_s), _cuda(t).requires_grad_(need_t)
        thg.gat_attention(ds, dt, _cuda(rows), S, counts=_cuda(cnt)).backward(_cuda(g))
        assert (ds.grad is not None) == need_s and (dt.grad is not None) == need_t
    assert asked == [(True, False), (False, True), (True, True)]
    with torch.no_grad():
        out = thg.gat_attention(_cuda(s), _cuda(t), _cuda(rows), S, counts=_cuda(cnt))
    assert not out.requires_grad and len(asked) == 3


def test_double_backward_is_refused(thg):
    import torch
    s, t, rows, cnt, S, g = _request(2, True)
    ds, dt = _cuda(s).requires_grad_(True), _cuda(t).requires_grad_(True)
    alpha = thg.gat_attention(ds, dt, _cuda(rows), S, counts=_cuda(cnt))
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(alpha, ds, _cuda(g), create_graph=True)


def test_bad_inputs_raise_value_error(thg):
    import torch
    s, t, rows, cnt, S, g = _request(2, True)
    ds, dt, dr, dc = _cuda(s), _cuda(t), _cuda(rows), _cuda(cnt)
    good = dict(s=ds, t=dt, index=dr, num_segments=S, counts=dc)
    bad = [
        dict(s=s), dict(t=t), dict(s=ds.double()), dict(t=dt.half()), dict(s=ds.cpu()), dict(t=dt.cpu()),
        dict(s=ds.t().contiguous().t()), dict(t=dt[:, :1]), dict(s=ds[:, :1].contiguous()),
        dict(s=ds.reshape(S, 2, 1)), dict(index=dr.int()), dict(index=dr.cpu()), dict(index=rows),
        dict(num_segments=S - 1), dict(num_segments=-1), dict(counts=dc.long()), dict(counts=dc.cpu()),
        dict(counts=dc[:-1]), dict(counts=dc.reshape(1, -1)), dict(counts=None),  # n is no multiple of S
        dict(negative_slope=-0.5), dict(negative_slope=float("inf")), dict(negative_slope=float("nan")),
        dict(dropout=1.0), dict(dropout=-0.1), dict(dropout=float("nan")), dict(seed=-1), dict(call=2 ** 64),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            thg.gat_attention(**dict(good, **change))
    with pytest.raises(ValueError):
        thg.gat_attention(ds[:0], dt, dr[:0], 0)  # the implied layout needs a segment
    assert thg.gat_attention(**good).shape == (len(rows), 2)
    assert torch.equal(thg.gat_attention(ds, dt, dr.reshape(-1, 1), S, counts=dc), thg.gat_attention(**good))


# ---- GATConv ---------------------------------------------------------------------------------------------------

IN, OUT, NODES = 12, 5, 40


def _batch(ragged, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((NODES, IN)).astype(np.float32)
    S = 9
    seed_local = rng.permutation(NODES)[:S].astype(np.int64)
    if ragged:
        cnt = np.array([3, 0, 12, 1, 7, 30, 0, 2, 5], np.int32)
        n = int(cnt.sum())
    else:
        cnt, n = None, S * 6
    index = rng.integers(0, NODES, n).astype(np.int64)
    return _cuda(x), _cuda(seed_local), _cuda(index), _cuda(cnt), S


def _composite(thg, layer, x, seed_local, index, counts, S):
    """the layer in eval mode out of the ops that existed before it -> (out, tolerance): the two paths compute the
    same logits bit for bit, so their coefficients differ by at most twice the softmax bound b_p, and the weighted
    sums of k terms by sum_p 2 b_p |z_p| plus the (k + 2) * 2^-23 * sum_p alpha_p |z_p| of two float32 folds"""
    import torch
    import segment_softmax_ref as sref
    H, C = layer.num_heads, layer.out_dim
    z = layer.linear(x)
    zh = z.view(-1, H, C)
    src_e = (zh * layer.attn_src).sum(-1).contiguous()
    dst_e = (zh * layer.attn_dst).sum(-1).contiguous()
    if layer.add_self_loops:
        index, counts = layer.with_self_loops(seed_local, index, counts, S)
    n = index.numel()
    if counts is None:
        seg = torch.arange(S, device=x.device).repeat_interleave(n // S)
    else:
        seg = torch.repeat_interleave(torch.arange(S, device=x.device), counts.long(), output_size=n)
    e = torch.nn.functional.leaky_relu(thg.gather_rows(src_e, seed_local[seg]) + thg.gather_rows(dst_e, index),
                                       layer.negative_slope).contiguous()
    alpha = thg.segment_softmax(e, S, counts=counts)
    out = thg.weighted_segment_aggregate(z, index, alpha, S, counts=counts)
    cnt = None if counts is None else counts.cpu().numpy()
    a64, b = sref.forward(e.detach().cpu().numpy(), cnt, S)
    zabs = np.abs(z.detach().cpu().numpy().astype(np.float64))[index.cpu().numpy()].reshape(n, H, C)
    start = sref.starts(cnt, n, S)
    tol = np.zeros((S, H, C))
    for sg in range(S):
        lo, hi = int(start[sg]), int(start[sg + 1])
        tol[sg] = ((2 * b[lo:hi, :, None] + (hi - lo + 2) * 2.0 ** -23 * a64[lo:hi, :, None]) * zabs[lo:hi]).sum(0)
    if layer.concat:
        return out, tol.reshape(S, H * C) + 2.0 ** -126, index, counts
    # the mean over the heads: H - 1 additions and a division of float32 terms
    mean_tol = (H + 1) * 2.0 ** -24 * np.abs(out.view(S, H, C).cpu().numpy().astype(np.float64)).mean(1)
    return out.view(S, H, C).mean(1), tol.mean(1) + mean_tol + 2.0 ** -126, index, counts


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("loops", [True, False], ids=["self_loops", "no_self_loops"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
def test_gat_conv_in_eval_mode_is_the_composite_of_the_existing_ops(thg, concat, loops, ragged):
    import torch
    torch.manual_seed(1)
    x, seed_local, index, counts, S = _batch(ragged)
    layer = thg.GATConv(IN, OUT, num_heads=3, concat=concat, dropout=0.4, use_bias=True, add_self_loops=loops).cuda().eval()
    with torch.no_grad():
        layer.bias.copy_(torch.randn_like(layer.bias))
        got = layer(x, seed_local, index, counts)
        want, tol, index2, counts2 = _composite(thg, layer, x, seed_local, index, counts, S)
        tol = tol + (np.abs(want.cpu().numpy()) + np.abs(layer.bias.cpu().numpy())) * 2.0 ** -23  # the bias: one add
        want = want + layer.bias
    assert tuple(got.shape) == (S, 3 * OUT if concat else OUT) and layer.bias.shape == (got.shape[1],)
    diff = np.abs(got.cpu().numpy().astype(np.float64) - want.cpu().numpy())
    assert np.all(diff <= tol), diff.max()
    assert layer.calls == 0  # eval mode draws no mask
    assert torch.equal(got, layer(x, seed_local, index, counts))
    if loops:  # every seed's own row is the last position of its segment
        k = (index.numel() // S if counts is None else counts.long()) + torch.zeros(S, dtype=torch.long, device="cuda")
        ends = torch.cumsum(k + 1, 0)
        assert index2.numel() == index.numel() + S and torch.equal(index2[ends - 1], seed_local)
        assert counts is None or torch.equal(counts2.long(), k + 1)
        keep = torch.ones(index2.numel(), dtype=torch.bool, device="cuda")
        keep[ends - 1] = False
        assert torch.equal(index2[keep], index)
    elif ragged:  # a seed without neighbours and without a self loop aggregates nothing: the bias alone
        empty = counts == 0
        assert bool(empty.any()) and torch.equal(got[empty], layer.bias.expand(int(empty.sum()), -1))


def _train(thg, steps=3):
    import torch
    torch.manual_seed(5)
    x, seed_local, index, counts, S = _batch(True, seed=2)
    layer = thg.GATConv(IN, OUT, num_heads=2, concat=True, dropout=0.4, use_bias=True).cuda().train()
    opt = torch.optim.SGD(layer.parameters(), lr=0.1)
    target = torch.randn(S, 2 * OUT, device="cuda")
    losses = []
    for _ in range(steps):
        loss = ((layer(x, seed_local, index, counts) - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return layer, losses


def test_two_training_runs_with_dropout_give_identical_parameters(thg):
    import torch
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        (a, la), (b, lb) = _train(thg), _train(thg)
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    assert a.calls == 3 and b.calls == 3 and [x.hex() for x in la] == [x.hex() for x in lb]
    for (name, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), name
        assert pa.grad is not None and bool(pa.grad.abs().sum() > 0), name
    # the mask is drawn, and another step draws another one
    x, seed_local, index, counts, S = _batch(True, seed=2)
    with torch.no_grad():
        one, two = a(x, seed_local, index, counts), a(x, seed_local, index, counts)
        quiet = a.eval()(x, seed_local, index, counts)
    assert a.calls == 3 + 2 and not torch.equal(one, two) and not torch.equal(one, quiet)


def test_state_dict_round_trip(thg):
    import torch
    torch.manual_seed(3)
    x, seed_local, index, counts, S = _batch(True)
    a = thg.GATConv(IN, OUT, num_heads=2, use_bias=True).cuda().eval()
    state = a.state_dict()
    assert sorted(state) == ["attn_dst", "attn_src", "bias", "linear.weight"]
    b = thg.GATConv(IN, OUT, num_heads=2, use_bias=True).cuda().eval()
    b.load_state_dict({k: v.clone() for k, v in state.items()})
    with torch.no_grad():
        assert torch.equal(a(x, seed_local, index, counts), b(x, seed_local, index, counts))
    assert sorted(thg.GATConv(IN, OUT).state_dict()) == ["attn_dst", "attn_src", "linear.weight"]
