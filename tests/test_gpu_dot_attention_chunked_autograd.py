"""graphlearn.nn.pytorch.dot_attention(chunked=True) and TransformerConv(chunked=True): the torch.autograd surface of
glx_dot_attention_chunked and glx_dot_attention_backward_chunked.  The float64 restatement of the layer and its
magnitudes (_layer64) are test_gpu_transformer_conv.py's own, imported, not copied: that file is unchanged."""
import numpy as np
import pytest

import glx
from test_gpu_transformer_conv import EDGE, IN, OUT, _batch, _cuda, _layer64, thg  # noqa: F401  (thg: the fixture)

pytestmark = pytest.mark.gpu

DIM, HEADS, ROWS = 16, 4, 50


def _request(seed=0):
    """segments of 3, 700, 0 and 40 positions with an unconsumed tail; row 7 is named by 300 positions of the long
    segment, row -1 once"""
    rng = np.random.default_rng(seed)
    cnt = np.array([3, 700, 0, 40], np.int32)
    S, n = len(cnt), int(cnt.sum()) + 2
    q = rng.standard_normal((S, DIM)).astype(np.float32)
    k = rng.standard_normal((ROWS, DIM)).astype(np.float32)
    v = rng.standard_normal((ROWS, DIM)).astype(np.float32)
    rows = rng.integers(8, ROWS, n).astype(np.int64)
    rows[3 + rng.permutation(700)[:300]] = 7
    rows[1] = -1
    edge = rng.standard_normal((n, DIM)).astype(np.float32)
    g = rng.standard_normal((S, DIM)).astype(np.float32)
    return q, k, v, rows, edge, cnt, S, g


def test_forward_and_backward_are_the_chunked_entry_points(thg):
    import torch
    q, k, v, rows, edge, cnt, S, g = _request()
    kw = dict(heads=HEADS, drop_p=0.4, seed=5, call=6)
    dq, dk, dv, de = (_cuda(a).requires_grad_(True) for a in (q, k, v, edge))
    out = thg.dot_attention(dq, dk, dv, _cuda(rows), S, counts=_cuda(cnt), edge=de, heads=HEADS, dropout=0.4, seed=5,
                            call=6, chunked=True)
    out.backward(_cuda(g))
    want, soft, _ = glx.dot_attention(_cuda(q), _cuda(k), _cuda(v), _cuda(rows), cnt=_cuda(cnt), edge=_cuda(edge),
                                      chunked=True, **kw)
    assert torch.equal(out.detach(), want)
    _, gq, gk, gv, ge = glx.dot_attention_backward(soft, _cuda(g), _cuda(q), _cuda(k), _cuda(v), _cuda(rows),
                                                   cnt=_cuda(cnt), edge=_cuda(edge), chunked=True, **kw)
    for got, ref in ((dq.grad, gq), (dk.grad, gk), (dv.grad, gv), (de.grad, ge)):
        assert torch.equal(got, ref) and bool(got.abs().sum() > 0)
    # the flag changes the long segment and the long row, and nothing else
    plain, _, _ = glx.dot_attention(_cuda(q), _cuda(k), _cuda(v), _cuda(rows), cnt=_cuda(cnt), edge=_cuda(edge), **kw)
    assert torch.equal(want[[0, 2, 3]], plain[[0, 2, 3]]) and not torch.equal(want[1], plain[1])


def test_only_the_needed_gradients_are_computed(thg, monkeypatch):
    q, k, v, rows, edge, cnt, S, g = _request(1)
    asked = []
    real = glx.dot_attention_backward

    def spy(*args, **kw):
        asked.append((kw["want_q"], kw["want_k"], kw["want_v"], kw["want_edge"], kw["chunked"]))
        return real(*args, **kw)

    monkeypatch.setattr(glx, "dot_attention_backward", spy)
    cases = [(True, False, False, False), (False, True, False, False), (False, False, True, False),
             (False, False, False, True), (True, True, True, True)]
    for need in cases:
        ts = [_cuda(a).requires_grad_(w) for a, w in zip((q, k, v, edge), need)]
        thg.dot_attention(ts[0], ts[1], ts[2], _cuda(rows), S, counts=_cuda(cnt), edge=ts[3], heads=HEADS,
                          chunked=True).backward(_cuda(g))
        assert [t.grad is not None for t in ts] == list(need)
    assert asked == [need + (True,) for need in cases]


def test_double_backward_is_refused(thg):
    import torch
    q, k, v, rows, edge, cnt, S, g = _request(2)
    dq = _cuda(q).requires_grad_(True)
    out = thg.dot_attention(dq, _cuda(k), _cuda(v), _cuda(rows), S, counts=_cuda(cnt), heads=HEADS, chunked=True)
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(out, dq, _cuda(g), create_graph=True)


def _layers(thg, with_edge, **kw):
    """a chunked and a default TransformerConv with the same weights"""
    import torch
    layers = []
    for chunked in (True, False):
        torch.manual_seed(4)
        layers.append(thg.TransformerConv(IN, OUT, heads=3, dropout=0.4, edge_dim=EDGE if with_edge else None, seed=17,
                                          chunked=chunked, **kw).cuda())
    assert "chunked=True" in repr(layers[0]) and "chunked=False" in repr(layers[1])
    assert layers[0].chunked is True and layers[1].chunked is False
    return layers


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("with_edge", [True, False], ids=["edge", "plain"])
def test_without_hubs_the_layer_does_not_depend_on_the_flag(thg, with_edge, ragged):
    """training mode, dropout 0.4, the same masks: segments of at most 30 positions, no node named more than 256
    times"""
    import torch
    x, seed_local, index, counts, ea, S = _batch(ragged, seed=5)
    g = _cuda(np.random.default_rng(1).standard_normal((S, 3 * OUT)).astype(np.float32))
    outs = []
    for layer in _layers(thg, with_edge):
        layer.train()
        out = layer(x, seed_local, index, counts, ea if with_edge else None)
        out.backward(g)
        assert layer.calls == 1
        outs.append((out.detach(), {name: p.grad for name, p in layer.named_parameters()}))
    assert torch.equal(outs[0][0], outs[1][0])
    assert sorted(outs[0][1]) == sorted(outs[1][1])
    for name, grad in outs[0][1].items():
        assert torch.equal(grad, outs[1][1][name]) and bool(grad.abs().sum() > 0), name


def _hub_batch(seed=0):
    """9 seeds over 40 nodes; seed 4 has 700 neighbours, 300 of them node 11"""
    rng = np.random.default_rng(seed)
    nodes = 40
    x = rng.standard_normal((nodes, IN)).astype(np.float32)
    cnt = np.array([3, 0, 12, 1, 700, 30, 0, 2, 5], np.int32)
    S, n = len(cnt), int(cnt.sum())
    seed_local = rng.permutation(nodes)[:S].astype(np.int64)
    index = rng.integers(0, nodes, n).astype(np.int64)
    index[index == 11] = 12
    index[16 + rng.permutation(700)[:300]] = 11
    ea = rng.standard_normal((n, EDGE)).astype(np.float32)
    return x, seed_local, index, cnt, ea, S


@pytest.mark.parametrize("with_edge", [True, False], ids=["edge", "plain"])
def test_a_hub_seed_against_float64_autograd_of_the_whole_layer(thg, with_edge):
    """test_transformer_conv_against_float64_autograd_of_the_whole_layer's criterion -- out and the gradient of every
    parameter within 1e-5 of the float64 restatement over the magnitudes of their terms -- on a batch with one seed of
    700 neighbours, and the same bits on a second run"""
    import torch
    x, seed_local, index, cnt, ea, S = _hub_batch(3)
    layer = _layers(thg, with_edge)[0].eval()
    g = np.random.default_rng(9).standard_normal((S, 3 * OUT)).astype(np.float32)
    runs = []
    for _ in range(2):
        layer.zero_grad(set_to_none=True)
        got = layer(_cuda(x), _cuda(seed_local), _cuda(index), _cuda(cnt), _cuda(ea) if with_edge else None)
        got.backward(_cuda(g))
        runs.append((got.detach().clone(), {name: p.grad.clone() for name, p in layer.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for name, grad in runs[0][1].items():
        assert torch.equal(grad, runs[1][1][name]), name
    want, grads, mags, m_out = _layer64(layer, x, seed_local, index, cnt, ea if with_edge else None, S, g)
    diff = np.abs(runs[0][0].cpu().numpy().astype(np.float64) - want)
    assert diff.shape == want.shape and np.all(diff <= 1e-5 * m_out), diff.max()
    assert sorted(grads) == sorted(runs[0][1])
    for name, grad in runs[0][1].items():
        a = grad.cpu().numpy().astype(np.float64)
        assert a.shape == grads[name].shape and np.all(np.abs(a - grads[name]) <= 1e-5 * mags[name]), \
            (name, np.abs(a - grads[name]).max())
        assert np.any(a != 0), name
