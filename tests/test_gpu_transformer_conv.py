"""graphlearn.nn.pytorch.dot_attention, the torch.autograd surface of glx_dot_attention and its gradients, and the
TransformerConv layer on top of it."""
import os
import sys

import numpy as np
import pytest

import dot_attention_ref as dref
import glx

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


def _request(heads, ragged, with_edge, seed=0):
    """segments of at most 12 positions, C = 4 columns to a head, rows outside the table and an unconsumed tail"""
    rng = np.random.default_rng(seed)
    M, D = 23, 4 * heads
    if ragged:
        cnt = np.array([0, 5, 1, 12, -3, 9, 0], np.int32)
        S, n = len(cnt), int(np.maximum(cnt, 0).sum()) + 3
    else:
        cnt, S, n = None, 9, 9 * 7
    q = rng.standard_normal((S, D)).astype(np.float32)
    k = rng.standard_normal((M, D)).astype(np.float32)
    v = rng.standard_normal((M, D)).astype(np.float32)
    rows = rng.integers(0, M, n).astype(np.int64)
    rows[::11] = -1
    edge = rng.standard_normal((n, D)).astype(np.float32) if with_edge else None
    g = rng.standard_normal((S, D)).astype(np.float32)
    return q, k, v, rows, edge, cnt, S, g


def attention64(tq, tk, tv, te, rows, cnt, S, heads, scale, default_attr, keep_scale):
    """out [S, D] of float64 CPU torch tensors, plain torch: gather, add the edge term, per-head dot products, softmax
    over each segment, keep_scale[n, H] on the coefficients, weighted sum"""
    import torch
    n, D = len(rows), tq.shape[1]
    C = D // heads
    inside = torch.tensor((rows >= 0) & (rows < len(tk)))
    at = torch.tensor(np.clip(rows, 0, len(tk) - 1))
    fill = torch.tensor(float(default_attr), dtype=torch.float64)
    kk = torch.where(inside[:, None], tk[at], fill)
    vv = torch.where(inside[:, None], tv[at], fill)
    if te is not None:
        kk, vv = kk + te, vv + te
    start = dref.starts(cnt, n, S)
    ks = torch.tensor(keep_scale, dtype=torch.float64)
    outs = []
    for sg in range(S):
        a, b = int(start[sg]), int(start[sg + 1])
        if a == b:
            outs.append(torch.zeros(D, dtype=torch.float64))
            continue
        e = (kk[a:b] * tq[sg]).view(b - a, heads, C).sum(2) * float(scale)
        alpha = torch.softmax(e, 0) * ks[a:b]
        outs.append((alpha[:, :, None] * vv[a:b].view(b - a, heads, C)).sum(0).reshape(D))
    return torch.stack(outs)


def torch_composite(q, k, v, rows, edge, cnt, S, g, heads, scale, default_attr, keep_scale):
    """(out, grad_q, grad_k, grad_v, grad_edge) of float64 CPU autograd of the plain-torch composite"""
    import torch
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)  # noqa: E731
    tq, tk, tv = t64(q), t64(k), t64(v)
    te = None if edge is None else t64(edge)
    out = attention64(tq, tk, tv, te, rows, cnt, S, heads, scale, default_attr, keep_scale)
    (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return (out.detach().numpy(), tq.grad.numpy(), tk.grad.numpy(), tv.grad.numpy(),
            None if te is None else te.grad.numpy())


def magnitudes(q, k, v, rows, edge, cnt, S, g, heads, scale, default_attr, keep_scale):
    """sum |terms| behind each element of out and of the four gradients, from the float64 restatement: a position
    contributes alpha |vv| to out, |soft| (|ga| + sum |soft ga|) |scale| to grad_e with |ga| <= keep_scale sum_c |go vv|"""
    n, D = len(rows), q.shape[1]
    C = D // heads
    kk = np.abs(dref.gathered(k, rows, edge, default_attr, np.float64))
    vv = np.abs(dref.gathered(v, rows, edge, default_attr, np.float64))
    _, soft, alpha = dref.forward64(q, k, v, rows, edge, cnt, S, heads, scale, default_attr, keep_scale)
    seg = dref.segment_of(cnt, n, S)
    used = seg < S
    aq, ag = np.abs(q.astype(np.float64)), np.abs(g.astype(np.float64))
    start = dref.starts(cnt, n, S)
    ga = np.zeros((n, heads))
    ga[used] = (ag[seg[used]] * vv[used]).reshape(-1, heads, C).sum(2) * keep_scale[used]
    me = np.zeros((n, heads))
    m_out, m_q = np.zeros((S, D)), np.zeros((S, D))
    for sg in range(S):
        a, b = int(start[sg]), int(start[sg + 1])
        me[a:b] = soft[a:b] * (ga[a:b] + (soft[a:b] * ga[a:b]).sum(0)) * abs(float(scale))
        m_out[sg] = (np.repeat(alpha[a:b], C, 1) * vv[a:b]).sum(0)
        m_q[sg] = (np.repeat(me[a:b], C, 1) * kk[a:b]).sum(0)
    mkk, mvv = np.zeros((n, D)), np.zeros((n, D))
    mkk[used] = np.repeat(me[used], C, 1) * aq[seg[used]]
    mvv[used] = np.repeat(alpha[used], C, 1) * ag[seg[used]]
    m_k, m_v = np.zeros(k.shape), np.zeros(v.shape)
    inside = used & (rows >= 0) & (rows < len(k))
    np.add.at(m_k, rows[inside], mkk[inside])
    np.add.at(m_v, rows[inside], mvv[inside])
    return m_out, m_q, m_k, m_v, mkk + mvv


@pytest.mark.parametrize("drop_p", [0.0, 0.4])
@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("heads", [1, 3])
def test_against_float64_autograd(thg, heads, ragged, with_edge, drop_p):
    """out and the gradients relative 1e-5 of float64 CPU autograd of the composite over the magnitudes of their terms
    (test_gpu_gat_conv's criterion: there a segment of at most 40 terms gives 42 * 2^-23 < 1e-5; here a segment has at
    most 12 positions of C = 4 columns and the chain is three stages long -- logit, softmax, fold -- each within
    (k + C + 2) * 2^-23 = 2.1e-6 of its terms to first order)"""
    q, k, v, rows, edge, cnt, S, g = _request(heads, ragged, with_edge, seed=heads)
    n, seed, call, da = len(rows), 11, 3, 0.25
    scale = float(dref.default_scale(q.shape[1], heads))
    dq, dk, dv = (_cuda(a).requires_grad_(True) for a in (q, k, v))
    de = None if edge is None else _cuda(edge).requires_grad_(True)
    out = thg.dot_attention(dq, dk, dv, _cuda(rows), S, counts=_cuda(cnt), edge=de, heads=heads, dropout=drop_p,
                            seed=seed, call=call, default_attr=da)
    assert tuple(out.shape) == (S, q.shape[1])
    out.backward(_cuda(g))
    keep = dref.keep_mask(n, heads, drop_p, seed, call)
    ks = np.where(keep, float(dref.gref.scale(drop_p)), 0.0) if drop_p else np.ones((n, heads))
    want = torch_composite(q, k, v, rows, edge, cnt, S, g, heads, scale, da, ks)
    mags = magnitudes(q, k, v, rows, edge, cnt, S, g, heads, scale, da, ks)
    got = [out.detach(), dq.grad, dk.grad, dv.grad, None if de is None else de.grad]
    for name, a, b, m in zip(("out", "grad_q", "grad_k", "grad_v", "grad_edge"), got, want, mags):
        if b is None:
            assert a is None
            continue
        a = a.cpu().numpy().astype(np.float64)
        assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-5 * m), (name, np.abs(a - b).max())
        assert np.any(a != 0), name


def test_key_and_value_in_one_tensor(thg):
    """autograd adds the two gradients: one more float32 add per element"""
    q, k, v, rows, edge, cnt, S, g = _request(2, True, True, seed=4)
    dq, dk = _cuda(q).requires_grad_(True), _cuda(k).requires_grad_(True)
    thg.dot_attention(dq, dk, dk, _cuda(rows), S, counts=_cuda(cnt), edge=_cuda(edge), heads=2).backward(_cuda(g))
    k1, k2 = _cuda(k).requires_grad_(True), _cuda(k).requires_grad_(True)
    thg.dot_attention(_cuda(q), k1, k2, _cuda(rows), S, counts=_cuda(cnt), edge=_cuda(edge), heads=2).backward(_cuda(g))
    import torch
    assert torch.equal(dk.grad, k1.grad + k2.grad) and bool(dk.grad.abs().sum() > 0)


def test_only_the_needed_gradients_are_computed(thg, monkeypatch):
    import torch
    q, k, v, rows, edge, cnt, S, g = _request(2, True, True)
    asked = []
    real = glx.dot_attention_backward

    def spy(*args, **kw):
        asked.append((kw["want_q"], kw["want_k"], kw["want_v"], kw["want_edge"]))
        return real(*args, **kw)

    monkeypatch.setattr(glx, "dot_attention_backward", spy)
    cases = [(True, False, False, False), (False, True, False, False), (False, False, True, False),
             (False, False, False, True), (True, True, True, True)]
    for need in cases:
        ts = [_cuda(a).requires_grad_(w) for a, w in zip((q, k, v, edge), need)]
        thg.dot_attention(ts[0], ts[1], ts[2], _cuda(rows), S, counts=_cuda(cnt), edge=ts[3], heads=2).backward(_cuda(g))
        assert [t.grad is not None for t in ts] == list(need)
    assert asked == cases
    with torch.no_grad():
        out = thg.dot_attention(_cuda(q), _cuda(k), _cuda(v), _cuda(rows), S, counts=_cuda(cnt), heads=2)
    assert not out.requires_grad and len(asked) == len(cases)


def test_double_backward_is_refused(thg):
    import torch
    q, k, v, rows, edge, cnt, S, g = _request(2, True, False)
    dq = _cuda(q).requires_grad_(True)
    out = thg.dot_attention(dq, _cuda(k), _cuda(v), _cuda(rows), S, counts=_cuda(cnt), heads=2)
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(out, dq, _cuda(g), create_graph=True)


def test_bad_inputs_raise_value_error(thg):
    import torch
    q, k, v, rows, edge, cnt, S, g = _request(2, True, True)
    dq, dk, dv, dr, de, dc = _cuda(q), _cuda(k), _cuda(v), _cuda(rows), _cuda(edge), _cuda(cnt)
    good = dict(q=dq, k=dk, v=dv, index=dr, num_segments=S, counts=dc, edge=de, heads=2)
    bad = [
        dict(q=q), dict(k=k), dict(v=v), dict(edge=edge), dict(q=dq.double()), dict(k=dk.half()), dict(q=dq.cpu()),
        dict(v=dv.cpu()), dict(edge=de.cpu()), dict(q=dq.t().contiguous().t()), dict(k=dk[:, :4]), dict(v=dv[:-1]),
        dict(q=dq.reshape(S, 2, 4)), dict(edge=de[:-1]), dict(edge=de[:, :4].contiguous()), dict(heads=3), dict(heads=0),
        dict(index=dr.int()), dict(index=dr.cpu()), dict(index=rows), dict(num_segments=S - 1), dict(num_segments=-1),
        dict(counts=dc.long()), dict(counts=dc.cpu()), dict(counts=dc[:-1]), dict(counts=dc.reshape(1, -1)),
        dict(counts=None),  # n is no multiple of S
        dict(scale=float("inf")), dict(scale=float("nan")), dict(dropout=1.0), dict(dropout=-0.1),
        dict(dropout=float("nan")), dict(seed=-1), dict(call=2 ** 64),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            thg.dot_attention(**dict(good, **change))
    with pytest.raises(ValueError):
        thg.dot_attention(dq[:0], dk, dv, dr[:0], 0, heads=2)  # the implied layout needs a segment
    assert thg.dot_attention(**good).shape == (S, 8)
    assert torch.equal(thg.dot_attention(**dict(good, index=dr.reshape(-1, 1))), thg.dot_attention(**good))
    assert torch.equal(thg.dot_attention(**dict(good, scale=0.5)), thg.dot_attention(**dict(good, scale=None)))  # C = 4


# ---- TransformerConv -------------------------------------------------------------------------------------------

IN, OUT, EDGE, NODES = 12, 4, 3, 40


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
    ea = rng.standard_normal((n, EDGE)).astype(np.float32)
    return _cuda(x), _cuda(seed_local), _cuda(index), _cuda(cnt), _cuda(ea), S


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("with_edge", [True, False], ids=["edge", "plain"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
def test_transformer_conv_in_eval_mode_is_the_composite_of_the_existing_ops(thg, concat, with_edge, ragged):
    """given the engine's own soft (held to the contract's bound in test_gpu_dot_attention.py), out is
    weighted_segment_aggregate of the materialised v[index] + edge, bit for bit"""
    import torch
    torch.manual_seed(1)
    x, seed_local, index, counts, ea, S = _batch(ragged)
    H = 3
    layer = thg.TransformerConv(IN, OUT, heads=H, concat=concat, dropout=0.4, edge_dim=EDGE if with_edge else None)
    layer = layer.cuda().eval()
    n = index.numel()
    with torch.no_grad():
        got = layer(x, seed_local, index, counts, ea if with_edge else None)
        q = thg.gather_rows(layer.lin_query(x), seed_local)
        k, v = layer.lin_key(x), layer.lin_value(x)
        edge = layer.lin_edge(ea) if with_edge else None
        _, soft, _ = glx.dot_attention(q, k, v, index, cnt=counts, edge=edge, heads=H)
        vv = thg.gather_rows(v, index)
        if with_edge:
            vv = vv + edge
        every = torch.arange(n, device="cuda")
        want = thg.weighted_segment_aggregate(vv.contiguous(), every, soft, S, counts=counts)  # empty: default_attr 0.0
        if not concat:
            want = want.view(S, H, OUT).mean(1)
        want = want + thg.gather_rows(layer.lin_skip(x), seed_local)
    assert tuple(got.shape) == (S, H * OUT if concat else OUT)
    assert torch.equal(got, want)
    assert layer.calls == 0  # eval mode draws no mask
    assert torch.equal(got, layer(x, seed_local, index, counts, ea if with_edge else None))
    with pytest.raises(ValueError):
        layer(x, seed_local, index, counts, None if with_edge else ea)


def _layer64(layer, x, seed_local, index, cnt, ea, S, g):
    """(out, {parameter: gradient}, {parameter: magnitude}, magnitude of out): the whole layer restated on the CPU in
    float64 from its weights alone -- x W^T + b for query, key, value and skip, ea W_e^T for the edge term, attention64
    with scale 1 / sqrt(out_dim), the heads side by side or their mean, plus the skip row -- with autograd of
    sum(out * g).  The magnitudes are the sums of |terms| behind each element: `magnitudes` for the attention, carried
    through the maps (a weight gradient sums |row gradient| |input| over the rows)."""
    import math
    import torch
    H, C, concat = layer.heads, layer.out_dim, layer.concat
    params = {name: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
              for name, p in layer.named_parameters()}
    tx = torch.tensor(x, dtype=torch.float64)
    at = torch.tensor(seed_local)

    def lin(name, inp):
        out = inp @ params[name + ".weight"].t()
        return out + params[name + ".bias"] if name + ".bias" in params else out

    qn, k, v = lin("lin_query", tx), lin("lin_key", tx), lin("lin_value", tx)
    te = None if ea is None else torch.tensor(ea, dtype=torch.float64) @ params["lin_edge.weight"].t()
    n = len(index)
    scale = 1.0 / math.sqrt(C)
    att = attention64(qn[at], k, v, te, index, cnt, S, H, scale, 0.0, np.ones((n, H)))
    skip = lin("lin_skip", tx)[at]
    if concat:
        out = att + skip
    else:
        out = sum(att[:, h * C:(h + 1) * C] for h in range(H)) / H + skip
    tg = torch.tensor(g, dtype=torch.float64)
    (out * tg).sum().backward()
    # magnitudes
    ag = np.abs(g.astype(np.float64))
    g_att = ag if concat else np.tile(ag, (1, H)) / H
    det = lambda t: None if t is None else t.detach().numpy()  # noqa: E731
    m_att, m_q, m_k, m_v, m_e = magnitudes(det(qn[at]), det(k), det(v), index, det(te), cnt, S, g_att, H, scale, 0.0,
                                           np.ones((n, H)))
    ax = np.abs(x.astype(np.float64))
    m_qn = np.zeros((len(x), H * C))
    np.add.at(m_qn, seed_local, m_q)
    ag_nodes = np.zeros((len(x), ag.shape[1]))
    np.add.at(ag_nodes, seed_local, ag)
    mags = {}
    for name, m_rows, inp in (("lin_query", m_qn, ax), ("lin_key", m_k, ax), ("lin_value", m_v, ax),
                              ("lin_skip", ag_nodes, ax), ("lin_edge", m_e, None if ea is None else np.abs(ea))):
        if name + ".weight" in params:
            mags[name + ".weight"] = m_rows.T @ inp.astype(np.float64)
        if name + ".bias" in params:
            mags[name + ".bias"] = m_rows.sum(0)
    m_skip = ax[seed_local] @ np.abs(det(params["lin_skip.weight"])).T + np.abs(det(params["lin_skip.bias"]))
    m_out = (m_att if concat else m_att.reshape(S, H, C).mean(1)) + m_skip
    return out.detach().numpy(), {k_: p.grad.numpy() for k_, p in params.items()}, mags, m_out


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "implied"])
@pytest.mark.parametrize("with_edge", [True, False], ids=["edge", "plain"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
def test_transformer_conv_against_float64_autograd_of_the_whole_layer(thg, concat, with_edge, ragged):
    """out and the gradient of EVERY parameter relative 1e-5 of the float64 restatement over the magnitudes of their
    terms, test_against_float64_autograd's criterion: segments of at most 30 positions of C = 4 columns, 40 nodes of
    12 columns; the maps add a stage of (12 + 2) * 2^-24 < 1e-6 of their terms in front of the attention's three and a
    sum over at most 60 positions or 40 nodes behind it, each of whose terms carries the attention's own error"""
    import torch
    torch.manual_seed(2)
    x, seed_local, index, counts, ea, S = _batch(ragged, seed=3)
    H = 3
    layer = thg.TransformerConv(IN, OUT, heads=H, concat=concat, dropout=0.4, edge_dim=EDGE if with_edge else None)
    layer = layer.cuda().eval()
    g = np.random.default_rng(9).standard_normal((S, H * OUT if concat else OUT)).astype(np.float32)
    got = layer(x, seed_local, index, counts, ea if with_edge else None)
    got.backward(_cuda(g))
    cnt = None if counts is None else counts.cpu().numpy()
    want, grads, mags, m_out = _layer64(layer, x.cpu().numpy(), seed_local.cpu().numpy(), index.cpu().numpy(), cnt,
                                        ea.cpu().numpy() if with_edge else None, S, g)
    diff = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
    assert got.shape == want.shape and np.all(diff <= 1e-5 * m_out), diff.max()
    names = sorted(name for name, _ in layer.named_parameters())
    assert sorted(grads) == names and sorted(mags) == names and ("lin_edge.weight" in names) == with_edge
    for name, p in layer.named_parameters():
        a = p.grad.cpu().numpy().astype(np.float64)
        assert a.shape == grads[name].shape and np.all(np.abs(a - grads[name]) <= 1e-5 * mags[name]), \
            (name, np.abs(a - grads[name]).max())
        assert np.any(a != 0), name


def test_example_trains_and_repeats_its_losses():
    """examples/train_transformer_conv.py, one short epoch twice from one seed in a process of its own: the loader's
    seeds, sample_full's edge ids into the edge-feature table, glx.unique and the layer under Adam; the loss falls
    inside the epoch, the two runs print the same per-batch losses bit for bit and the exit status says so"""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_transformer_conv.py"), "1", "4096"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("run ")]
    assert len(lines) == 2, r.stdout[-2000:]
    first, second = (float(v) for v in lines[0].split("loss ")[1].split(" (")[0].split(" -> "))
    assert second < first, lines[0]
    bits = [ln.split("bits ")[1] for ln in lines]
    assert bits[0] == bits[1] and len(bits[0].split(",")) == 8, lines
    assert "8 dropout masks drawn" in lines[0]
    assert "the two runs' losses are the same bits" in r.stdout


def _train(thg, steps=3):
    import torch
    torch.manual_seed(5)
    x, seed_local, index, counts, ea, S = _batch(True, seed=2)
    layer = thg.TransformerConv(IN, OUT, heads=2, dropout=0.4, edge_dim=EDGE).cuda().train()
    opt = torch.optim.SGD(layer.parameters(), lr=0.1)
    target = torch.randn(S, 2 * OUT, device="cuda")
    losses = []
    for _ in range(steps):
        loss = ((layer(x, seed_local, index, counts, ea) - target) ** 2).mean()
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
    x, seed_local, index, counts, ea, S = _batch(True, seed=2)
    with torch.no_grad():
        one, two = a(x, seed_local, index, counts, ea), a(x, seed_local, index, counts, ea)
        quiet = a.eval()(x, seed_local, index, counts, ea)
    assert a.calls == 3 + 2 and not torch.equal(one, two) and not torch.equal(one, quiet)


def test_state_dict_round_trip(thg):
    import torch
    torch.manual_seed(3)
    x, seed_local, index, counts, ea, S = _batch(True)
    a = thg.TransformerConv(IN, OUT, heads=2, edge_dim=EDGE).cuda().eval()
    state = a.state_dict()
    assert sorted(state) == ["lin_edge.weight", "lin_key.bias", "lin_key.weight", "lin_query.bias", "lin_query.weight",
                             "lin_skip.bias", "lin_skip.weight", "lin_value.bias", "lin_value.weight"]
    b = thg.TransformerConv(IN, OUT, heads=2, edge_dim=EDGE).cuda().eval()
    b.load_state_dict({k: v.clone() for k, v in state.items()})
    with torch.no_grad():
        assert torch.equal(a(x, seed_local, index, counts, ea), b(x, seed_local, index, counts, ea))
    plain = thg.TransformerConv(IN, OUT, heads=2, concat=False, root_weight=False, bias=False)
    assert sorted(plain.state_dict()) == ["lin_key.weight", "lin_query.weight", "lin_value.weight"]
    assert thg.TransformerConv(IN, OUT, heads=2, concat=False).lin_skip.weight.shape == (OUT, IN)
