"""glx_gat_attention_backward_chunked on the GPU: grad_t in the chunked order against
agg_chunked_ref -- the Sum row gradient of grad_e with one position per segment and dim = heads -- grad_e and grad_s
with the default call's bits, and GATConv(chunked_grad=True).  Every comparison is to the bit."""
import os
import sys

import numpy as np
import pytest

import agg_backward_ref as ref
import agg_chunked_ref as cref
import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

NUM_ROWS = 16
LISTS = {0: 0, 1: 1, 2: 255, 3: 256, 4: 257, 5: 512, 6: 513, 7: 700}  # row of t -> entries of its list
CONSUMED, TAIL = 2560, 40


def _request():
    """(rows, counts): 2,560 consumed positions with the lists above, -1 and NUM_ROWS among them, in ragged segments
    (two of them empty, one of 900 positions); 40 more positions name row 7 and are consumed by nobody"""
    rng = np.random.default_rng(21)
    rows = [np.full(n, r, np.int64) for r, n in LISTS.items()] + [np.array([-1, NUM_ROWS], np.int64)]
    rows.append(rng.integers(8, NUM_ROWS - 1, CONSUMED - sum(LISTS.values()) - 2))  # row 15: named by nobody
    rows = np.concatenate(rows)
    rng.shuffle(rows)
    cnt = np.array([0, 900, 3, 257, 0, 1, 600, 799], np.int32)
    assert cnt.sum() == CONSUMED == len(rows)
    return np.concatenate([rows, np.full(TAIL, 7, np.int64)]), cnt


ROWS, CNT = _request()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("heads", [1, 2, 4, 3])
def test_grad_t_against_the_restatement(heads, drop_p):
    import torch
    rng = np.random.default_rng(heads)
    s = _cuda(rng.standard_normal((len(CNT), heads)).astype(np.float32))
    t = _cuda(rng.standard_normal((NUM_ROWS, heads)).astype(np.float32))
    ga = _cuda(rng.standard_normal((len(ROWS), heads)).astype(np.float32))
    rows, cnt = _cuda(ROWS), _cuda(CNT)
    kw = dict(cnt=cnt, drop_p=drop_p, seed=5, call=2)
    _, soft = glx.gat_attention(s, t, rows, **kw)
    nan = lambda n: torch.full((n, heads), float("nan"), device="cuda")  # noqa: E731  (every element must be written)
    plain = glx.gat_attention_backward(soft, ga, s, t, rows, **kw)
    got = glx.gat_attention_backward(soft, ga, s, t, rows, out=nan(len(ROWS)), out_s=nan(len(CNT)), out_t=nan(NUM_ROWS),
                                     chunked=True, **kw)
    assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), plain[1].view(torch.int32))
    grad_e = got[0].cpu().numpy()[:CONSUMED]
    want = cref.backward(ref.SUM, ROWS[:CONSUMED], np.ones(CONSUMED, np.int32), grad_e, NUM_ROWS)
    assert ref.same_bits(got[2].cpu().numpy(), want)
    short = [r for r in range(NUM_ROWS) if LISTS.get(r, 0) <= cref.CHUNK]
    assert torch.equal(got[2][short].view(torch.int32), plain[2][short].view(torch.int32))


def _layer_grads(chunked, index, counts, x, seed_local):
    import torch
    from graphlearn.nn.pytorch import GATConv
    torch.manual_seed(3)
    layer = GATConv(6, 4, num_heads=3, concat=True, dropout=0.3, use_bias=True, seed=11, chunked_grad=chunked).cuda().train()
    out = layer(x, seed_local, index, counts)
    out.backward(torch.cos(out.detach()))
    return out.detach(), [p.grad.clone() for p in layer.parameters()]


def test_gat_conv_takes_the_flag():
    import torch
    rng = np.random.default_rng(4)
    x = _cuda(rng.standard_normal((NUM_ROWS, 6)).astype(np.float32))
    seed_local = _cuda(rng.permutation(NUM_ROWS)[:len(CNT)].astype(np.int64))
    hubs = (_cuda(np.clip(ROWS[:CONSUMED], 0, NUM_ROWS - 1)), _cuda(CNT), x, seed_local)
    out, first = _layer_grads(True, *hubs)
    again = _layer_grads(True, *hubs)
    plain = _layer_grads(False, *hubs)
    assert torch.equal(out, again[0]) and torch.equal(out, plain[0])  # the forward ignores the flag
    assert all(torch.equal(a, b) for a, b in zip(first, again[1]))
    assert not all(torch.equal(a, b) for a, b in zip(first, plain[1]))  # the flag reached both ops' gradients
    flat = (_cuda(rng.integers(0, NUM_ROWS, 600)), _cuda(np.array([0, 100, 3, 57, 0, 1, 200, 239], np.int32)), x, seed_local)
    for a, b in zip(_layer_grads(True, *flat)[1], _layer_grads(False, *flat)[1]):  # no row named above 256 times
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
