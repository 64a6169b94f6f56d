"""glx_pair_dot_backward_chunked on the GPU, through glx.py's wrapper and graphlearn.nn.pytorch.pair_dot, against the
numpy restatement of the chunked order (pair_dot_chunked_ref.py).  Every comparison is to
the bit.

One request per `repeat`, each with both index arrays full of hubs, so either side has long runs:
  repeat 1    ia and ib both give rows 0 .. 7 runs of exactly 0, 1, 255, 256, 257, 512, 513 and 700 pairs
  repeat 3    ia names rows 1 .. 4 85 / 86 / 171 / 234 times: runs of 255 / 258 / 513 / 702 pairs on side 0, whose chunk
              boundaries (256 = 85 * 3 + 1, ...) fall inside an entry's three pairs; ib as above
  repeat 300  row 3 of ia is one entry -- alone a long run of 300 pairs -- row 5 two entries, 600 pairs
Every index array holds -1 and NUM_ROWS once (other side: they read default_attr; own side: they receive nothing), and
rows 0, 12 and 23 are named by nobody."""
import functools
import os
import sys

import numpy as np
import pytest

import bf16_training_ref as b16
import glx
import pair_dot_chunked_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

NUM_ROWS = 24
ABSENT = (0, 12, 23)
RUNS = {0: 0, 1: 1, 2: 255, 3: 256, 4: 257, 5: 512, 6: 513, 7: 700}
# VEC 1 and 4, groups of 8 to 64, sub-groups, a second column tile
SHAPES = [(1, 1), (5, 1), (6, 2), (12, 1), (16, 4), (36, 1), (256, 4), (260, 1)]
DEFAULT_ATTR = 0.75


def _index(counts, total, seed):
    """`total` entries: row r counts[r] times, -1 and NUM_ROWS once each, the rest over the rows that are neither in
    `counts` nor ABSENT; shuffled"""
    rng = np.random.default_rng(seed)
    pool = np.array([r for r in range(NUM_ROWS) if r not in counts and r not in ABSENT], np.int64)
    idx = [np.full(n, r, np.int64) for r, n in counts.items()] + [np.array([-1, NUM_ROWS], np.int64)]
    idx.append(rng.choice(pool, total - sum(counts.values()) - 2))
    idx = np.concatenate(idx)
    rng.shuffle(idx)
    return idx


REQUESTS = {  # repeat -> (ia, ib)
    1: (_index(RUNS, 2600, 1), _index(RUNS, 2600, 2)),
    3: (_index({1: 85, 2: 86, 3: 171, 4: 234}, 900, 3), _index(RUNS, 2700, 4)),
    300: (np.array([5, NUM_ROWS, 3, 5, -1], np.int64), _index({1: 257, 2: 300}, 1500, 5)),
}
SHORT = (_index({1: 255, 2: 256, 3: 1}, 700, 6), _index({4: 256, 5: 200}, 700, 7))  # no run above 256, repeat 1


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(x, dtype):
    """the device table of float32 values x (bfloat16: of their codes)"""
    import torch
    return _cuda(x) if dtype == "float32" else _cuda(b16.to_bf16(x).view(np.int16)).view(torch.bfloat16)


def _bits(t, dtype):
    import torch
    if dtype == "float32":
        return t.cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _guarded(dim, dtype):
    """a grad_self of NaNs: every row has to be written"""
    import torch
    return torch.full((NUM_ROWS, dim), float("nan"), dtype=getattr(torch, dtype), device="cuda")


@functools.lru_cache(maxsize=None)
def _case(repeat, side, dim, heads, dtype):
    """(g, x_other's float32 values, the restatement's bits), computed once"""
    ia, ib = REQUESTS[repeat]
    rng = np.random.default_rng(100 * dim + heads)
    g = rng.standard_normal((len(ib), heads)).astype(np.float32)
    x = rng.standard_normal((NUM_ROWS, dim)).astype(np.float32)
    if dtype == "bfloat16":
        x = b16.upcast(b16.to_bf16(x))
    want = cref.backward(side, ia, ib, g, x, NUM_ROWS, repeat, DEFAULT_ATTR)
    return g, x, want.view(np.uint32) if dtype == "float32" else b16.to_bf16(want)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("dim,heads", SHAPES)
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("repeat", sorted(REQUESTS))
def test_against_the_restatement(repeat, side, dim, heads, dtype):
    ia, ib = REQUESTS[repeat]
    g, x, want = _case(repeat, side, dim, heads, dtype)
    args = (side, _cuda(ia), _cuda(ib), _cuda(g), _table(x, dtype), NUM_ROWS)
    got = glx.pair_dot_backward(*args, repeat=repeat, default_attr=DEFAULT_ATTR, out=_guarded(dim, dtype), chunked=True)
    assert np.array_equal(_bits(got, dtype), want)
    assert not _bits(got, dtype)[list(ABSENT)].any()  # a row nobody names: all bits clear
    again = glx.pair_dot_backward(*args, repeat=repeat, default_attr=DEFAULT_ATTR, chunked=True)
    assert np.array_equal(_bits(again, dtype), want)  # the same bits on every call


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("dim,heads", [(5, 1), (16, 4)])
@pytest.mark.parametrize("side", [0, 1])
def test_a_request_without_long_runs_gets_the_default_bits(side, dim, heads, dtype):
    ia, ib = SHORT
    rng = np.random.default_rng(9)
    g = _cuda(rng.standard_normal((len(ib), heads)).astype(np.float32))
    x = _table(rng.standard_normal((NUM_ROWS, dim)).astype(np.float32), dtype)
    got = [glx.pair_dot_backward(side, _cuda(ia), _cuda(ib), g, x, NUM_ROWS, default_attr=DEFAULT_ATTR,
                                 out=_guarded(dim, dtype), chunked=c) for c in (False, True)]
    assert np.array_equal(_bits(got[0], dtype), _bits(got[1], dtype))


def test_host_pointers():
    ia, ib = REQUESTS[3]
    g, x, want = _case(3, 0, 12, 1, "float32")
    got = glx.pair_dot_backward(0, ia, ib, g, x, NUM_ROWS, repeat=3, default_attr=DEFAULT_ATTR, chunked=True)
    assert np.array_equal(got.view(np.uint32), want)


def test_autograd_takes_the_flag_on_both_sides():
    """one leaf on both sides: its gradient is the two engine gradients added by torch; the scores ignore the flag"""
    import torch
    from graphlearn.nn.pytorch import pair_dot
    ia, ib = REQUESTS[3]
    g, x, _ = _case(3, 0, 12, 1, "float32")
    d_ia, d_ib, d_g = _cuda(ia), _cuda(ib).view(len(ia), 3), _cuda(g).view(len(ia), 3)
    z = _cuda(x).requires_grad_()
    out = pair_dot(z, d_ia, z, d_ib, default_attr=DEFAULT_ATTR, chunked_grad=True)
    assert torch.equal(out, pair_dot(z, d_ia, z, d_ib, default_attr=DEFAULT_ATTR))
    out.backward(d_g)
    sides = [glx.pair_dot_backward(s, d_ia, d_ib, d_g.view(-1, 1), z.detach(), NUM_ROWS, repeat=3,
                                   default_attr=DEFAULT_ATTR, chunked=True) for s in (0, 1)]
    assert np.array_equal(_bits(z.grad, "float32"), _bits(sides[0] + sides[1], "float32"))
    plain = glx.pair_dot_backward(0, d_ia, d_ib, d_g.view(-1, 1), z.detach(), NUM_ROWS, repeat=3,
                                  default_attr=DEFAULT_ATTR)
    assert not torch.equal(plain, sides[0])  # the flag reached the engine
