"""The bfloat16 training path on special values (cases in bf16_special_values.py).

Tables: every NaN kind, +-inf, +-0, subnormals and +-the largest finite code planted at one (row, column) of a bfloat16
x, xa, xb or x_other, against weights and gradients of 0, -0.0, inf and a subnormal.  A bfloat16 call must give the
float32 entry point's output on the upcast table to the bit -- NaN sign and payload included: the same arithmetic on the
same device --, agree with the numpy restatement, and leave every column or head without the planted element as the
request with a finite value there has it.

Stores: every kernel that rounds a float32 sum to bfloat16 gets the planted one-rounding cases through its own
arithmetic, and must store the code written in the table; the float32 output of the same call has the restatement's
bits.  Every comparison is to the bit."""
import numpy as np
import pytest

import agg_backward_ref as ref
import agg_weighted_ref as wref
import bf16_special_values as sv
import bf16_training_ref as b16
import glx
import pair_dot_ref as pref

pytestmark = pytest.mark.gpu

OPS = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}
NAN = float("nan")
PLANTED = [(d, h, c) for d, h in sv.SPECIAL_SHAPES for c in sv.planted_columns(d)]


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cuda_bf16(codes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(codes).view(np.int16)).cuda().view(torch.bfloat16)


def _codes(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _tables(dim, col, seed):
    """(bfloat16 table, its float32 upcast, the float32 numpy matrix) of the special table and of its finite twin"""
    out = []
    for finite in (False, True):
        codes = sv.special_table(dim, col, seed, finite)
        xf = b16.upcast(codes)
        out.append((_cuda_bf16(codes), _cuda(xf), xf))
    return out


def _other_columns(dim, col):
    return np.arange(dim) != col


# ---- special codes in a table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("default_attr", [0.25, NAN], ids=["attr", "nan_attr"])
@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("dim,heads,col", PLANTED)
def test_weighted_forward_and_grad_w_take_the_planted_column_and_nothing_else(dim, heads, col, op, default_attr):
    op = OPS[op]
    (xb, x32, xf), (tb, _, _) = _tables(dim, col, 0)
    rows, w, cnt, grad_out = sv.weighted_request(dim, heads, col)
    S = len(cnt)
    d_rows, d_w, d_cnt, d_go = _cuda(rows), _cuda(w), _cuda(cnt), _cuda(grad_out)
    # forward
    emb = glx.aggregate_weighted(op, xb, d_rows, d_w, S, cnt=d_cnt, default_attr=default_attr)
    emb32 = glx.aggregate_weighted(op, x32, d_rows, d_w, S, cnt=d_cnt, default_attr=default_attr)
    assert np.array_equal(_bits(emb), _bits(emb32))
    assert wref.same_bits(emb.cpu().numpy(), wref.forward(op, xf, rows, w, cnt, S, default_attr))
    twin = glx.aggregate_weighted(op, tb, d_rows, d_w, S, cnt=d_cnt, default_attr=default_attr)
    keep = _other_columns(dim, col)
    assert np.array_equal(_bits(emb)[:, keep], _bits(twin)[:, keep])
    nan = np.isnan(emb.cpu().numpy())
    assert nan[:5, col].all()  # the five NaN codes, whatever their weight
    if default_attr == default_attr:
        assert nan[5, col] and nan[6, col] and nan[7, col] and nan[8, col]  # inf x 0, -inf x -0, 0 x inf, -0 x -inf
        assert not nan[sv.NUM_SPECIAL:].any() and not nan[:, keep].any()
    else:
        assert nan.all()  # every segment reads one row outside the table
    # grad_w
    gw = glx.aggregate_weighted_backward_w(op, xb, d_rows, heads, d_cnt, d_go, default_attr=default_attr)
    gw32 = glx.aggregate_weighted_backward_w(op, x32, d_rows, heads, d_cnt, d_go, default_attr=default_attr)
    assert np.array_equal(_bits(gw), _bits(gw32))
    want, bound = wref.backward_w(op, xf, rows, heads, cnt, grad_out, default_attr)
    assert wref.within_bound(gw.cpu().numpy(), want, bound)
    twin = glx.aggregate_weighted_backward_w(op, tb, d_rows, heads, d_cnt, d_go, default_attr=default_attr)
    other = np.arange(heads) != col // (dim // heads)
    assert np.array_equal(_bits(gw)[:, other], _bits(twin)[:, other])
    assert np.isnan(gw.cpu().numpy()[0:15:3, col // (dim // heads)]).all()  # the positions of the five NaN rows


@pytest.mark.parametrize("default_attr", [0.25, NAN], ids=["attr", "nan_attr"])
@pytest.mark.parametrize("dim,heads,col", PLANTED)
def test_pair_dot_and_its_backward_take_the_planted_column_and_nothing_else(dim, heads, col, default_attr):
    (ab, a32, af), (atb, _, _) = _tables(dim, col, 1)
    (bb, b32, bf), (btb, _, _) = _tables(dim, col, 2)
    ia, ib, g = sv.pair_request(dim, heads, col)
    d_ia, d_ib, d_g = _cuda(ia), _cuda(ib), _cuda(g)
    kw = dict(default_attr=default_attr)
    head = col // (dim // heads)
    other = np.arange(heads) != head
    keep = _other_columns(dim, col)
    out = glx.pair_dot(ab, d_ia, bb, d_ib, heads=heads, **kw)
    out32 = glx.pair_dot(a32, d_ia, b32, d_ib, heads=heads, **kw)
    assert np.array_equal(_bits(out), _bits(out32))
    want, bound = pref.forward(af, ia, bf, ib, heads, 1, default_attr)
    assert pref.within_bound(out.cpu().numpy(), want, bound)
    twin = glx.pair_dot(atb, d_ia, btb, d_ib, heads=heads, **kw)
    assert np.array_equal(_bits(out)[:, other], _bits(twin)[:, other])
    nan = np.isnan(out.cpu().numpy())
    assert nan[:5, head].all() and nan[16:21, head].all()  # the NaN codes of xa and of xb
    for side, (other_b, other_32, other_f, other_twin) in enumerate([(bb, b32, bf, btb), (ab, a32, af, atb)]):
        gs = glx.pair_dot_backward(side, d_ia, d_ib, d_g, other_b, sv.TABLE_ROWS, **kw)
        gs32 = glx.pair_dot_backward(side, d_ia, d_ib, d_g, other_32, sv.TABLE_ROWS, **kw).cpu().numpy()
        assert str(gs.dtype) == "torch.bfloat16"
        got = _codes(gs)
        assert np.array_equal(got, b16.to_bf16(gs32)), side
        assert np.array_equal(got == 0xFFFF, np.isnan(gs32)), side  # a NaN is 0xFFFF, and nothing else is
        want = pref.backward(side, ia, ib, g, other_f, sv.TABLE_ROWS, 1, default_attr)
        assert pref.same_bits(gs32, want), side
        assert np.array_equal(got, b16.to_bf16(want)), side
        assert np.isnan(gs32[sv.NUM_SPECIAL:, col]).all(), side  # each finite row meets a NaN code of the other table
        twin = _codes(glx.pair_dot_backward(side, d_ia, d_ib, d_g, other_twin, sv.TABLE_ROWS, **kw))
        assert np.array_equal(got[:, keep], twin[:, keep]), side


# ---- one rounding in every store -------------------------------------------------------------------------------------
def _check_rounding(got16, got32, case):
    codes = _codes(got16)
    assert np.array_equal(codes, case["codes"]), [hex(v) for v in codes[:, 0]]
    assert wref.same_bits(got32.cpu().numpy(), case["sums"])
    assert np.array_equal(codes, b16.to_bf16(got32.cpu().numpy()))
    # rounding after every add would have stored another code for the accumulation case
    terms, code = sv.ROUNDING_CASES[sv.ACCUMULATION_CASE]
    assert codes[sv.ACCUMULATION_CASE, 0] == code != sv.per_add_rounding_code(terms, b16.to_bf16)


@pytest.mark.parametrize("dim,heads", sv.ROUNDING_SHAPES)
@pytest.mark.parametrize("op", ["sum", "mean"])
def test_weighted_backward_x_rounds_the_float32_sum_once(op, dim, heads):
    case = sv.weighted_backward_x_rounding(OPS[op], dim, heads)
    args = (OPS[op], _cuda(case["rows"]), _cuda(case["w"]), _cuda(case["cnt"]), _cuda(case["grad_out"]),
            case["num_rows"])
    _check_rounding(glx.aggregate_weighted_backward_x(*args, out_dtype="bfloat16"),
                    glx.aggregate_weighted_backward_x(*args), case)


@pytest.mark.parametrize("dim,heads", sv.ROUNDING_SHAPES)
@pytest.mark.parametrize("repeat", [1, 3])
@pytest.mark.parametrize("side", [0, 1])
def test_pair_dot_backward_rounds_the_float32_sum_once(side, repeat, dim, heads):
    case = sv.pair_dot_backward_rounding(side, repeat, dim, heads)
    d_ia, d_ib, d_g = _cuda(case["ia"]), _cuda(case["ib"]), _cuda(case["g"])
    got16 = glx.pair_dot_backward(side, d_ia, d_ib, d_g, _cuda_bf16(case["x_other"]), case["num_rows"], repeat=repeat)
    got32 = glx.pair_dot_backward(side, d_ia, d_ib, d_g, _cuda(b16.upcast(case["x_other"])), case["num_rows"],
                                  repeat=repeat)
    _check_rounding(got16, got32, case)


@pytest.mark.parametrize("dim", [6, 12])
@pytest.mark.parametrize("op", sorted(OPS))
def test_aggregate_backward_rounds_the_float32_sum_once(op, dim):
    case = sv.aggregate_backward_rounding(OPS[op], dim)
    args = (OPS[op], _cuda(case["rows"]), _cuda(case["cnt"]), _cuda(case["grad_out"]), case["num_rows"])
    _check_rounding(glx.aggregate_backward(*args, arg=_cuda(case["arg"]), out_dtype="bfloat16"),
                    glx.aggregate_backward(*args, arg=_cuda(case["arg"])), case)
