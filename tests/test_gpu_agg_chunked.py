"""glx_aggregate_backward_chunked / glx_aggregate_weighted_backward_x_chunked on the GPU, through glx.py's wrappers,
against the numpy restatement of the chunked order (agg_chunked_ref.py).

Every comparison is to the bit.  One request serves every test: 2,600 consumed positions over 40 rows whose lists have
exactly 0, 1, 255, 256, 257, 512, 513 and 700 entries (one chunk or less; one entry more; two whole chunks; two and one
entry; two and a part), the ids -1 and num_rows among them, in the three layouts of test_gpu_bf16_training.py."""
import functools

import numpy as np
import pytest

import agg_backward_ref as ref
import agg_chunked_ref as cref
import agg_weighted_ref as wref
import bf16_training_ref as b16
import glx

pytestmark = pytest.mark.gpu

OPS = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}
DIMS = [1, 5, 12, 36, 256, 260]  # VEC 1 (1, 5) and 4; groups of 8, 16 and 64; a second column tile (260)
HEAD_SHAPES = [(6, 2), (12, 1), (16, 4), (256, 4)]  # C % 4 != 0 (VEC 1); one head; sub-groups; a head over several lanes
NUM_ROWS = 40
LISTS = {0: 0, 1: 1, 2: 255, 3: 256, 4: 257, 5: 512, 6: 513, 7: 700}  # row -> entries of its list
ABSENT = (0, 20, 39)
CONSUMED, TAIL = 2600, 30
GUARD32, GUARD16 = 0x7FC01234, 0x1234
NO_TERM_ROW, NO_TERM_CHUNK = 5, 1  # Max / Min: no entry of this chunk is selected


def _positions():
    """2,630 positions: the first 2,600 give the lists above, 2 ids outside the table and 104 entries over the other
    rows; the last 30 name row 7 again and are consumed by no layout"""
    rng = np.random.default_rng(11)
    rows = [np.full(n, r, np.int64) for r, n in LISTS.items()]
    pool = np.array([r for r in range(len(LISTS), NUM_ROWS) if r not in ABSENT], np.int64)
    rows.append(rng.choice(pool, CONSUMED - sum(LISTS.values()) - 2))
    rows.append(np.array([-1, NUM_ROWS], np.int64))
    rows = np.concatenate(rows)
    rng.shuffle(rows)
    assert len(rows) == CONSUMED
    return np.concatenate([rows, np.full(TAIL, 7, np.int64)])


ROWS = _positions()


def _counts():
    rng = np.random.default_rng(12)
    cnt = rng.multinomial(CONSUMED, np.ones(24) / 24).astype(np.int32)
    cnt = np.insert(cnt, [0, 5, 5, 24], 0)  # empty segments, two of them adjacent, one at either end
    assert cnt.sum() == CONSUMED
    return cnt


_CNT = _counts()
_OVER = _CNT.copy()
_OVER[-2] += 90  # the last segment that has positions promises 90 more than the request holds
# layout -> (rows, cnt, num_segments); the implied layout: 65 segments of 2630 // 65 = 40 positions
LAYOUTS = {"implied": (ROWS, None, 65), "ragged_tail": (ROWS, _CNT, len(_CNT)),
           "ragged_over": (ROWS[:CONSUMED], _OVER, len(_OVER))}


def test_the_request_has_the_lists_it_claims():
    for rows, cnt, S in LAYOUTS.values():
        lengths = cref.list_lengths(rows, cnt, S, NUM_ROWS)
        assert all(lengths[r] == n for r, n in LISTS.items())
        assert not lengths[list(ABSENT)].any() and lengths.sum() == CONSUMED - 2


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _codes(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _request(op, layout, dim):
    """(cnt, grad_out, arg, the restatement's chunked result, its ascending-order result), computed once"""
    rows, cnt, S = LAYOUTS[layout]
    rng = np.random.default_rng(1000 + dim)
    arg = None
    if op in (ref.MAX, ref.MIN):  # small integers: ties everywhere, so arg matters
        grad_out = rng.integers(-3, 4, (S, dim)).astype(np.float32)
        X = rng.integers(-2, 3, (NUM_ROWS, dim)).astype(np.float32)
        start = np.minimum(ref.segment_starts(cnt, len(rows), S), len(rows))
        arg = ref.fold_arg(op, X, rows, start)[1]
        # deselect every entry of one chunk (as a NaN would: arg -1); its partial is +0.0 and is still added
        lst = np.flatnonzero(rows[:CONSUMED] == NO_TERM_ROW)[NO_TERM_CHUNK * cref.CHUNK:(NO_TERM_CHUNK + 1) * cref.CHUNK]
        assert len(lst) == cref.CHUNK
        arg[np.isin(arg, lst)] = -1
        assert not np.isin(arg, lst).any()
    else:
        grad_out = rng.standard_normal((S, dim)).astype(np.float32)
        grad_out[0, 0] = -0.0
    want = cref.backward(op, rows, cnt, grad_out, NUM_ROWS, arg)
    plain = ref.backward(op, rows, cnt, grad_out, NUM_ROWS, arg)
    return cnt, grad_out, arg, want, plain


def _guarded(dtype, dim, pad=3):
    """(the whole buffer, its first NUM_ROWS rows): every element a NaN with a payload"""
    import torch
    if dtype == "float32":
        big = torch.full((NUM_ROWS + pad, dim), GUARD32, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        big = torch.full((NUM_ROWS + pad, dim), GUARD16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return big, big[:NUM_ROWS]


def _guard_ok(big, dtype):
    if dtype == "float32":
        return bool((big[NUM_ROWS:].cpu().numpy().view(np.uint32) == GUARD32).all())
    return bool((_codes(big)[NUM_ROWS:] == GUARD16).all())


def _agg(op, layout, dim, dtype, chunked=True):
    rows, cnt, S = LAYOUTS[layout]
    _, grad_out, arg, _, _ = _request(op, layout, dim)
    big, out = _guarded(dtype, dim)
    got = glx.aggregate_backward(op, _cuda(rows), _cuda(cnt), _cuda(grad_out), NUM_ROWS, arg=_cuda(arg), out=out,
                                 chunked=chunked)
    assert got is out
    assert _guard_ok(big, dtype)  # nothing behind the last row is touched
    return out.cpu().numpy() if dtype == "float32" else _codes(out)


SHORT = [r for r in range(NUM_ROWS) if LISTS.get(r, 0) <= cref.CHUNK]
LONG = [r for r in range(NUM_ROWS) if LISTS.get(r, 0) > cref.CHUNK]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim", DIMS)
def test_aggregate_backward_chunked(dim, op, layout):
    _, _, _, want, plain = _request(OPS[op], layout, dim)
    got = _agg(OPS[op], layout, dim, "float32")
    assert ref.same_bits(got, want)  # every row overwritten: the buffer held NaN
    assert ref.same_bits(got[SHORT], plain[SHORT])  # at most one chunk: the default order's bits
    assert ref.same_bits(got[SHORT], _agg(OPS[op], layout, dim, "float32", chunked=False)[SHORT])
    assert not got[list(ABSENT)].view(np.uint32).any()  # rows nobody references: all bits clear
    if op in ("sum", "mean") and dim >= 5:
        assert (got[LONG].view(np.uint32) != plain[LONG].view(np.uint32)).any()  # the orders differ where they may
    assert ref.same_bits(got, _agg(OPS[op], layout, dim, "float32"))  # the same bits on every call
    bf = _agg(OPS[op], layout, dim, "bfloat16")
    assert np.array_equal(bf, b16.to_bf16(got))  # one rounding of the float32 chunked sum
    assert not bf[list(ABSENT)].any()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("dim", DIMS)
def test_sum_is_rows_coalesce_of_the_gathered_rows(dim, layout):
    rows, cnt, S = LAYOUTS[layout]
    _, grad_out, _, _, _ = _request(ref.SUM, layout, dim)
    start = wref.starts(cnt, len(rows), S)
    seg = np.searchsorted(start, np.arange(int(start[-1])), side="right") - 1
    urows, ug, count = glx.rows_coalesce(_cuda(rows[:len(seg)]), _cuda(grad_out[seg]), NUM_ROWS)
    U = int(count.item())
    want = np.zeros((NUM_ROWS, dim), np.float32)
    want[urows[:U].cpu().numpy()] = ug[:U].cpu().numpy()
    assert ref.same_bits(_agg(ref.SUM, layout, dim, "float32"), want)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim", [5, 256])
def test_host_pointers_agree_with_device_pointers(dim, op, dtype):
    rows, cnt, S = LAYOUTS["ragged_tail"]
    _, grad_out, arg, _, _ = _request(OPS[op], "ragged_tail", dim)
    host = glx.aggregate_backward(OPS[op], rows, cnt, grad_out, NUM_ROWS, arg=arg, out_dtype=dtype, chunked=True)
    dev = _agg(OPS[op], "ragged_tail", dim, dtype)
    assert np.array_equal(host.view(np.uint32 if dtype == "float32" else np.uint16),
                          dev.view(np.uint32 if dtype == "float32" else np.uint16))


def _offset4(a):
    """a CUDA copy of float32 / int32 `a` that starts 4 bytes past a 16-byte boundary"""
    import torch
    flat = torch.empty(a.size + 1, dtype=torch.float32 if a.dtype == np.float32 else torch.int32, device="cuda")
    view = flat[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim", [12, 256])
def test_a_misaligned_grad_out_takes_the_scalar_path(dim, op):
    rows, cnt, S = LAYOUTS["ragged_over"]
    _, grad_out, arg, want, _ = _request(OPS[op], "ragged_over", dim)
    got = glx.aggregate_backward(OPS[op], _cuda(rows), _cuda(cnt), _offset4(grad_out), NUM_ROWS, arg=_cuda(arg),
                                 chunked=True)
    assert ref.same_bits(got.cpu().numpy(), want)


# ---- the weighted row gradient -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wrequest(op, layout, dim, heads):
    rows, cnt, S = LAYOUTS[layout]
    rng = np.random.default_rng(2000 + dim + heads)
    grad_out = rng.standard_normal((S, dim)).astype(np.float32)
    w = rng.standard_normal((len(rows), heads)).astype(np.float32)
    w[::97] = -0.0
    want = cref.backward_weighted_x(op, rows, w, cnt, grad_out, NUM_ROWS)
    plain = wref.backward_x(op, rows, w, cnt, grad_out, NUM_ROWS)
    return cnt, grad_out, w, want, plain


def _wagg(op, layout, dim, heads, dtype, chunked=True, grad_out_dev=None):
    rows, cnt, S = LAYOUTS[layout]
    _, grad_out, w, _, _ = _wrequest(op, layout, dim, heads)
    big, out = _guarded(dtype, dim)
    go = _cuda(grad_out) if grad_out_dev is None else grad_out_dev
    got = glx.aggregate_weighted_backward_x(op, _cuda(rows), _cuda(w), _cuda(cnt), go, NUM_ROWS, out=out,
                                            chunked=chunked)
    assert got is out
    assert _guard_ok(big, dtype)
    return out.cpu().numpy() if dtype == "float32" else _codes(out)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("dim,heads", HEAD_SHAPES)
def test_weighted_backward_x_chunked(dim, heads, op, layout):
    _, _, _, want, plain = _wrequest(OPS[op], layout, dim, heads)
    got = _wagg(OPS[op], layout, dim, heads, "float32")
    assert ref.same_bits(got, want)
    assert ref.same_bits(got[SHORT], plain[SHORT])
    assert ref.same_bits(got[SHORT], _wagg(OPS[op], layout, dim, heads, "float32", chunked=False)[SHORT])
    assert not got[list(ABSENT)].view(np.uint32).any()
    assert (got[LONG].view(np.uint32) != plain[LONG].view(np.uint32)).any()
    assert ref.same_bits(got, _wagg(OPS[op], layout, dim, heads, "float32"))
    bf = _wagg(OPS[op], layout, dim, heads, "bfloat16")
    assert np.array_equal(bf, b16.to_bf16(got))
    assert not bf[list(ABSENT)].any()


@pytest.mark.parametrize("dim,heads", [(6, 2), (256, 4)])
def test_weighted_host_pointers_and_a_misaligned_grad_out(dim, heads):
    rows, cnt, S = LAYOUTS["ragged_tail"]
    _, grad_out, w, want, _ = _wrequest(ref.MEAN, "ragged_tail", dim, heads)
    host = glx.aggregate_weighted_backward_x(ref.MEAN, rows, w, cnt, grad_out, NUM_ROWS, chunked=True)
    assert ref.same_bits(host, want)
    host16 = glx.aggregate_weighted_backward_x(ref.MEAN, rows, w, cnt, grad_out, NUM_ROWS, out_dtype="bfloat16",
                                               chunked=True)
    assert np.array_equal(host16, b16.to_bf16(want))
    got = _wagg(ref.MEAN, "ragged_tail", dim, heads, "float32", grad_out_dev=_offset4(grad_out))
    assert ref.same_bits(got, want)
