"""glx_aggregate_arg / glx_aggregate_backward on the GPU against the numpy restatement of the contract
(agg_backward_ref.py).  Tolerance 0 everywhere: bit equality, the sign of zero included."""
import numpy as np
import pytest

import agg_backward_ref as ref
import glx

pytestmark = pytest.mark.gpu

OPS = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}
U = 4  # grad_out rows the reduce kernel keeps in flight per lane (kBwdU)
NAN = np.float32(np.nan)


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_backward(op, rows, cnt, grad_out, num_rows, arg=None, host=False):
    """grad_x as numpy; the output buffer starts as a NaN canary (the entry point overwrites, the caller clears nothing)"""
    import torch
    D = grad_out.shape[1]
    if host:
        out = np.full((num_rows, D), NAN, np.float32)
        glx.aggregate_backward(op, rows, cnt, grad_out, num_rows, arg=arg, out=out)
        return out
    out = torch.full((num_rows, D), float("nan"), dtype=torch.float32, device="cuda")
    glx.aggregate_backward(op, _cuda(rows), _cuda(cnt), _cuda(grad_out), num_rows, arg=_cuda(arg), out=out)
    return out.cpu().numpy()


def check(op, rows, cnt, S, D, num_rows, seed=0, host=False):
    """one request through the GPU and the restatement; Max / Min take the restatement's arg of a random table"""
    rng = np.random.default_rng(seed)
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    grad_out[0, 0] = -0.0
    arg = None
    if op in (ref.MAX, ref.MIN):
        X = rng.standard_normal((num_rows, D)).astype(np.float32)
        arg = ref.fold_arg(op, X, rows, ref.segment_starts(cnt, len(rows), S))[1]
    want = ref.backward(op, rows, cnt, grad_out, num_rows, arg)
    got = gpu_backward(op, rows, cnt, grad_out, num_rows, arg, host)
    assert not np.isnan(got).any(), "a row was not written"
    assert ref.same_bits(got, want)
    return got


# 3 segments x 5 positions over 7 rows: row 2 four times, row 5 never, indices -1 and num_rows
BASE_ROWS = np.array([2, 2, -1, 4, 2, 0, 7, 2, 1, 3, 6, 6, 0, 3, 1], np.int64)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("dim", [1, 4, 32, 64, 100, 128, 256, 260])
def test_base_request_every_dimension_path(dim, op, host):
    """dim 1: scalar path; 4, 32: G = 8; 64: 16; 100 (25 lanes), 128: 32; 256: 64; 260: a second column tile"""
    got = check(OPS[op], BASE_ROWS, None, 3, dim, 7, seed=dim, host=host)
    assert not got[5].any() and not np.signbit(got[5]).any()  # nobody refers to row 5: +0.0


@pytest.mark.parametrize("op", ["sum", "mean", "max"])
@pytest.mark.parametrize("dim", [4, 100])
def test_list_lengths_at_the_launch_edges(dim, op):
    lengths = [0, 1, U, U + 1, 63, 64, 65, 200]
    rows = np.repeat(np.arange(len(lengths)), lengths).astype(np.int64)
    np.random.default_rng(3).shuffle(rows)
    assert len(rows) == 402
    check(OPS[op], rows, None, 6, dim, len(lengths), seed=1)


@pytest.mark.parametrize("dim", [4, 64, 128, 256])  # 32 / 16 / 8 / 4 rows per workgroup
@pytest.mark.parametrize("num_rows", [1, 63, 64, 65, 257])
def test_row_counts_at_the_workgroup_edges(num_rows, dim):
    rng = np.random.default_rng(num_rows)
    rows = rng.integers(-1, num_rows + 1, 3 * 40).astype(np.int64)
    rows[-1] = num_rows - 1  # the last row of the last workgroup has a list
    check(ref.MEAN, rows, None, 40, dim, num_rows, seed=2)


def _forward(op, X, ids, seg, S, default_attr=0.0):
    f = glx.Features(_cuda(X), view=True)
    emb, cnt = f.aggregate(op, _cuda(ids), _cuda(seg), S, default_attr)
    return emb.cpu().numpy(), cnt.cpu().numpy()


SEG_CASES = {
    # empty segments first, in the middle and last
    "ragged": (np.array([1, 1, 1, 2, 4, 4, 4, 4, 4, 6, 6], np.int32), 8),
    # position 5 steps back: the cursor stalls there for good
    "out_of_order": (np.array([0, 0, 1, 3, 3, 2, 3, 4, 4, 5, 5], np.int32), 6),
    # position 4 names a segment that does not exist
    "out_of_range": (np.array([0, 1, 1, 2, 9, 2, 3, 3, 4, 4, 4], np.int32), 5),
}


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("case", sorted(SEG_CASES))
def test_explicit_segment_ids(case, op):
    seg, S = SEG_CASES[case]
    rng = np.random.default_rng(11)
    num_rows, D = 6, 8
    ids = rng.integers(-1, num_rows + 1, len(seg)).astype(np.int64)
    ids[-1] = 2  # behind the violation (or in the last segment): a row that must get nothing from there
    X = rng.standard_normal((num_rows, D)).astype(np.float32)
    emb, cnt = _forward(OPS[op], X, ids, seg, S, default_attr=0.5)
    assert cnt.tolist() == ref.cursor_counts(seg, S).tolist()
    if case != "ragged":
        assert cnt.sum() < len(seg)
    # "segments are the prefix sums of cnt", pinned against the code that defines it
    start = ref.segment_starts(cnt, len(ids), S)
    assert ref.same_bits(emb, ref.fold(OPS[op], X, ids, start, 0.5))
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    arg = ref.fold_arg(OPS[op], X, ids, start, 0.5)[1] if op in ("max", "min") else None
    want = ref.backward(OPS[op], ids, cnt, grad_out, num_rows, arg)
    got = gpu_backward(OPS[op], ids, cnt, grad_out, num_rows, arg)
    assert ref.same_bits(got, want)
    consumed = ids[:cnt.sum()]
    for r in range(num_rows):
        if r not in consumed:
            assert not got[r].any()


def _arg_case(name):
    """(X, ids, S, default_attr) of the Max / Min corner cases, 4 positions per segment"""
    rng = np.random.default_rng(23)
    X = rng.standard_normal((9, 8)).astype(np.float32)
    ids = rng.integers(0, 9, 20).astype(np.int64)
    default_attr = 0.0
    if name == "tie":
        X[3] = X[1]
        ids[4:8] = [5, 1, 3, 1]  # rows 1 and 3 are equal: wherever they win, position 5 does
        X[5] = -50.0
    elif name == "all_below_start":
        X[2], X[4] = -38.0, -1000.0
        ids[ids == 4] = 0
        ids[8:12] = [2, 4, 4, 2]  # Max starts at -37: nothing replaces it; no other segment refers to row 4
    elif name == "nan":
        X[6, ::2] = np.nan
        ids[0:4] = [6, 0, 6, 7]
    elif name == "default_row_wins":
        default_attr = 100.0
        ids[12:16] = [0, -1, 9, 1]  # unknown ids read a row of 100: position 13 is the argument, its gradient is dropped
    return X, ids, 5, default_attr


@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("case", ["plain", "tie", "all_below_start", "nan", "default_row_wins"])
def test_recording_forward_and_its_backward(case, op):
    X, ids, S, default_attr = _arg_case(case)
    if op == "min":
        X, default_attr = -X, -default_attr  # the mirror image: the same positions win
    f = glx.Features(_cuda(X), view=True)
    emb0, cnt0 = f.aggregate(OPS[op], _cuda(ids), None, S, default_attr)
    emb, cnt, arg = f.aggregate_arg(OPS[op], _cuda(ids), None, S, default_attr)
    emb, cnt, arg = emb.cpu().numpy(), cnt.cpu().numpy(), arg.cpu().numpy()
    assert ref.same_bits(emb, emb0.cpu().numpy()) and np.array_equal(cnt, cnt0.cpu().numpy())
    want_emb, want_arg = ref.fold_arg(OPS[op], X, ids, ref.segment_starts(None, len(ids), S), default_attr)
    assert ref.same_bits(emb, want_emb) and np.array_equal(arg, want_arg)
    if case == "tie":
        assert (arg[1] == 5).all()
    if case == "all_below_start" and op == "max":
        assert (arg[2] == -1).all() and (emb[2] == -37.0).all()
    if case == "nan":
        assert not np.isin(arg[0, ::2], [0, 2]).any()  # the comparison never selects a NaN
    if case == "default_row_wins":
        assert (arg[3] == 13).all()
    grad_out = np.random.default_rng(4).standard_normal((S, X.shape[1])).astype(np.float32)
    want = ref.backward(OPS[op], ids, None, grad_out, X.shape[0], arg)
    got = gpu_backward(OPS[op], ids, None, grad_out, X.shape[0], arg)
    assert ref.same_bits(got, want)
    if case == "all_below_start" and op == "max":
        assert not got[4].any()  # row 4 is referenced by that segment alone


@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("table", ["float16", "hashed", "host_pointers", "segment_ids", "dim_5"])
def test_recording_forward_on_other_tables_and_layouts(table, op):
    """emb / cnt equal glx_aggregate's for any storage type and id map; arg equals the restatement"""
    rng = np.random.default_rng(31)
    V, D, S = 40, 5 if table == "dim_5" else 12, 7
    X = rng.standard_normal((V, D)).astype(np.float32)
    keys = None
    if table == "float16":
        X = X.astype(np.float16)
    if table == "hashed":
        keys = rng.permutation(1000)[:V].astype(np.int64) * 7 + 3
    ids_rows = rng.integers(-1, V + 1, 35).astype(np.int64)  # rows; -1 and V: unknown ids
    ids = ids_rows if keys is None else np.where((ids_rows >= 0) & (ids_rows < V), keys[np.clip(ids_rows, 0, V - 1)], -5)
    seg = np.sort(rng.integers(0, S, 35)).astype(np.int32) if table == "segment_ids" else None
    f = glx.Features(X, ids=keys)
    if table == "host_pointers":
        emb0, cnt0 = f.aggregate(OPS[op], ids, seg, S, 0.25)
        emb, cnt, arg = f.aggregate_arg(OPS[op], ids, seg, S, 0.25)
    else:
        emb0, cnt0 = (t.cpu().numpy() for t in f.aggregate(OPS[op], _cuda(ids), _cuda(seg), S, 0.25))
        emb, cnt, arg = (t.cpu().numpy() for t in f.aggregate_arg(OPS[op], _cuda(ids), _cuda(seg), S, 0.25))
    assert ref.same_bits(emb, emb0) and np.array_equal(cnt, cnt0)
    start = ref.segment_starts(None if seg is None else cnt, len(ids), S)
    want_emb, want_arg = ref.fold_arg(OPS[op], X.astype(np.float32), ids_rows, start, 0.25)
    assert ref.same_bits(emb, want_emb) and np.array_equal(arg, want_arg)


@pytest.mark.parametrize("op", ["mean", "max"])
def test_identical_on_every_run_and_stream(op):
    """300 K positions over 20 K rows, three hub rows with lists of ~3000: five runs and one on a second stream"""
    import torch
    rng = np.random.default_rng(77)
    n, num_rows, D, S = 300000, 20000, 16, 30000
    rows = rng.integers(0, num_rows, n).astype(np.int64)
    hubs = rng.random(n) < 0.03
    rows[hubs] = rng.integers(0, 3, int(hubs.sum())) * 5000 + 17
    assert np.bincount(rows, minlength=num_rows).max() > 2000
    grad_out = rng.standard_normal((S, D)).astype(np.float32)
    arg = None
    if op == "max":
        X = rng.standard_normal((num_rows, D)).astype(np.float32)
        arg = X[rows].reshape(S, n // S, D).argmax(1).astype(np.int32) + (np.arange(S, dtype=np.int32) * (n // S))[:, None]
    want = ref.backward(OPS[op], rows, None, grad_out, num_rows, arg)
    d_rows, d_go, d_arg = _cuda(rows), _cuda(grad_out), _cuda(arg)
    runs = [glx.aggregate_backward(OPS[op], d_rows, None, d_go, num_rows, arg=d_arg) for _ in range(5)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(glx.aggregate_backward(OPS[op], d_rows, None, d_go, num_rows, arg=d_arg))
    side.synchronize()
    torch.cuda.synchronize()
    for r in runs:
        assert ref.same_bits(r.cpu().numpy(), want)


def test_offsets_beyond_2_31_elements():
    """num_rows = 2^23 + 1 at dim 256: grad_x is just over 2^31 elements; the last row, row 0 and a middle row"""
    import torch
    num_rows, D = (1 << 23) + 1, 256
    rows = np.array([num_rows - 1, 0, 5000001], np.int64)
    grad_out = np.random.default_rng(8).standard_normal((3, D)).astype(np.float32)
    grad_out[grad_out == 0] = 1.0
    out = torch.full((num_rows, D), float("nan"), dtype=torch.float32, device="cuda")
    glx.aggregate_backward(ref.SUM, _cuda(rows), None, _cuda(grad_out), num_rows, out=out)
    for k, r in enumerate(rows):
        assert ref.same_bits(out[int(r)].cpu().numpy(), (np.float32(0) + grad_out[k]).astype(np.float32))
    # every other element is +0.0: all of its bits are clear
    assert int(torch.count_nonzero(out.view(torch.int32))) == 3 * D
    del out
    torch.cuda.empty_cache()


def test_prod_has_no_backward():
    with pytest.raises(glx.GlxError) as e:
        glx.aggregate_backward(ref.PROD, _cuda(BASE_ROWS), None, _cuda(np.ones((3, 4), np.float32)), 7)
    assert e.value.code == 3 and "Prod" in str(e.value)


def test_empty_requests_write_zeros():
    import torch
    out = torch.full((5, 4), float("nan"), dtype=torch.float32, device="cuda")
    glx.aggregate_backward(ref.SUM, _cuda(np.zeros(0, np.int64)), None, _cuda(np.ones((3, 4), np.float32)), 5, out=out)
    assert ref.same_bits(out.cpu().numpy(), np.zeros((5, 4), np.float32))
    # fewer positions than segments: the implied fan-out is 0, nothing was consumed
    got = gpu_backward(ref.SUM, np.array([1, 2], np.int64), None, np.ones((3, 4), np.float32), 5)
    assert ref.same_bits(got, np.zeros((5, 4), np.float32))
