"""glx_columns: the device table of label / weight / timestamp / int-attribute records and its lookup kernel, against a
numpy gather with the reference's rules (memory_node_storage.cc:88-138, memory_edge_storage.cc:90-125): a column the
type lacks answers 0.0 / -1 / -1, an unknown id the caller's default.  Every comparison is bit for bit: the values are
moved, never converted, so a NaN's payload, -0.0 and a subnormal weight must arrive as they were stored."""
import ctypes
import itertools

import numpy as np
import pytest

import glx

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]  # wave and workgroup edges
I_NUMS = [0, 1, 3, 15, 16, 17, 40]  # records of 4 B .. 336 B: 8, 16, and just over every power of two of 16-byte pieces
SCALARS = ("weights", "labels", "timestamps")
SUBSETS = [s for r in range(4) for s in itertools.combinations(SCALARS, r)]
DEFAULTS = {"weights": float("nan"), "labels": 7, "timestamps": I64_MIN + 1, "int_attrs": -5}
LACKS = {"weights": np.float32(0.0), "labels": np.int32(-1), "timestamps": np.int64(-1)}
DTYPES = {"weights": np.float32, "labels": np.int32, "timestamps": np.int64, "int_attrs": np.int64}


def make_columns(rng, rows, i_num, has):
    """{name: array or None}; the first weights are a NaN with a payload, -0.0 and a subnormal."""
    cols = dict.fromkeys(glx.COLUMN_NAMES)
    if "weights" in has:
        w = rng.standard_normal(rows).astype(np.float32)
        special = np.array([0x7FC12345, 0x80000000, 0x00000003, 0xFF800001], np.uint32).view(np.float32)
        w[:min(rows, 4)] = special[:rows]
        cols["weights"] = w
    if "labels" in has:
        cols["labels"] = rng.integers(-2 ** 31, 2 ** 31, rows).astype(np.int32)
    if "timestamps" in has:
        cols["timestamps"] = rng.integers(-2 ** 63, 2 ** 63 - 1, rows, dtype=np.int64)
    if i_num > 0:
        cols["int_attrs"] = rng.integers(-2 ** 63, 2 ** 63 - 1, (rows, i_num), dtype=np.int64)
    return cols


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def expected(cols, i_num, rows_of_ids, want, defaults):
    """The numpy gather: rows_of_ids[i] is the row of request id i, -1 for an unknown id."""
    known = rows_of_ids >= 0
    r = np.where(known, rows_of_ids, 0)
    out = {}
    for name in want:
        dflt = np.array(defaults[name], DTYPES[name])
        if name == "int_attrs":
            got = np.full((len(r), i_num), dflt, np.int64)
            if i_num > 0 and cols[name].shape[0] > 0:
                got = np.where(known[:, None], cols[name][r], dflt)
        elif cols[name] is None:
            got = np.full(len(r), LACKS[name])
        elif cols[name].shape[0] == 0:
            got = np.full(len(r), dflt)
        else:  # select on the bits: a float NaN must keep its payload
            got = np.where(known, bits(cols[name])[r], bits(dflt)).view(DTYPES[name])
        out[name] = got.astype(DTYPES[name], copy=False)
    return out


def check(table, cols, i_num, ids, rows_of_ids, want=glx.COLUMN_NAMES, defaults=DEFAULTS, device=False):
    import torch
    q = torch.from_numpy(ids).cuda() if device else ids
    got = table.lookup(q, want=want, defaults=defaults)
    exp = expected(cols, i_num, rows_of_ids, want, defaults)
    assert set(got) == set(want)
    for name in want:
        g = got[name].cpu().numpy() if device else got[name]
        assert g.dtype == DTYPES[name] and g.shape == exp[name].shape, (name, g.dtype, g.shape)
        np.testing.assert_array_equal(bits(g), bits(exp[name]), err_msg=name)


def request(rng, ids, n, unknown):
    """n request ids: known ones (duplicates included) mixed with unknown ones; -> (ids, rows)"""
    pick = rng.integers(0, len(ids), n)
    q, rows = ids[pick].copy(), pick.astype(np.int64)
    bad = rng.random(n) < 0.25
    q[bad] = rng.choice(unknown, int(bad.sum()))
    rows[bad] = -1
    return q, rows


@pytest.mark.parametrize("has", SUBSETS, ids=lambda s: "+".join(s) or "none")
@pytest.mark.parametrize("i_num", I_NUMS)
def test_every_record_width_at_every_request_size(i_num, has):
    rng = np.random.default_rng(1000 * i_num + len(has))
    rows = 333
    cols = make_columns(rng, rows, i_num, has)
    ids = rng.permutation(np.arange(-400, 600, dtype=np.int64))[:rows]  # hashed, negative ids among them
    table = glx.Columns(rows, ids=ids, **cols)
    layout = glx.columns_layout(i_num, "weights" in has, "labels" in has, "timestamps" in has)
    assert table.record_bytes == layout["record_bytes"] and table.i_num == i_num
    assert table.has == {"weights": "weights" in has, "labels": "labels" in has, "timestamps": "timestamps" in has,
                         "int_attrs": i_num > 0}
    unknown = np.array([-401, 600, 10 ** 12, I64_MIN, np.iinfo(np.int64).max], np.int64)
    for k, n in enumerate(SIZES):
        q, r = request(rng, ids, n, unknown)
        check(table, cols, i_num, q, r, device=bool(k % 2))
        check(table, cols, i_num, q, r, device=not k % 2)


# 8-byte, 16-byte, 2- and 4-lane records, and one longer than 64 lanes x 16 B (the lane count caps: several rounds)
WIDTHS = [(0, ("labels",)), (1, ("weights", "labels")), (1, SCALARS), (3, SCALARS), (130, ("labels", "timestamps"))]


def build(kind, rng, rows, cols):
    """-> (table, ids, unknown ids, keep-alive)"""
    import torch
    if kind == "dense":
        return (glx.Columns(rows, **cols), np.arange(rows, dtype=np.int64), np.array([-1, rows, rows + 5, I64_MIN], np.int64),
                glx.COLUMNS_MAP_DENSE)
    if kind == "arithmetic":
        ids = 7 + 3 * np.arange(rows, dtype=np.int64)
        return (glx.Columns(rows, ids=ids, **cols), ids, np.array([6, 8, 9, 7 + 3 * rows, -2, I64_MIN], np.int64),
                glx.COLUMNS_MAP_OWN)
    ids = rng.permutation(np.arange(-5000, 5000, dtype=np.int64))[:rows] * 1000003
    unknown = np.array([1, -1, 999, I64_MIN, 5000 * 1000003], np.int64)
    if kind == "hashed":
        return glx.Columns(rows, ids=ids, **cols), ids, unknown, glx.COLUMNS_MAP_OWN
    feats = glx.Features(torch.zeros((rows, 4), device="cuda"), ids=torch.from_numpy(ids).cuda())
    return glx.Columns(rows, map_of=feats, **cols), ids, unknown, glx.COLUMNS_MAP_BORROWED


@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "i%d+%s" % (w[0], "+".join(x[0] for x in w[1])))
@pytest.mark.parametrize("kind", ["dense", "arithmetic", "hashed", "borrowed"])
def test_id_maps(kind, width):
    i_num, has = width
    rng = np.random.default_rng(77 + i_num)
    rows = 517
    cols = make_columns(rng, rows, i_num, has)
    table, ids, unknown, map_kind = build(kind, rng, rows, cols)
    assert table.id_map == map_kind and table.num_rows == rows
    q, r = request(rng, ids, 700, unknown)  # known (with duplicates) and unknown ids mixed
    q[:3], r[:3] = ids[5], 5  # a run of duplicates
    q[3], r[3] = I64_MIN, -1
    for device in (False, True):
        check(table, cols, i_num, q, r, device=device)
        check(table, cols, i_num, np.repeat(unknown, 40), np.full(40 * len(unknown), -1), device=device)  # all unknown
        first_last = np.array([ids[0], ids[-1]], np.int64)
        check(table, cols, i_num, first_last, np.array([0, rows - 1]), device=device)


@pytest.mark.parametrize("width", WIDTHS[:4], ids=lambda w: "i%d+%s" % (w[0], "+".join(x[0] for x in w[1])))
def test_edge_table_answers_defaults_outside_its_edge_ids(width):
    i_num, has = width
    E = 200
    cols = make_columns(np.random.default_rng(5), E, i_num, has)
    table = glx.Columns(E, **cols)
    q = np.array([-1, E, E - 1, 0, -1, E + 1], np.int64)
    r = np.array([-1, -1, E - 1, 0, -1, -1], np.int64)
    for device in (False, True):
        check(table, cols, i_num, q, r, device=device)


@pytest.mark.parametrize("width", WIDTHS[1:4], ids=lambda w: "i%d+%s" % (w[0], "+".join(x[0] for x in w[1])))
def test_every_subset_of_outputs(width):
    """the outputs that are not asked for are NULL pointers; a table that lacks a column answers the constant"""
    i_num, has = width
    rng = np.random.default_rng(9)
    rows = 130
    cols = make_columns(rng, rows, i_num, has)
    table = glx.Columns(rows, **cols)
    bare = glx.Columns(rows, weights=cols["weights"])  # lacks labels, timestamps and int attributes
    bare_cols = dict.fromkeys(glx.COLUMN_NAMES)
    bare_cols["weights"] = cols["weights"]
    q, r = request(rng, np.arange(rows, dtype=np.int64), 300, np.array([-1, rows], np.int64))
    for k in range(5):
        for want in itertools.combinations(glx.COLUMN_NAMES, k):
            for device in (False, True):
                check(table, cols, i_num, q, r, want=want, device=device)
                check(bare, bare_cols, 0, q, r, want=want, device=device)


def test_table_without_rows_or_without_columns():
    none = dict.fromkeys(glx.COLUMN_NAMES)
    table = glx.Columns(50)  # no column at all: every answer is the "type lacks it" constant
    assert table.record_bytes == 0
    q = np.array([0, 49, 50, -1, I64_MIN], np.int64)
    for device in (False, True):
        check(table, none, 0, q, np.array([0, 49, -1, -1, -1]), device=device)
    cols = make_columns(np.random.default_rng(1), 0, 3, SCALARS)
    empty = glx.Columns(0, ids=np.zeros(0, np.int64), **cols)  # every id is unknown
    for device in (False, True):
        check(empty, cols, 3, q, np.full(5, -1), device=device)


def test_pointer_kinds_and_a_second_stream():
    """a table built from CUDA tensors equals one built from numpy arrays; lookups take host or device pointers,
    and run on the caller's current stream"""
    import torch
    rng = np.random.default_rng(3)
    rows, i_num = 900, 5
    cols = make_columns(rng, rows, i_num, SCALARS)
    ids = rng.permutation(np.arange(10 ** 6, dtype=np.int64))[:rows]
    dev = {k: torch.from_numpy(v).cuda() for k, v in cols.items()}
    tables = [glx.Columns(rows, ids=ids, **cols), glx.Columns(rows, ids=torch.from_numpy(ids).cuda(), **dev)]
    q, r = request(rng, ids, 5000, np.array([-1, 10 ** 6], np.int64))
    for table in tables:
        for device in (False, True):
            check(table, cols, i_num, q, r, device=device)
    side = torch.cuda.Stream()
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = tables[1].lookup(dq, defaults=DEFAULTS)
    side.synchronize()
    exp = expected(cols, i_num, r, glx.COLUMN_NAMES, DEFAULTS)
    for name in glx.COLUMN_NAMES:
        np.testing.assert_array_equal(bits(got[name].cpu().numpy()), bits(exp[name]), err_msg=name)


def test_table_beyond_4_gib():
    """2^22 rows of 130 int attributes + a label: 1056-byte records, a 4.4 GB table -- byte offsets beyond 2^32, and
    more 16-byte pieces per record than a wave has lanes"""
    import torch
    rows, i_num = 1 << 22, 130
    ia = torch.arange(rows, device="cuda", dtype=torch.int64)[:, None] * 131 + torch.arange(i_num, device="cuda")
    labels = (torch.arange(rows, device="cuda", dtype=torch.int64) % 1000).to(torch.int32)
    table = glx.Columns(rows, labels=labels, int_attrs=ia)
    del ia
    assert table.record_bytes == 1056 and table.num_rows * table.record_bytes > 1 << 32
    rng = np.random.default_rng(8)
    q = np.concatenate([[0, rows - 1, rows, -1], rng.integers(0, rows, 1000)]).astype(np.int64)
    known = (q >= 0) & (q < rows)
    exp_ia = np.where(known[:, None], q[:, None] * 131 + np.arange(i_num), DEFAULTS["int_attrs"])
    exp_l = np.where(known, q % 1000, DEFAULTS["labels"]).astype(np.int32)
    for ids in (q, torch.from_numpy(q).cuda()):
        got = table.lookup(ids, want=("labels", "int_attrs"), defaults=DEFAULTS)
        got = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()}
        np.testing.assert_array_equal(got["int_attrs"], exp_ia)
        np.testing.assert_array_equal(got["labels"], exp_l)


def test_invalid_arguments():
    import torch
    L = glx.lib()
    ids = np.arange(4, dtype=np.int64)
    ia = np.zeros((4, 2), np.int64)
    feats = glx.Features(torch.zeros((4, 4), device="cuda"), ids=torch.from_numpy(ids).cuda())
    h = ctypes.c_void_p()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert L.glx_columns_create(0, 4, 0, None, None, None, None, p(ids), feats._h, 0, None, ctypes.byref(h)) == 3
    assert b"both ids and map_of" in L.glx_last_error() and not h.value
    assert L.glx_columns_create(0, 4, -1, None, None, None, None, None, None, 0, None, ctypes.byref(h)) == 3
    assert b"negative i_num" in L.glx_last_error() and not h.value
    assert L.glx_columns_create(0, 4, 0, None, None, None, p(ia), None, None, 0, None, ctypes.byref(h)) == 3
    assert b"int_attrs given with i_num == 0" in L.glx_last_error() and not h.value
    with pytest.raises(ValueError):
        glx.Columns(4).lookup(ids, want=("label",))
