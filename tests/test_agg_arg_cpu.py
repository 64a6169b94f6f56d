"""CPU tests of the recording forward's test cases (agg_arg_cases.py): the case lists keep reaching every launch path
of glx_aggregate_arg_kernel, the reference the GPU tests compare with (agg_backward_ref.fold_arg) agrees with a second,
vectorised statement of the contract on every case, and aggregate_arg's out= refuses buffers of the wrong shape or type
before any device use."""
import numpy as np
import pytest

import agg_arg_cases as cases
import agg_backward_ref as ref
import agg_special_values as sv
import glx

INVALID = 3
SPECIAL_DIMS = [3, 8, 100, 264]  # tests/test_gpu_agg_arg.py runs the same


def test_case_lists_reach_every_launch_path():
    """every (VEC, G, min(tiles, 3)) the launch rule can produce, no more and no fewer: trimming DIMS fails here"""
    assert cases.reached_paths() == cases.ALL_PATHS
    assert len(cases.ALL_PATHS) == 18
    aligned = {cases.launch_rule(d)[:2] for d in cases.DIMS}
    assert {g for v, g in aligned if v == 4} == {1, 2, 4, 8, 16, 32, 64}
    forced = {cases.launch_rule(d, out_aligned=False) for d in cases.MISALIGNED_DIMS}
    assert {v for v, _, _ in forced} == {1}
    # any one of the four conditions sends a multiple of 4 down the scalar path
    assert cases.launch_rule(8) == (4, 2, 1)
    assert cases.launch_rule(8, pitch=9)[0] == cases.launch_rule(8, table_aligned=False)[0] == 1
    assert cases.launch_rule(260) == (4, 64, 2) and cases.launch_rule(516) == (4, 64, 3)
    assert cases.launch_rule(129) == (1, 64, 3) and cases.launch_rule(33) == (1, 64, 1)


def test_segment_counts_sit_on_the_workgroup_edges():
    for G in (1, 2, 4, 8, 16, 32, 64):
        P = cases.segments_per_workgroup(G)
        assert P * G == 256
        S = cases.segment_counts(G)
        assert {P - 1, P, P + 1, 2 * P + 1, 1} <= set(S) and 0 not in S and len(set(S)) == len(S)
    for dim in cases.DIMS:
        for mis in ([False, True] if dim in cases.MISALIGNED_DIMS else [False]):
            _, G, _ = cases.launch_rule(dim, out_aligned=not mis)
            got = cases.launch_path_cases(dim, mis)
            for layout in (True, False):
                assert sorted(c.S for c in got if (c.seg is None) == layout) == cases.segment_counts(G), (dim, mis)


def test_lengths_and_tables_are_what_the_kernel_needs():
    assert cases.FANOUTS == [1, 3, 4, 5, 25]
    lengths = cases.long_lengths()
    assert lengths[0] == 0 and lengths[-1] == 0 and sorted(lengths[1:-1]) == cases.RAGGED_LENGTHS
    U = cases.UNROLL
    assert {U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1} <= set(cases.RAGGED_LENGTHS)
    assert [cases.launch_rule(d)[1:] for d in cases.UNROLL_DIMS] == [(1, 1), (32, 1), (64, 2)]
    for dim in cases.UNROLL_DIMS:
        got = cases.unroll_cases(dim)
        assert got[0].seg is not None and np.bincount(got[0].seg, minlength=got[0].S).tolist() == lengths.tolist()
        assert [len(c.rows) // c.S for c in got[1:]] == cases.FANOUTS
    for c in cases.all_cases():
        X = c.table(cases.MAX)
        assert X.shape == (c.V, c.dim) and X.dtype == np.float32
        band = cases.band_rows(c.V)
        rest = np.setdiff1d(np.arange(c.V), band)
        assert X[rest].min() >= -3 and X[rest].max() <= 3 and X[band].min() >= -40 and X[band].max() <= -36
        assert np.array_equal(X, np.round(X)) and np.array_equal(sv.half_upcast(X, "bfloat16"), X)
        assert np.array_equal(c.table(cases.MIN), -X)
        assert len(c.rows) <= 60000 and c.V <= 8192 + 5
        if len(c.rows) >= 8:
            assert -1 in c.rows and c.V in c.rows
    big = cases.owned_case(8192 + 5, 12)
    block = big.rows[(big.rows >= 0) & (big.rows < big.V)] // cases.SWIZZLE_BLOCK
    assert set(block.tolist()) == {0, 1, 2}  # two swizzled blocks and the tail


def _both(op, X, rows, start, default_attr):
    want = ref.fold_arg(op, X, rows, start, default_attr)
    got = cases.extreme_arg(op, X, rows, start, default_attr)
    assert np.array_equal(sv.bits(got[0]), sv.bits(want[0]))
    assert np.array_equal(got[1], want[1])
    return want


@pytest.mark.parametrize("op", [cases.MAX, cases.MIN], ids=["max", "min"])
def test_fold_arg_agrees_with_the_vectorised_statement(op):
    stayed = won = tied = 0
    for c in cases.all_cases():
        X, d = c.table(op), c.default(op)
        emb, arg = _both(op, X, c.rows, c.starts(), d)
        length = np.diff(c.starts())
        stayed += int(((arg == -1) & (length > 0)[:, None]).sum())
        unknown = (c.rows < 0) | (c.rows >= c.V)
        named = arg[arg >= 0]
        won += int(unknown[named].sum())
        tied += int((emb == 0).sum())
    # the start value (Max: the mirrored band is far below Min's FLT_MAX), a winning default_attr and ties all occur
    assert (stayed > 100) == (op == cases.MAX) and won > 100 and tied > 100


@pytest.mark.parametrize("op", [cases.MAX, cases.MIN], ids=["max", "min"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_fold_arg_agrees_on_the_special_values(dtype, op):
    for k, D in enumerate(SPECIAL_DIMS):
        X, ids, seg, Sg, d = sv.build_case(D, 200 + D, sv.DEFAULTS[k % len(sv.DEFAULTS)])
        up = X if dtype == "float32" else sv.half_upcast(X, dtype)
        start = ref.segment_starts(ref.cursor_counts(seg, Sg), len(ids), Sg)
        _both(op, up, ids, start, d)


# ---- out= ----------------------------------------------------------------------------------------------------
def _features_without_a_device(dim):
    """aggregate_arg's Python side needs only the row width; a NULL handle is refused by the entry point itself"""
    f = glx.Features.__new__(glx.Features)
    f._h, f.dim, f.device = None, dim, 0
    return f


def _good(S, D):
    return np.zeros((S, D), np.float32), np.zeros(S, np.int32), np.zeros((S, D), np.int32)


@pytest.mark.parametrize("which, bad", [
    ("emb", np.zeros((2, 3), np.float32)),      # a column short
    ("emb", np.zeros(8, np.float32)),           # flat
    ("emb", np.zeros((2, 4), np.float64)),
    ("counts", np.zeros(3, np.int32)),
    ("counts", np.zeros(2, np.int64)),
    ("arg", np.zeros((1, 4), np.int32)),        # a segment short
    ("arg", np.zeros((2, 4), np.float32)),
])
def test_out_of_another_shape_or_type_is_refused(which, bad):
    f = _features_without_a_device(4)
    out = dict(zip(("emb", "counts", "arg"), _good(2, 4)))
    out[which] = bad
    with pytest.raises(ValueError) as e:
        f.aggregate_arg(glx.MAX, np.zeros(4, np.int64), None, 2, out=(out["emb"], out["counts"], out["arg"]))
    assert which in str(e.value)
    with pytest.raises(ValueError):  # two buffers are not three
        f.aggregate_arg(glx.MAX, np.zeros(4, np.int64), None, 2, out=_good(2, 4)[:2])


def test_well_formed_out_reaches_the_entry_point_untouched():
    f = _features_without_a_device(4)
    emb, cnt, arg = _good(2, 4)
    emb[:], cnt[:], arg[:] = 7.0, 7, 7
    with pytest.raises(glx.GlxError) as e:
        f.aggregate_arg("MaxAggregator", np.zeros(4, np.int64), None, 2, out=(emb, cnt, arg))
    assert e.value.code == INVALID and "features is NULL" in str(e.value)
    assert (emb == 7.0).all() and (cnt == 7).all() and (arg == 7).all()
