"""CPU tests of the embedding special-value inputs (tests/embedding_special_values.py): the numpy restatement of the
contracts (embedding_ref.py) agrees on every scenario with a second restatement -- every operation carried out in
float64 and rounded to float32 at once --, the named cases give what the contract's text says, the restatement alone
produces every outcome class the GPU tests rely on (so none of them holds vacuously), and no dropped position's value
reaches an output."""
import numpy as np
import pytest

import embedding_ref as eref
import embedding_special_values as sv
from agg_special_values import NANS, bits

IGNORE = dict(all="ignore")


# ---- the second restatement ---------------------------------------------------------------------------------------
def _r(x):
    """round a float64 result to float32, and carry it on as a float64"""
    with np.errstate(**IGNORE):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def twin_sum(seq, chunk=eref.CHUNK):
    """the contract's sum of one column's float32 values in fold order, one float64 operation and one rounding at a
    time: +0.0 plus each chunk's partial, a partial +0.0 plus its entries.  A run of one chunk has no combine pass, but
    +0.0 + partial is the partial (a partial is never -0.0), so the same expression serves."""
    total = np.float64(0.0)
    with np.errstate(**IGNORE):
        for lo in range(0, len(seq), chunk):
            part = np.float64(0.0)
            for v in seq[lo:lo + chunk]:
                part = _r(part + np.float64(np.float32(v)))
            total = _r(total + part)
        return np.float32(total)


def twin_coalesce(rows, g, num_rows):
    """(urows, ug, U): the rows picked apart with plain Python, each column summed by twin_sum's rule"""
    lists = {}
    for p, r in enumerate(rows.tolist()):
        if 0 <= r < num_rows:
            lists.setdefault(r, []).append(p)
    uniq = sorted(lists)
    urows = np.full(len(rows), -1, np.int64)
    urows[:len(uniq)] = uniq
    ug = np.zeros((len(uniq), g.shape[1]), np.float32)
    g64 = g.astype(np.float64)
    for u, r in enumerate(uniq):
        at = lists[r]
        total = np.zeros(g.shape[1])
        for lo in range(0, len(at), eref.CHUNK):
            part = np.zeros(g.shape[1])
            for p in at[lo:lo + eref.CHUNK]:
                part = _r(part + g64[p])
            total = _r(total + part)
        ug[u] = total.astype(np.float32)
    return urows, ug, len(uniq)


def twin_update(algo, w, g, s1, s2, scalars):
    """one step on float32 arrays of elements -> (w, s1, s2), every operation in float64, rounded to float32 at once"""
    alpha, eps, beta1, c1, beta2, c2 = (np.float64(np.float32(x)) for x in scalars)
    w, g, s1, s2 = (None if a is None else np.asarray(a, np.float32).astype(np.float64) for a in (w, g, s1, s2))
    if algo == eref.SGD:
        w = _r(w - _r(alpha * g))
    elif algo == eref.ADAGRAD:
        s1 = _r(s1 + _r(g * g))
        den = _r(_r(np.sqrt(s1)) + eps)
        w = _r(w - _r(alpha * _r(g / den)))
    else:
        s1 = _r(_r(beta1 * s1) + _r(c1 * g))
        s2 = _r(_r(beta2 * s2) + _r(c2 * _r(g * g)))
        den = _r(_r(np.sqrt(s2)) + eps)
        w = _r(w - _r(alpha * _r(s1 / den)))
    return tuple(None if a is None else a.astype(np.float32) for a in (w, s1, s2))


def test_float64_then_round_is_the_float32_operation_on_these_operands():
    """53 >= 2 * 24 + 2: rounding the float64 result of + - * / sqrt of float32 operands gives the correctly rounded
    float32 result.  Seen here on the grid of the scenarios' own values and the values a step derives from them,
    subnormal results included, against numpy's float32 operators."""
    vals = [v for v in sv.VALUES + sv.STATES + sv.MOMENTS + [sv.HALF_TINY, 1e-10, 1e-8, 0.05, 0.9, 0.999, 0.001]]
    a = np.array(vals, np.float32)
    with np.errstate(**IGNORE):
        a = np.unique(np.concatenate([a, a * a, np.sqrt(np.abs(a)), a * np.float32(0.001)]).view(np.uint32)).view(np.float32)
        x, y = a[:, None], a[None, :]
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        seen_subnormal = 0
        for f in (np.add, np.subtract, np.multiply, np.divide):
            want, got = f(x, y), f(x64, y64).astype(np.float32)
            assert want.dtype == np.float32 and not sv.mismatch(got, want), f.__name__
            seen_subnormal += int(((want != 0) & (np.abs(want) < sv.TINY)).sum())
        want, got = np.sqrt(a), np.sqrt(a.astype(np.float64)).astype(np.float32)
        assert not sv.mismatch(got, want)
        assert np.sqrt(np.float32(sv.SUB)) >= np.float32(sv.TINY)  # the root of a subnormal is a normal
    assert seen_subnormal > 100


# ---- the comparison rule ------------------------------------------------------------------------------------------
def test_the_rule_ignores_nan_payloads_except_where_the_value_is_a_move():
    a = np.array([[NANS[0], 1.0], [0.0, NANS[2]]], np.float32)
    b = np.array([[NANS[1], 1.0], [0.0, NANS[3]]], np.float32)
    assert not sv.mismatch(a, b) and not sv.mismatch(a, a, moved=[True, True])
    assert "1 of 4" in sv.mismatch(a, b, moved=[False, True])  # by rows
    assert "2 of 4" in sv.mismatch(a, b, moved=np.ones((2, 2), bool))
    assert sv.mismatch(np.float32([0.0]), np.float32([-0.0])) and sv.mismatch(np.float32([np.nan]), np.float32([1.0]))
    assert sv.mismatch(np.float32([1.0]), np.float32([np.nan])) and sv.mismatch(np.zeros(2), np.zeros(3))
    c = sv.canary((2, 3))
    assert np.isnan(c).all() and sv.is_canary(c).all()
    c[0, 1] = np.float32(np.nan)  # a NaN result is not the canary
    assert sv.is_canary(c).sum() == 5
    # no input of any scenario carries the canary's bits
    for dim in (1, 4):
        assert not sv.is_canary(sv.build_coalesce(dim).g).any()
    for algo in sv.ALGOS:
        assert not sv.is_canary(sv.elements(algo)).any()


# ---- coalesce -----------------------------------------------------------------------------------------------------
def _expect_ok(value, expect):
    if expect == "nan":
        return bool(np.isnan(value))
    return bool(bits(np.float32(value)) == bits(np.float32(expect)))


def test_each_coalesce_scenario_gives_what_the_contract_says():
    """every scenario alone: the restatement, its float64 twin and the expectation written next to the scenario; the
    two order cases against plain ascending order"""
    names = [s.name for s in sv.COALESCE]
    assert len(set(names)) == len(names)
    lengths = set()
    with np.errstate(**IGNORE):
        for s in sv.COALESCE:
            rows, g = np.zeros(len(s.seq), np.int64), np.array(s.seq, np.float32)[:, None]
            _, ug, U = eref.coalesce(rows, g, 1)
            got = ug[0, 0]
            assert U == 1 and not sv.mismatch([got], [twin_sum(s.seq)]), s.name
            if s.expect is not None:
                assert _expect_ok(got, s.expect), (s.name, float(got))
            plain = eref.plain_sum(rows, g, 1)[1][0, 0]
            if s.name in sv.PLAIN_ORDER:
                assert _expect_ok(plain, sv.PLAIN_ORDER[s.name]) and not _expect_ok(plain, s.expect), s.name
            elif len(s.seq) <= sv.LONG:
                assert not sv.mismatch([plain], [got]), s.name
            lengths.add(len(s.seq))
    assert {1, 2, 3, 257, 513, 1025} <= lengths and set(sv.PLAIN_ORDER) <= set(names)
    # the 2^-127 pair across the chunk edge: both partials are subnormal, the combine makes the smallest normal
    s = sv.COALESCE[names.index("257: 2^-127 at 255 and 256")]
    assert twin_sum(s.seq[:256]) == np.float32(sv.HALF_TINY) == twin_sum(s.seq[256:]) and sv.HALF_TINY < sv.TINY
    assert twin_sum(s.seq) == np.float32(sv.TINY)


@pytest.mark.parametrize("dim", [1, 3, 4, 64, 260])
def test_the_request_holds_every_scenario_and_the_restatements_agree(dim):
    case = sv.build_coalesce(dim)
    urows, ug, U = sv.expected_coalesce(dim)
    n = len(case.rows)
    assert case.g.shape == (n, dim) and U == len(case.blocks) and n <= 6000
    # every scenario has a column; neighbouring columns differ; a block of three or more scenarios has different ones
    # in its first, a middle and its last column
    assert {k for _, cols in case.blocks for k in cols} == set(range(len(sv.COALESCE)))
    if dim >= 3:
        for _, cols in case.blocks:
            count = len(set(cols))
            assert count == 1 or all(a != b for a, b in zip(cols, cols[1:]))
            if count >= 3:
                assert any(len({cols[0], m, cols[-1]}) == 3 for m in cols[1:-1]), cols
        assert sum(len(set(cols)) >= 3 for _, cols in case.blocks) >= 5
    # rows: the blocks' table rows, rows nobody references between them, and every kind of dropped position
    valid = (case.rows >= 0) & (case.rows < case.num_rows)
    assert sorted(set(case.rows[valid].tolist())) == sorted(r for r, _ in case.blocks) == urows[:U].tolist()
    assert U < case.num_rows and (urows[U:] == -1).all()
    dropped = case.rows[~valid]
    assert sorted(np.flatnonzero(~valid).tolist()) == sorted(case.dropped_at)
    assert {-1, case.num_rows, 2 ** 40, -(2 ** 40)} <= set(dropped.tolist())
    gd = case.g[~valid]
    assert np.isnan(gd).any() and np.isinf(gd).any()
    # interleaved: the positions of a long row are not contiguous
    long_rows = [r for r, cols in case.blocks if len(sv.COALESCE[cols[0]].seq) > sv.LONG]
    assert len(long_rows) >= 3
    for r in long_rows:
        at = np.flatnonzero(case.rows == r)
        assert at[-1] - at[0] + 1 > len(at) + 100
    # the second restatement, on the whole request
    with np.errstate(**IGNORE):
        t_urows, t_ug, t_U = twin_coalesce(case.rows, case.g, case.num_rows)
    assert t_U == U and np.array_equal(t_urows, urows) and not sv.mismatch(ug, t_ug)
    # every scenario's element is what the scenario alone gives
    for k, value in sv.scenario_outputs(case, urows, ug):
        s = sv.COALESCE[k]
        assert not sv.mismatch([value], [twin_sum(s.seq)]), s.name
        assert s.expect is None or _expect_ok(value, s.expect), s.name
    # without the long runs nothing has more than one chunk
    short = sv.build_coalesce(dim, long=False)
    assert np.bincount(short.rows[(short.rows >= 0) & (short.rows < short.num_rows)]).max() <= sv.LONG
    with np.errstate(**IGNORE):
        plain = eref.plain_sum(short.rows, short.g, short.num_rows)[1]
    assert not sv.mismatch(sv.expected_coalesce(dim, long=False)[1], plain)


def test_the_restatement_alone_produces_every_coalesce_outcome():
    """counts of each outcome class in the expected output of one request: an edit to the scenarios cannot empty one"""
    case = sv.build_coalesce(4)
    urows, ug, U = sv.expected_coalesce(4)
    count = {}
    for k, value in sv.scenario_outputs(case, urows, ug):
        s = sv.COALESCE[k]
        seq = np.array(s.seq, np.float32)
        b = int(np.float32(value).view(np.uint32))
        sub = value != 0 and abs(float(value)) < sv.TINY
        ok = {
            "zero_from_negzero": b == 0 and (bits(seq) == 0x80000000).all(),
            "nan_in_reduce": np.isnan(value) and not np.isnan(seq).any() and len(seq) <= sv.LONG,
            "nan_in_combine": np.isnan(value) and not np.isnan(seq).any()
            and not any(np.isnan(twin_sum(s.seq[lo:lo + sv.CHUNK])) for lo in range(0, len(seq), sv.CHUNK)),
            "subnormal_sum": sub,
            "normal_from_subnormal_partials": len(seq) > sv.LONG and abs(float(value)) >= sv.TINY and np.isfinite(value)
            and all(abs(float(twin_sum(s.seq[lo:lo + sv.CHUNK]))) < sv.TINY for lo in range(0, len(seq), sv.CHUNK)),
            "inf_from_overflow": np.isinf(value) and np.isfinite(seq).all(),
            "inf_in_combine": np.isinf(value) and np.isfinite(seq).all()
            and all(np.isfinite(twin_sum(s.seq[lo:lo + sv.CHUNK])) for lo in range(0, len(seq), sv.CHUNK)),
            "order": np.isfinite(value) and s.name in sv.PLAIN_ORDER and np.isinf(sv.PLAIN_ORDER[s.name]),
            "mirror": np.isinf(value) and s.name in sv.PLAIN_ORDER and np.isfinite(sv.PLAIN_ORDER[s.name]),
        }
        if s.tag is not None:
            assert ok[s.tag], (s.name, s.tag, float(value))
        for tag, hit in ok.items():
            count[tag] = count.get(tag, 0) + int(bool(hit))
    for tag in ("zero_from_negzero", "nan_in_reduce", "nan_in_combine", "subnormal_sum",
                "normal_from_subnormal_partials", "inf_from_overflow", "inf_in_combine", "order", "mirror"):
        assert count.get(tag, 0) > 0, (tag, count)
    assert count["zero_from_negzero"] >= 5 and count["subnormal_sum"] >= 5 and count["nan_in_reduce"] >= 4


def test_no_dropped_position_reaches_an_output():
    """the dropped positions hold NaN, inf and FLT_MAX: rotating those values among them leaves every output bit, NaN
    payloads included, as it was -- and so does replacing them all by 1.0"""
    dim = 4
    base = sv.build_coalesce(dim)
    urows, ug, U = sv.expected_coalesce(dim)
    with np.errstate(**IGNORE):
        for shift in (1, 5):
            moved = sv.build_coalesce(dim, dropped_shift=shift)
            assert np.array_equal(moved.rows, base.rows)
            differ = np.flatnonzero((bits(moved.g) != bits(base.g)).any(axis=1))
            assert len(differ) >= 6 and set(differ.tolist()) <= set(base.dropped_at)
            nan_at = lambda c: {p for p in c.dropped_at if np.isnan(c.g[p]).any()}
            assert nan_at(moved) and nan_at(moved) != nan_at(base)
            m_urows, m_ug, m_U = eref.coalesce(moved.rows, moved.g, moved.num_rows)
            assert m_U == U and np.array_equal(m_urows, urows) and np.array_equal(bits(m_ug), bits(ug))
        g = base.g.copy()
        g[list(base.dropped_at)] = 1.0
        assert np.array_equal(bits(eref.coalesce(base.rows, g, base.num_rows)[1]), bits(ug))


# ---- update -------------------------------------------------------------------------------------------------------
def _find(algo, element):
    el = sv.elements(algo)
    hit = np.flatnonzero((bits(el) == bits(np.array(element, np.float32))).all(axis=1))
    assert len(hit) == 1, element
    return int(hit[0])


def _one(algo, element, scalars):
    """the restatement's step on one element -> (w, state1, state2) as float32 scalars"""
    tabs = [np.array([[v]], np.float32) for v in (element[0], element[2], element[3])]
    with np.errstate(**IGNORE):
        eref.update(algo, tabs[0], np.array([0], np.int64), np.array([[element[1]]], np.float32), tabs[1], tabs[2],
                    *scalars)
    return tuple(t[0, 0] for t in tabs)


def test_each_named_update_case_gives_what_the_contract_says():
    for c in sv.NAMED_UPDATES:
        _find(c.algo, c.element)  # it is one of the elements every step covers
        sc = sv.scalar_sets(c.algo)[c.which]
        w, s1, s2 = _one(c.algo, c.element, sc)
        expect = c.element[0] if c.expect == "kept" else c.expect
        assert expect is None or _expect_ok(w, expect), (c.name, float(w))
    f = np.float32
    with np.errstate(**IGNORE):
        # the intermediate values the names speak of
        assert f(sv.SUB) * f(sv.SUB) == 0 and np.isinf(f(sv.SUB) / f(0.0)) and np.isinf(f(sv.BIG) * f(sv.BIG))
        assert f(-1e-23) * f(-1e-23) == 0 and f(3e-23) * f(3e-23) == f(sv.SUB)
        gg = f(1e-20) * f(1e-20)
        assert 0 < gg < f(sv.TINY) and 0 < f(0.001) * gg < f(sv.TINY)
        c = [x for x in sv.NAMED_UPDATES if x.name == "adam: v subnormal, c2 g g subnormal"][0]
        w, m, v = _one(c.algo, c.element, sv.scalar_sets(c.algo)[c.which])
        assert 0 < v < f(sv.TINY) and np.sqrt(v) >= f(sv.TINY) and np.isfinite(w) and w != f(1.0)
        c = [x for x in sv.NAMED_UPDATES if x.name == "adam: m over a subnormal den"][0]
        w, m, v = _one(c.algo, c.element, sv.scalar_sets(c.algo)[c.which])
        assert v == 0 and m == f(0.9) and np.isinf(m / (np.sqrt(v) + f(sv.SUB)))
        c = [x for x in sv.NAMED_UPDATES if x.name == "adagrad: subnormal denominator"][0]
        w, s, _ = _one(c.algo, c.element, sv.scalar_sets(c.algo)[c.which])
        assert s == 0 and np.isfinite(w) and w > f(1e20)
    for algo in sv.ALGOS:
        sets = sv.scalar_sets(algo)
        assert any(s[0] == 0.0 for s in sets)
        if algo != eref.SGD:
            assert {f(s[1]) for s in sets} == {f(0.0), f(sv.EPS[algo]), f(sv.SUB)}


@pytest.mark.parametrize("dim", [1, 4, 64, 260])
@pytest.mark.parametrize("algo", sv.ALGOS)
def test_the_tables_hold_every_element_and_the_restatements_agree(algo, dim):
    case = sv.build_update(algo, dim)
    el = sv.elements(algo)
    V = case.W.shape[0]
    named = sv.named_rows(case)
    inside = (case.urows >= 0) & (case.urows < V)
    assert set(case.elem[inside].reshape(-1).tolist()) == set(range(len(el))) and (case.elem[~inside] == -1).all()
    assert {-1, V} <= set(case.urows[~inside].tolist()) and np.isnan(case.ug[~inside]).any()
    assert 8 <= (~named).sum() and named.sum() == inside.sum() == len(set(case.urows[inside].tolist()))
    assert np.isnan(case.W[~named]).any() and not np.all(np.diff(case.urows[inside]) > 0)
    tables = (case.W, case.state1, case.state2)
    for k, t in enumerate(tables):  # the tables hold the elements where elem says
        if t is not None:
            assert np.array_equal(bits(t[case.urows[inside]]), bits(el[case.elem[inside], (0, 2, 3)[k]]))
    assert np.array_equal(bits(case.ug[inside]), bits(el[case.elem[inside], 1]))
    for which, sc in enumerate(sv.scalar_sets(algo)):
        first, second = sv.expected_update(algo, dim, which)
        before = tables
        for after, scalars in ((first, sc), (second, sv.second_scalars(algo, sc))):
            with np.errstate(**IGNORE):
                r = case.urows[inside]
                twin = twin_update(algo, before[0][r], case.ug[inside], None if before[1] is None else before[1][r],
                                   None if before[2] is None else before[2][r], scalars)
            for t_before, t_after, t_twin in zip(before, after, twin):
                if t_before is None:
                    assert t_after is None
                    continue
                # rows the step does not name keep their bits; the named rows are the twin's
                assert np.array_equal(bits(t_after[~named]), bits(t_before[~named]))
                assert not sv.mismatch(t_after[r], t_twin), (algo, dim, which)
            before = after
        if sc[0] != 0.0:  # the second step moves the tables on
            assert any(t is not None and not np.array_equal(bits(t), bits(u)) for t, u in zip(first, second))


def _classes(a, before=None):
    a = np.asarray(a, np.float32)
    c = {"nan": int(np.isnan(a).sum()), "+inf": int((a == np.inf).sum()), "-inf": int((a == -np.inf).sum()),
         "subnormal": int(((a != 0) & (np.abs(a) < np.float32(sv.TINY))).sum())}
    if before is not None:
        c["kept"] = int(((bits(a) == bits(before)) & ~np.isnan(a)).sum())
    return c


@pytest.mark.parametrize("algo", sv.ALGOS)
def test_the_restatement_alone_produces_every_update_outcome(algo):
    """after the steps of every scalar set: weights that are NaN, +inf, -inf, subnormal and unchanged; states that are
    subnormal and inf -- among them NaNs whose inputs held no NaN and infinities whose inputs were all finite.  The second
    step reads such states."""
    case = sv.build_update(algo, 4)
    named = sv.named_rows(case)
    total, made = {}, {}
    for which in range(len(sv.scalar_sets(algo))):
        first, second = sv.expected_update(algo, 4, which)
        for key, n in _classes(first[0][named], case.W[named]).items():
            total["w " + key] = total.get("w " + key, 0) + n
        w0, w1 = case.W[named], first[0][named]
        inputs = [w0, _g_of(case, named)] + [t[named] for t in (case.state1, case.state2) if t is not None]
        no_nan = ~np.any([np.isnan(t) for t in inputs], axis=0)
        finite = np.all([np.isfinite(t) for t in inputs], axis=0)
        made["w nan"] = made.get("w nan", 0) + int((np.isnan(w1) & no_nan).sum())
        made["w inf"] = made.get("w inf", 0) + int((np.isinf(w1) & finite).sum())
        for k, t in enumerate(first[1:]):
            if t is not None:
                for key, n in _classes(t[named]).items():
                    total["s%d %s" % (k + 1, key)] = total.get("s%d %s" % (k + 1, key), 0) + n
        # the second step starts from states that hold NaN, inf and subnormals
        for t in first[1:]:
            if t is not None:
                c = _classes(t[named])
                assert c["nan"] and c["+inf"] and c["subnormal"], (algo, which, c)
    for key in ("w nan", "w +inf", "w -inf", "w subnormal", "w kept"):
        assert total[key] >= 12, (key, total)
    assert made["w nan"] >= 4 and made["w inf"] >= 4, made
    for k in range({eref.SGD: 0, eref.ADAGRAD: 1, eref.ADAM: 2}[algo]):
        for key in ("subnormal", "+inf", "nan"):
            assert total["s%d %s" % (k + 1, key)] >= 12, (k, key, total)


def _g_of(case, named):
    """the gradient of each named row, in table-row order"""
    V = case.W.shape[0]
    inside = np.flatnonzero((case.urows >= 0) & (case.urows < V))
    g = np.zeros(case.W.shape, np.float32)
    g[case.urows[inside]] = case.ug[inside]
    return g[named]


# ---- the two paths of SparseEmbedding -----------------------------------------------------------------------------
def test_the_distinct_path_differs_from_the_coalesced_one_only_in_the_sign_of_a_zero():
    """w -0.0 and g -0.0 under SGD: handed on as it is, w - alpha * -0.0 = +0.0; through the coalesce the gradient is
    +0.0 and w stays -0.0.  Nothing else differs, for any element of the SGD cross product without a repeated row."""
    el = sv.elements(eref.SGD)
    W = el[:, 0].reshape(-1, 1).copy()
    g = el[:, 1].reshape(-1, 1)
    ids = np.arange(len(el), dtype=np.int64)
    direct, through = W.copy(), W.copy()
    with np.errstate(**IGNORE):
        eref.update(eref.SGD, direct, ids, g, alpha=0.05)
        u, ug, _ = eref.coalesce(ids, g, len(el))
        eref.update(eref.SGD, through, u, ug, alpha=0.05)
    differ = [i for i in range(len(el)) if sv.mismatch(direct[i], through[i])]
    assert differ
    for i in differ:
        assert bits(g[i, 0]) == 0x80000000 and direct[i, 0] == 0 and through[i, 0] == 0
        assert bits(direct[i, 0]) != bits(through[i, 0])
    k = _find(eref.SGD, (-0.0, -0.0, 0.0, 0.0))
    assert k in differ and bits(direct[k, 0]) == 0 and bits(through[k, 0]) == 0x80000000
