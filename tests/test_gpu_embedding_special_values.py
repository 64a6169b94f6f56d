"""glx_rows_coalesce, glx_embedding_update and SparseEmbedding with its optimizers on the GPU, on NaN, inf, signed-zero,
subnormal and overflowing gradients, weights and optimizer states (tests/embedding_special_values.py), against the numpy
restatement of the contracts (embedding_ref.py; test_embedding_special_values_cpu.py pins it against a float64 twin).

Comparison (embedding_special_values.mismatch): non-NaN elements bit for bit, the sign of zero included; NaN positions
exactly; NaN payloads only where the kernel must not write or only moves a value.  Every output buffer starts as one
fixed NaN canary that no input carries, and "not written" is read off its bits."""
import os
import sys

import numpy as np
import pytest

import embedding_ref as eref
import embedding_special_values as sv
import glx
from agg_special_values import INF, NAN, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu
CANARY_ROW = -7
IGNORE = dict(all="ignore")


def _cuda(a, offset=False):
    """a CUDA copy of `a`; offset: 4 bytes into its buffer, so that it is not 16-byte aligned"""
    import torch
    a = np.array(a)  # a writable, contiguous copy: the scenario arrays are shared and read-only
    if not offset:
        return torch.from_numpy(a).cuda()
    assert a.dtype == np.float32
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _np(t):
    return t.detach().cpu().numpy()


# ---- coalesce -----------------------------------------------------------------------------------------------------
def gpu_coalesce(case, host=False, offset=False):
    """(urows, ug, count) as numpy / int from one call whose outputs start as canaries"""
    n, D = case.g.shape
    urows, ug = np.full(n, CANARY_ROW, np.int64), sv.canary((n, D))
    if host:
        _, _, count = glx.rows_coalesce(np.array(case.rows), np.array(case.g), case.num_rows, out_rows=urows, out_g=ug)
        return urows, ug, count
    d_urows, d_ug = _cuda(urows), _cuda(ug)
    d_g = _cuda(case.g, offset)
    assert d_ug.data_ptr() % 16 == 0 and d_g.data_ptr() % 16 == (4 if offset else 0)
    _, _, count = glx.rows_coalesce(_cuda(case.rows), d_g, case.num_rows, out_rows=d_urows, out_g=d_ug)
    assert count.is_cuda and count.numel() == 1  # no host read inside the call
    return _np(d_urows), _np(d_ug), int(count.cpu()[0])


def check_coalesce(got, want, label):
    urows, ug, count = got
    want_urows, want_ug, U = want
    assert count == U, label
    assert np.array_equal(urows, want_urows), (label, "urows: the distinct rows ascending, then -1")
    m = sv.mismatch(ug[:U], want_ug)
    assert not m, "%s\n%s" % (label, m)
    assert sv.is_canary(ug[U:]).all(), (label, "a row of ug past U was written")


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dim", [1, 3, 4, 64, 260])
def test_coalesce_every_scenario_on_every_launch_path(dim, offset):
    """one column per lane and four (dim 4, 64, 260 aligned), lane groups of 8 to 64, one column tile and two (260);
    device pointers twice -- the second call repeats the bits, arithmetic NaNs included --, host pointers once"""
    case, want = sv.build_coalesce(dim), sv.expected_coalesce(dim)
    first = gpu_coalesce(case, offset=offset)
    check_coalesce(first, want, "device")
    again = gpu_coalesce(case, offset=offset)
    check_coalesce(again, want, "device again")
    assert np.array_equal(bits(first[1]), bits(again[1]))
    if not offset:
        check_coalesce(gpu_coalesce(case, host=True), want, "host")
    # each scenario's own expectation, read off the device's output
    for k, value in sv.scenario_outputs(case, first[0], first[1]):
        s = sv.COALESCE[k]
        if s.expect == "nan":
            assert np.isnan(value), s.name
        elif s.expect is not None:
            assert bits(value) == bits(np.float32(s.expect)), (s.name, float(value))


@pytest.mark.parametrize("dim", [1, 3, 4, 64, 260])
def test_coalesce_of_short_runs_is_the_dense_sum_gradient(dim):
    """runs of at most 256 entries: the rows of glx_aggregate_backward's Sum are ug, under the rule; the rows nobody
    references are +0.0 although dropped positions hold NaN and inf"""
    case, (want_urows, want_ug, U) = sv.build_coalesce(dim, long=False), sv.expected_coalesce(dim, long=False)
    got = gpu_coalesce(case)
    check_coalesce(got, (want_urows, want_ug, U), "short runs")
    dense = _np(glx.aggregate_backward(glx.SUM, _cuda(case.rows), None, _cuda(case.g), case.num_rows))
    m = sv.mismatch(dense[want_urows[:U]], want_ug)
    assert not m, m
    assert not sv.mismatch(dense[want_urows[:U]], got[1][:U])
    untouched = np.setdiff1d(np.arange(case.num_rows), want_urows[:U])
    assert len(untouched) and not bits(dense[untouched]).any()


# ---- update -------------------------------------------------------------------------------------------------------
def _step_kw(sc):
    return dict(zip(("alpha", "eps", "beta1", "c1", "beta2", "c2"), sc))


def check_tables(d_tables, want, named, label):
    """the whole table and the whole state tables: rows the step names under the rule, every other row on all 32 bits"""
    for which, (d_t, w) in enumerate(zip(d_tables, want)):
        if w is None:
            continue
        m = sv.mismatch(_np(d_t), w, moved=~named)
        assert not m, "%s table %d\n%s" % (label, which, m)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dim", [1, 4, 64, 260])
@pytest.mark.parametrize("algo", sv.ALGOS)
def test_update_every_element_under_every_scalar_set(algo, dim, offset):
    """every (w, g, state) of the cross product under eps 0, the default, 2^-149 and with alpha 0; then a second step on
    the tables the first left, which reads the NaN, inf and subnormal states it wrote"""
    case = sv.build_update(algo, dim)
    named = sv.named_rows(case)
    d_urows, d_ug = _cuda(case.urows), _cuda(case.ug, offset)
    for which, sc in enumerate(sv.scalar_sets(algo)):
        d_tables = [None if t is None else _cuda(t, offset) for t in (case.W, case.state1, case.state2)]
        want = sv.expected_update(algo, dim, which)
        for step, scalars in enumerate((sc, sv.second_scalars(algo, sc))):
            glx.embedding_update(algo, d_tables[0], d_urows, d_ug, state1=d_tables[1], state2=d_tables[2],
                                 **_step_kw(scalars))
            check_tables(d_tables, want[step], named, "algo %d dim %d scalars %d step %d" % (algo, dim, which, step))


def test_named_update_cases_on_the_device():
    """the cases DESIGN.md and the scenarios call out by name, read off the device's tables one by one"""
    got = {}
    for c in sv.NAMED_UPDATES:
        key = (c.algo, c.which)
        if key not in got:
            case = sv.build_update(c.algo, 4)
            d = [None if t is None else _cuda(t) for t in (case.W, case.state1, case.state2)]
            glx.embedding_update(c.algo, d[0], _cuda(case.urows), _cuda(case.ug), state1=d[1], state2=d[2],
                                 **_step_kw(sv.scalar_sets(c.algo)[c.which]))
            got[key] = (case, _np(d[0]))
        case, W = got[key]
        el = sv.elements(c.algo)
        k = int(np.flatnonzero((bits(el) == bits(np.array(c.element, np.float32))).all(axis=1))[0])
        u, col = np.argwhere(case.elem == k)[0]
        w = W[case.urows[u], col]
        if c.expect == "nan":
            assert np.isnan(w), c.name
        elif c.expect is not None:
            expect = c.element[0] if c.expect == "kept" else c.expect
            assert bits(w) == bits(np.float32(expect)), (c.name, float(w))


@pytest.mark.parametrize("algo", sv.ALGOS)
def test_coalesce_feeds_the_update_without_a_host_read(algo):
    """the -1 tail of urows and the unwritten canary rows of ug go straight into a step over n entries: the U rows are
    the restatement's, nothing else in W or the states changes a bit, and ug's canaries are still there afterwards"""
    dim = 4
    case, (urows, ug, U) = sv.build_coalesce(dim), sv.expected_coalesce(dim)
    V, n = case.num_rows, len(case.rows)
    fill = np.array(sv.VALUES, np.float32)
    states = {eref.SGD: 0, eref.ADAGRAD: 1, eref.ADAM: 2}[algo]
    tables = [fill[(np.arange(V * dim) * (5, 7, 11)[k] + k) % len(fill)].reshape(V, dim).copy() if k <= states else None
              for k in range(3)]
    d_tables = [None if t is None else _cuda(t) for t in tables]
    sc = sv.scalar_sets(algo)[1 if algo != eref.SGD else 0]
    d_urows, d_ug, _ = glx.rows_coalesce(_cuda(case.rows), _cuda(case.g), V, out_g=_cuda(sv.canary((n, dim))))
    glx.embedding_update(algo, d_tables[0], d_urows, d_ug, state1=d_tables[1], state2=d_tables[2], **_step_kw(sc))
    with np.errstate(**IGNORE):
        eref.update(algo, tables[0], urows, ug, tables[1], tables[2], *sc)
    named = np.zeros(V, bool)
    named[urows[:U]] = True
    assert 0 < U < V
    check_tables(d_tables, tables, named, "coalesce into update, algo %d" % algo)
    assert sv.is_canary(_np(d_ug)[U:]).all() and (_np(d_urows)[U:] == -1).all()


# ---- SparseEmbedding and its optimizers ---------------------------------------------------------------------------
V, D, LR = 29, 12, 0.05


@pytest.fixture(scope="module")
def thg():
    import graphlearn.nn.pytorch as m
    return m


def _make(thg, algo, emb):
    return {eref.SGD: thg.SparseSGD, eref.ADAGRAD: thg.SparseAdagrad, eref.ADAM: thg.SparseAdam}[algo](emb, lr=LR)


def _ref_scalars(algo, t):
    if algo == eref.ADAM:
        return eref.adam_scalars(LR, (0.9, 0.999), 1e-8, t)
    return (LR, 1e-10 if algo == eref.ADAGRAD else 0.0, 0.0, 0.0, 0.0, 0.0)


def _ref_step(algo, W, states, ids, g, t, coalesce=True):
    with np.errstate(**IGNORE):
        if coalesce:
            ids, g, _ = eref.coalesce(ids, g, W.shape[0])
        eref.update(algo, W, ids, g, states[0], states[1], *_ref_scalars(algo, t))


def _module_step(emb, opt, ids, g, distinct=False):
    """forward, a backward that hands `g` to the module as it is, and the optimizer's step"""
    opt.zero_grad()
    emb(_cuda(ids), distinct=distinct).backward(_cuda(g))
    opt.step()


def _tables(emb, opt):
    return [_np(emb.weight)] + [None if opt.state[0][k] is None else _np(opt.state[0][k]) for k in ("state1", "state2")]


def _grad(shape, seed):
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(-10.0, 3.0, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@pytest.mark.parametrize("algo", sv.ALGOS)
def test_a_poisoned_batch_spoils_its_own_rows_only(thg, algo):
    """one id's gradient holds NaN, another's inf (one of its two positions): after step() those rows of the weight and
    of the states are what the restatement says, every row outside the batch keeps all its bits, and a clean step on
    other rows equals the restatement too -- the poisoned rows keeping theirs"""
    emb = thg.SparseEmbedding(V, D, seed=algo)
    opt = _make(thg, algo, emb)
    W = _np(emb.weight).copy()
    states = [np.zeros((V, D), np.float32) for _ in range({eref.SGD: 0, eref.ADAGRAD: 1}.get(algo, 2))] + [None, None]
    ids = np.array([3, 8, 20, 8, -1, 11, 20, V, 5], np.int64)
    g = _grad((len(ids), D), 60 + algo)
    g[2, :] = NAN[2]          # id 20, its first position: the whole row
    g[1, ::2] = INF           # id 8, its first position: every other column
    g[3, 1] = -INF            # id 8 again: +inf + -inf in no column (column 1 is finite above)
    g[4], g[7] = NAN[0], INF  # dropped positions
    _module_step(emb, opt, ids, g)
    _ref_step(algo, W, states, ids, g, 1)
    in_batch = np.zeros(V, bool)
    in_batch[[3, 5, 8, 11, 20]] = True
    got = _tables(emb, opt)
    for k, (t, w) in enumerate(zip(got, [W] + states[:2])):
        if w is not None:
            m = sv.mismatch(t, w, moved=~in_batch)
            assert not m, "table %d\n%s" % (k, m)
    # exactly the poisoned rows hold non-finite values, in the weight and wherever a state takes the gradient in
    spoiled = ~np.isfinite(got[0]).all(axis=1)
    assert np.flatnonzero(spoiled).tolist() == [8, 20] and np.isnan(got[0][20]).all()
    for t in got[1:]:
        if t is not None:
            assert np.flatnonzero(~np.isfinite(t).all(axis=1)).tolist() == [8, 20]
    # a clean step on other rows
    ids2 = np.array([1, 3, 1, 27, 0], np.int64)
    g2 = _grad((len(ids2), D), 70 + algo)
    before = [None if t is None else t.copy() for t in got]
    _module_step(emb, opt, ids2, g2)
    _ref_step(algo, W, states, ids2, g2, 2)
    in_batch2 = np.zeros(V, bool)
    in_batch2[ids2] = True
    after = _tables(emb, opt)
    for k, (t, w, b) in enumerate(zip(after, [W] + states[:2], before)):
        if w is not None:
            assert not sv.mismatch(t, w), k
            # outside the batch nothing is written: the bits the first step left, its arithmetic NaNs in rows 8 and 20
            # included (their signs and payloads are the device's, not the restatement's)
            assert np.array_equal(bits(t[~in_batch2]), bits(b[~in_batch2])), k
    assert np.isfinite(after[0][in_batch2]).all()


@pytest.mark.parametrize("algo", sv.ALGOS)
def test_distinct_and_coalesced_paths_differ_only_in_the_sign_of_a_zero(thg, algo):
    """-0.0 elements in the gradient on -0.0 elements of the weight: distinct=True hands -0.0 on as it is, the coalesce
    makes it +0.0.  Each path equals its restatement; the paths differ only in the sign of a zero, only where the two
    restatements differ, and under SGD and Adagrad they do differ (w = -0.0 - alpha * -0.0 against -0.0 - alpha * +0.0)"""
    import torch
    ids = np.random.default_rng(5).permutation(V + 1)[:13].astype(np.int64)  # distinct; V itself may be among them
    ids[4] = V
    g = _grad((len(ids), D), 80 + algo)
    g[:, 0], g[:, 5], g[::2, 7] = -0.0, 0.0, -0.0
    results = {}
    for distinct in (True, False):
        emb = thg.SparseEmbedding(V, D, seed=9)
        with torch.no_grad():
            emb.weight[:, 0], emb.weight[:, 5], emb.weight[:, 7], emb.weight[:, 2] = -0.0, -0.0, 0.0, -0.0
        opt = _make(thg, algo, emb)
        W = _np(emb.weight).copy()
        states = [np.zeros((V, D), np.float32) for _ in range({eref.SGD: 0, eref.ADAGRAD: 1}.get(algo, 2))] + [None, None]
        if algo == eref.ADAGRAD:  # a non-zero accumulator: 0 / (sqrt(s) + eps) is a zero with g's sign, not 0 / 0
            opt.state[0]["state1"] = torch.full_like(emb.weight, 0.25)
            states[0][:] = 0.25
        _module_step(emb, opt, ids, g, distinct=distinct)
        _ref_step(algo, W, states, ids, g, 1, coalesce=not distinct)
        got = _tables(emb, opt)
        touched = np.zeros(V, bool)
        touched[ids[ids < V]] = True
        for k, (t, w) in enumerate(zip(got, [W] + states[:2])):
            if w is not None:
                m = sv.mismatch(t, w, moved=~touched)
                assert not m, "distinct %s table %d\n%s" % (distinct, k, m)
        results[distinct] = (got, [W] + states[:2])
    differ_any = False
    for k in range(3):
        a, b = results[True][0][k], results[False][0][k]
        if a is None:
            continue
        wa, wb = results[True][1][k], results[False][1][k]
        differ = bits(a) != bits(b)
        assert np.array_equal(differ, bits(wa) != bits(wb)), k
        assert (a[differ] == 0).all() and (b[differ] == 0).all(), k  # zeros of opposite sign, nothing else
        differ_any |= bool(differ.any())
    assert differ_any == (algo != eref.ADAM)  # Adam's m = 0.9 * 0 + 0.1 * -0.0 is +0.0 on both paths
