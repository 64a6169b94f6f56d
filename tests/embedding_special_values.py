"""Special-value inputs for glx_rows_coalesce and glx_embedding_update (tests/test_embedding_special_values_cpu.py,
tests/test_gpu_embedding_special_values.py; the contract is DESIGN.md 4, K5-emb, restated in embedding_ref.py).

Requests and tables built on purpose -- nothing is drawn at random except the order of positions: NaNs of both signs,
infinities, signed zeros, subnormals, FLT_MAX and 3e38 as the gradients of a coalesce (runs of one entry, runs inside
one chunk, runs of 257 / 513 / 1025 entries that cross GLX_COALESCE_CHUNK) and as the weights, gradients and optimizer
states of one SGD / Adagrad / Adam step, with eps 0, the default and 2^-149.  Plus the comparison rule the tests apply.
Test infrastructure only."""
import collections
import functools
import itertools

import numpy as np

import embedding_ref as eref
from agg_special_values import FLT_MAX, INF, NAN, NANS, SUB, SUB_BIG, SUB_MID, TINY, bits, f32

BIG = float(np.float32(3e38))   # 3e38 + 3e38 overflows float32; so does 3e38 * 3e38
HALF_TINY = 2.0 ** -127         # a subnormal: two of them are the smallest normal
CHUNK = eref.CHUNK
# what an output buffer holds before a call: one NaN that no input carries, compared as uint32 -- a NaN RESULT and an
# untouched canary are told apart by their bits, never by np.isnan
CANARY_BITS = 0x7FD5A5A5
assert CANARY_BITS not in set(int(b) for b in bits(NANS))


def canary(shape):
    return np.full(shape, CANARY_BITS, np.uint32).view(np.float32)


def is_canary(a):
    """True where the float32 array still holds the canary's bits"""
    return bits(a) == np.uint32(CANARY_BITS)


# ---- the comparison rule ------------------------------------------------------------------------------------------
def mismatch(got, want, moved=None):
    """Empty string when float32 `got` equals `want` under the rule, else a description of the first differences.
    Non-NaN elements: the same bits, the sign of zero included.  NaN positions: the same.  NaN payloads and signs: not
    compared -- every NaN these kernels emit is arithmetic, and x86 and gfx950 disagree on those -- except where `moved`
    (a boolean mask of the arrays' shape, or of their rows) is set: there the kernel must not have written at all, or
    only copied, and all 32 bits are compared."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    gb, wb = bits(got), bits(want)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & (gb != wb))
    if moved is not None:
        moved = np.asarray(moved, bool)
        if moved.ndim < got.ndim:
            moved = moved.reshape(moved.shape + (1,) * (got.ndim - moved.ndim))
        bad |= np.broadcast_to(moved, got.shape) & (gb != wb)
    if not bad.any():
        return ""
    idx = np.argwhere(bad)
    out = ["%d of %d elements differ" % (len(idx), bad.size)]
    for i in idx[:8]:
        i = tuple(i)
        out.append("  at %s: got %08x (%r) want %08x (%r)" % (i, gb[i], float(got[i]), wb[i], float(want[i])))
    return "\n".join(out)


# ---- coalesce scenarios -------------------------------------------------------------------------------------------
def _run(n, fill, at):
    """a run of n entries: `fill` (one value, or a cycle of values) everywhere but at the positions of `at`"""
    cycle = fill if isinstance(fill, (list, tuple)) else [fill]
    seq = [cycle[i % len(cycle)] for i in range(n)]
    for pos, v in at.items():
        assert 0 <= pos < n
        seq[pos] = v
    return seq


PLAIN = [1.5, -2.25, 3.0, 0.1, -7.0]

# (name, the fold-order g values of one column for one row, what the contract makes of them or None, outcome class).
# The expectation is a float (compared on bits), "nan", or None where only the restatements are asked.
Scenario = collections.namedtuple("Scenario", "name seq expect tag")
COALESCE = [Scenario(*s) for s in [
    # runs of one entry: +0.0 + g
    ("one -0.0", [-0.0], 0.0, "zero_from_negzero"),
    ("one +0.0", [0.0], 0.0, None),
    ("one nan", [NAN[2]], "nan", None),
    ("one -nan", [NAN[3]], "nan", None),
    ("one inf", [INF], INF, None),
    ("one -inf", [-INF], -INF, None),
    ("one 2^-149", [SUB], SUB, "subnormal_sum"),
    ("one -subnormal", [-SUB_MID], -SUB_MID, "subnormal_sum"),
    ("one largest subnormal", [SUB_BIG], SUB_BIG, "subnormal_sum"),
    ("one FLT_MAX", [FLT_MAX], FLT_MAX, None),
    ("one normal", [1.5], 1.5, None),
    # two entries
    ("-0.0 -0.0", [-0.0, -0.0], 0.0, "zero_from_negzero"),
    ("+0.0 -0.0", [0.0, -0.0], 0.0, None),
    ("-0.0 +0.0", [-0.0, 0.0], 0.0, None),
    ("inf -inf", [INF, -INF], "nan", "nan_in_reduce"),
    ("-inf inf", [-INF, INF], "nan", "nan_in_reduce"),
    ("inf inf", [INF, INF], INF, None),
    ("nan first of 2", [NAN[0], 1.0], "nan", None),
    ("nan last of 2", [1.0, NAN[1]], "nan", None),
    ("FLT_MAX + FLT_MAX", [FLT_MAX, FLT_MAX], INF, "inf_from_overflow"),
    ("-FLT_MAX - FLT_MAX", [-FLT_MAX, -FLT_MAX], -INF, "inf_from_overflow"),
    ("3e38 + 3e38", [BIG, BIG], INF, "inf_from_overflow"),
    ("FLT_MAX - FLT_MAX", [FLT_MAX, -FLT_MAX], 0.0, None),
    ("subnormals to 2^-126", [SUB_BIG, SUB], TINY, None),
    ("2^-127 twice", [HALF_TINY, HALF_TINY], TINY, None),
    ("subnormal + subnormal", [SUB_MID, SUB_MID], 2 * SUB_MID, "subnormal_sum"),
    ("2^-126 - 2^-149", [TINY, -SUB], SUB_BIG, "subnormal_sum"),
    ("2^-149 - 2^-149", [SUB, -SUB], 0.0, None),
    ("x - x", [1.5, -1.5], 0.0, None),
    # three entries
    ("-0.0 three times", [-0.0, -0.0, -0.0], 0.0, "zero_from_negzero"),
    ("-0.0 +0.0 -0.0", [-0.0, 0.0, -0.0], 0.0, None),
    ("nan first of 3", [NAN[4], 1.0, 2.0], "nan", None),
    ("nan middle of 3", [1.0, NAN[5], 2.0], "nan", None),
    ("nan last of 3", [1.0, 2.0, NAN[6]], "nan", None),
    ("nans only", [NAN[7], NAN[0], NAN[1]], "nan", None),
    ("inf 1 -inf", [INF, 1.0, -INF], "nan", "nan_in_reduce"),
    ("2^-149 three times", [SUB, SUB, SUB], 3 * SUB, "subnormal_sum"),
    ("mixed subnormals", [SUB_MID, SUB, -SUB_BIG], None, "subnormal_sum"),
    ("overflow then back", [FLT_MAX, FLT_MAX, -FLT_MAX], INF, "inf_from_overflow"),
    ("3e38 -3e38 3e38", [BIG, -BIG, BIG], BIG, None),
    # nine and seventy entries: past one pass of a lane group of 8 and of 64 (entry 8, entry 64 and later)
    ("-0.0 nine times", [-0.0] * 9, 0.0, "zero_from_negzero"),
    ("nan last of 9", _run(9, PLAIN, {8: NAN[2]}), "nan", None),
    ("inf first, -inf last of 9", _run(9, PLAIN, {0: INF, 8: -INF}), "nan", "nan_in_reduce"),
    ("subnormals, nine", _run(9, SUB_MID, {8: -SUB}), 8 * SUB_MID - SUB, "subnormal_sum"),
    ("-0.0 seventy times", [-0.0] * 70, 0.0, "zero_from_negzero"),
    ("nan at 69 of 70", _run(70, PLAIN, {69: NAN[3]}), "nan", None),
    ("inf at 1, -inf at 65 of 70", _run(70, 0.0, {1: INF, 65: -INF}), "nan", "nan_in_reduce"),
    ("2^-127 at 63 and 64 of 70", _run(70, -0.0, {63: HALF_TINY, 64: HALF_TINY}), TINY, None),
    # 257 entries: a full chunk and a chunk of one entry
    ("257: nan only in the last chunk", _run(257, PLAIN, {256: NAN[4]}), "nan", None),
    ("257: all -0.0", [-0.0] * 257, 0.0, "zero_from_negzero"),
    ("257: 2^-127 at 255 and 256", _run(257, 0.0, {255: HALF_TINY, 256: HALF_TINY}), TINY, "normal_from_subnormal_partials"),
    ("257: subnormal partials, subnormal sum", _run(257, -0.0, {3: SUB_MID, 200: SUB, 256: -SUB_BIG}), None,
     "subnormal_sum"),
    # 513 entries: two full chunks and a chunk of one entry
    ("513: inf in chunk 0, -inf in chunk 2", _run(513, 1.0, {3: INF, 512: -INF}), "nan", "nan_in_combine"),
    ("513: chunked order keeps 3e38", _run(513, 0.0, {0: BIG, 256: BIG, 257: -BIG}), BIG, "order"),
    ("513: chunked order overflows", _run(513, 0.0, {0: -BIG, 256: BIG, 257: BIG}), INF, "mirror"),
    ("513: nan only in the last chunk", _run(513, PLAIN, {512: NAN[5]}), "nan", None),
    # 1025 entries: four full chunks and a chunk of one entry
    ("1025: nan only in the last chunk", _run(1025, PLAIN, {1024: NAN[6]}), "nan", None),
    ("1025: FLT_MAX in chunks 1 and 4", _run(1025, -0.0, {300: FLT_MAX, 1024: FLT_MAX}), INF, "inf_in_combine"),
]]
LONG = CHUNK  # runs longer than this have more than one chunk
# what plain ascending order makes of the two order cases
PLAIN_ORDER = {"513: chunked order keeps 3e38": INF, "513: chunked order overflows": BIG}

# positions the coalesce must drop, each with the value that fills its whole g row: none of it may reach an output
DROPPED = [(-1, NAN[0]), (None, INF), (2 ** 40, -INF), (-(2 ** 40), NAN[5]), (-1, 1.0), (None, FLT_MAX),
           (2 ** 40, -0.0), (-(2 ** 40), 7.0), (-1, -INF), (None, NAN[7]), (2 ** 31, SUB), (-(2 ** 31) - 1, 3.5)]

CoalesceCase = collections.namedtuple("CoalesceCase", "rows g num_rows blocks dropped_at")


@functools.lru_cache(maxsize=None)
def build_coalesce(dim, seed=0, long=True, dropped_shift=0):
    """One request (rows[n] int64, g[n, dim] float32, num_rows) that holds every scenario, and where each went.

    The scenarios of one length L share table rows of L positions: column j of such a row carries scenario
    (j + offset) % count of that length, so neighbouring columns differ; enough rows that every scenario has a column,
    and for the short lengths one more row with another offset.  The rows' positions are interleaved at random (the
    order inside a row is the scenario's), the DROPPED positions are scattered among them; table rows 0, 3, 6, ..
    are referenced by nobody.  long=False leaves out the runs of more than one chunk.  dropped_shift rotates the values
    of the dropped positions among them.  blocks: (table row, [scenario index of each column]).  The arrays are shared
    and read-only.  About 1,900 positions from dim 4 on; dim 1 has one column, so every scenario needs a row of its own
    and the ten long runs alone are 5,130 positions."""
    rng = np.random.default_rng(1000 * dim + seed)
    by_len = collections.OrderedDict()
    for k, s in enumerate(COALESCE):
        if long or len(s.seq) <= LONG:
            by_len.setdefault(len(s.seq), []).append(k)
    cols = []  # per block: the scenario of each column
    for L, group in by_len.items():
        cover = -(-len(group) // dim)
        offsets = [k * dim for k in range(cover)] + ([dim + 8] if L <= 9 else [])
        for off in offsets:
            cols.append([group[(j + off) % len(group)] for j in range(dim)])
    B = len(cols)
    num_rows = 3 * B + 1
    table_row = 3 * rng.permutation(B) + 1 + rng.integers(0, 2, B)  # distinct, in [1, 3 B), not in block order
    lens = np.array([len(COALESCE[c[0]].seq) for c in cols])
    data = [np.stack([np.array(COALESCE[k].seq, np.float32) for k in c], axis=1) for c in cols]  # [L, dim] each
    drop = [(num_rows if r is None else r, DROPPED[(i + dropped_shift) % len(DROPPED)][1])
            for i, (r, _) in enumerate(DROPPED)]
    owner = np.concatenate([np.repeat(np.arange(B), lens), -1 - np.arange(len(drop))])
    # dropped_shift must move values only: the interleaving is drawn before it is looked at
    owner = owner[rng.permutation(len(owner))]
    n = len(owner)
    rows, g = np.empty(n, np.int64), np.empty((n, dim), np.float32)
    seen = np.zeros(B, np.int64)
    for i, o in enumerate(owner):
        if o < 0:
            rows[i], g[i] = drop[-1 - o]
        else:
            rows[i], g[i] = table_row[o], data[o][seen[o]]
            seen[o] += 1
    assert np.array_equal(seen, lens)
    for a in (rows, g):
        a.setflags(write=False)
    blocks = tuple((int(table_row[b]), tuple(cols[b])) for b in range(B))
    return CoalesceCase(rows, g, num_rows, blocks, tuple(np.flatnonzero(owner < 0).tolist()))


@functools.lru_cache(maxsize=None)
def expected_coalesce(dim, seed=0, long=True):
    """embedding_ref.coalesce of build_coalesce(dim, seed, long): (urows, ug, U), computed once, read-only"""
    case = build_coalesce(dim, seed, long)
    with np.errstate(all="ignore"):
        urows, ug, U = eref.coalesce(case.rows, case.g, case.num_rows)
    for a in (urows, ug):
        a.setflags(write=False)
    return urows, ug, U


def scenario_outputs(case, urows, ug):
    """[(scenario index, the element of ug that holds its sum)] over every column of every block"""
    at = {int(r): u for u, r in enumerate(urows) if r >= 0}
    return [(k, ug[at[row], j]) for row, cols in case.blocks for j, k in enumerate(cols)]


# ---- update scenarios ---------------------------------------------------------------------------------------------
ALGOS = (eref.SGD, eref.ADAGRAD, eref.ADAM)
# the gradient (and, under SGD, the weight) of an element.  1e-23 squared underflows to 0, 3e-23 squared to 2^-149,
# 1e-20 squared is a subnormal; 1e19 squared is a normal, 2e19 squared overflows
VALUES = [NAN[0], NAN[1], NAN[2], NAN[7], INF, -INF, 0.0, -0.0, SUB, -SUB, SUB_MID, SUB_BIG, -SUB_BIG, TINY, -TINY,
          FLT_MAX, -FLT_MAX, BIG, -BIG, 1.0, -1.5, 1e-20, -1e-23, 3e-23, 1e19, -2e19, 0.1]
# the weight of an element under Adagrad and Adam, where it only enters the last subtraction
WEIGHTS = [1.0, -0.0, SUB_MID, FLT_MAX, INF, NAN[1]]
# Adagrad's accumulator and Adam's second moment; Adam's first moment (signed)
STATES = [0.0, SUB_MID, 1.0, FLT_MAX, INF, NAN[2]]
MOMENTS = [0.0, -SUB_MID, 1.0, FLT_MAX, -INF, NAN[3]]
EPS = {eref.ADAGRAD: 1e-10, eref.ADAM: 1e-8}  # the optimizers' defaults


def scalar_sets(algo):
    """the (alpha, eps, beta1, c1, beta2, c2) of the steps every element takes: eps 0, the default and 2^-149, and one
    step with alpha = 0"""
    if algo == eref.SGD:
        return [(0.05, 0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]
    if algo == eref.ADAGRAD:
        return [(0.05, e, 0.0, 0.0, 0.0, 0.0) for e in (0.0, EPS[algo], SUB)] + [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]
    sets = [eref.adam_scalars(0.01, (0.9, 0.999), e, 1) for e in (0.0, EPS[algo], SUB)]
    return sets + [(0.0,) + sets[0][1:]]


def second_scalars(algo, sc):
    """the scalars of the step that follows a step with `sc`: Adam's step count moves on"""
    if algo != eref.ADAM or sc[0] == 0.0:
        return sc
    return eref.adam_scalars(0.01, (0.9, 0.999), sc[1], 2)


@functools.lru_cache(maxsize=None)
def elements(algo):
    """[E, 4] float32 (w, g, state1, state2) of every element: the cross product of the value lists"""
    if algo == eref.SGD:
        prod = [(w, g, 0.0, 0.0) for w, g in itertools.product(VALUES, VALUES)]
    elif algo == eref.ADAGRAD:
        prod = [(w, g, s, 0.0) for w, g, s in itertools.product(WEIGHTS, VALUES, STATES)]
    else:
        prod = list(itertools.product(WEIGHTS, VALUES, MOMENTS, STATES))
    e = np.array(prod, np.float32)
    e.setflags(write=False)
    return e


UpdateCase = collections.namedtuple("UpdateCase", "W state1 state2 urows ug elem")


@functools.lru_cache(maxsize=None)
def build_update(algo, dim, seed=0):
    """Tables and one step's (urows, ug) that put every element of elements(algo) into a row the step names.

    Element e sits at column e % dim of the (e // dim)-th named row (the last named row is filled up with the first
    elements again).  The named rows are scattered over the table in no order; between them lie rows the step does not
    name, full of the same special values (NaN payloads included), and urows carries entries of -1 and num_rows whose
    ug rows are NaN and inf.  elem[u, c]: the element of entry u's column c, -1 for an entry outside the table.  The
    arrays are shared and read-only: a test copies the tables before a step."""
    rng = np.random.default_rng(100 * dim + algo + seed)
    el = elements(algo)
    named = -(-len(el) // dim)
    V = named + max(8, named // 4)
    idx = np.arange(named * dim) % len(el)
    table_row = rng.permutation(V)[:named]
    fill = np.array(VALUES, np.float32)
    tables = [fill[(np.arange(V * dim) * (5, 7, 11)[k] + k) % len(fill)].reshape(V, dim).copy() for k in range(3)]
    for k, t in enumerate(tables):
        t[table_row] = el[idx, (0, 2, 3)[k]].reshape(named, dim)
    # the entries: every named row once, and entries outside the table among them
    outside = [(-1, NAN[0]), (V, INF), (-1, -INF), (V, 1.0), (-1, NAN[4])]
    owner = np.concatenate([np.arange(named), -1 - np.arange(len(outside))])
    owner = owner[rng.permutation(len(owner))]
    n = len(owner)
    urows, ug, elem = np.empty(n, np.int64), np.empty((n, dim), np.float32), np.full((n, dim), -1, np.int64)
    for u, o in enumerate(owner):
        if o < 0:
            urows[u], ug[u] = outside[-1 - o]
        else:
            urows[u] = table_row[o]
            elem[u] = idx[o * dim:(o + 1) * dim]
            ug[u] = el[elem[u], 1]
    states = {eref.SGD: 0, eref.ADAGRAD: 1, eref.ADAM: 2}[algo]
    out = [tables[0]] + [tables[k] if k <= states else None for k in (1, 2)] + [urows, ug, elem]
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return UpdateCase(*out)


@functools.lru_cache(maxsize=None)
def expected_update(algo, dim, which, seed=0):
    """the tables after the step with scalar_sets(algo)[which] and after the step that follows it:
    ((W, state1, state2), (W, state1, state2)) of embedding_ref.update, computed once, read-only"""
    case = build_update(algo, dim, seed)
    sc = scalar_sets(algo)[which]
    tabs = [None if t is None else t.copy() for t in (case.W, case.state1, case.state2)]
    out = []
    with np.errstate(all="ignore"):
        for scalars in (sc, second_scalars(algo, sc)):
            eref.update(algo, tabs[0], case.urows, case.ug, tabs[1], tabs[2], *scalars)
            snap = tuple(None if t is None else t.copy() for t in tabs)
            for t in snap:
                if t is not None:
                    t.setflags(write=False)
            out.append(snap)
    return tuple(out)


def named_rows(case):
    """boolean [V]: the rows of the table that the step names"""
    V = case.W.shape[0]
    m = np.zeros(V, bool)
    m[case.urows[(case.urows >= 0) & (case.urows < V)]] = True
    return m


# Cases called out by name: (name, algo, (w, g, state1, state2), index into scalar_sets(algo), the w after the step:
# a float compared on bits, "nan", or "kept" for the bits w had).  Each is an element of elements(algo).
Named = collections.namedtuple("Named", "name algo element which expect")
NAMED_UPDATES = [Named(*c) for c in [
    # g * g underflows to 0: den = 0, q = g / 0 = inf, alpha * inf = inf, w = 1 - inf
    ("adagrad: g 2^-149, state 0, eps 0", eref.ADAGRAD, (1.0, SUB, 0.0, 0.0), 0, -INF),
    ("adagrad: g 2^-149, state 0, eps 1e-10", eref.ADAGRAD, (1.0, SUB, 0.0, 0.0), 1, "kept"),
    ("adagrad: alpha 0 times q inf", eref.ADAGRAD, (1.0, SUB, 0.0, 0.0), 3, "nan"),
    ("adagrad: 0 / 0", eref.ADAGRAD, (1.0, 0.0, 0.0, 0.0), 0, "nan"),
    ("adagrad: -0 / 0", eref.ADAGRAD, (1.0, -0.0, 0.0, 0.0), 0, "nan"),
    ("adagrad: g 3e38, g * g inf, q 0", eref.ADAGRAD, (1.0, BIG, 0.0, 0.0), 0, "kept"),
    ("adagrad: g 3e38 on w -0.0", eref.ADAGRAD, (-0.0, BIG, 1.0, 0.0), 1, "kept"),
    ("adagrad: inf / inf", eref.ADAGRAD, (1.0, INF, 0.0, 0.0), 1, "nan"),
    ("adagrad: subnormal denominator", eref.ADAGRAD, (1.0, -1e-23, 0.0, 0.0), 2, None),
    ("sgd: w -0.0, g +0.0", eref.SGD, (-0.0, 0.0, 0.0, 0.0), 0, -0.0),
    ("sgd: w -0.0, g -0.0", eref.SGD, (-0.0, -0.0, 0.0, 0.0), 0, 0.0),
    ("sgd: alpha 0 times g inf", eref.SGD, (1.0, INF, 0.0, 0.0), 1, "nan"),
    ("sgd: inf - alpha * inf", eref.SGD, (INF, INF, 0.0, 0.0), 0, "nan"),
    # v and c2 * g * g subnormal: their sum is a subnormal whose square root is a normal
    ("adam: v subnormal, c2 g g subnormal", eref.ADAM, (1.0, 1e-20, 0.0, SUB_MID), 0, None),
    # v = 0 and g * g = 0: den = sqrt(0) + 2^-149, m / den overflows, w = 1 - alpha * inf
    ("adam: m over a subnormal den", eref.ADAM, (1.0, -1e-23, 1.0, 0.0), 2, -INF),
    ("adam: alpha 0 times q inf", eref.ADAM, (1.0, SUB, 1.0, 0.0), 3, "nan"),
    ("adam: 0 / 0", eref.ADAM, (1.0, 0.0, 0.0, 0.0), 0, "nan"),
    ("adam: g 3e38, v inf, q 0", eref.ADAM, (1.0, BIG, 1.0, 1.0), 1, "kept"),
    ("adam: inf / inf", eref.ADAM, (1.0, INF, 0.0, 0.0), 1, "nan"),
]]
