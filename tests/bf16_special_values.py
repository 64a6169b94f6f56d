"""What the bfloat16 special-value tests share (test_bf16_special_values_cpu.py, test_gpu_bf16_special_values.py), built
with numpy only: the sixteen bfloat16 codes planted into tables, the requests that plant one of them per table row, and
the one-rounding cases of bf16_training_ref.ROUNDING_CASES extended and planted through each rounding kernel's own
arithmetic -- every product and quotient exact, so each kernel's float32 sum is the case's sum and its bfloat16 code the
one written in the table.  Nothing here comes from a GPU: the CPU test confirms every code three ways."""
import numpy as np

import agg_backward_ref as ref
import bf16_training_ref as b16

f32 = b16.f32


def P(e):
    return np.float32(2.0 ** e)


# quiet, negative quiet, signalling, negative signalling and all-ones NaN; +-inf; +-0; the smallest subnormals, the
# largest ones, the smallest normal; +-the largest finite value
SPECIAL_CODES = [0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0xFFFF, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F,
                 0x0080, 0x7F7F, 0xFF7F]
# the weight (or incoming gradient) that meets each code above: 0 and -0.0 against NaN and inf (inf x 0 and -inf x -0
# are NaN), inf against zeros and subnormals, a subnormal weight, and plain finite ones
SPECIAL_FACTORS = np.array([1.5, 0.0, -0.0, 1e-41, -2.0, 0.0, -0.0, np.inf, -np.inf, np.inf, 1e-41, 2.0, -0.5, 1e-41,
                            2.0, np.inf], np.float32)
FINITE_CODE = 0x3FC0  # 1.5: what stands in the planted cell of the finite twin of a request
NUM_SPECIAL = len(SPECIAL_CODES)
NUM_FINITE = 4
TABLE_ROWS = NUM_SPECIAL + NUM_FINITE
SPECIAL_SHAPES = [(6, 2), (12, 1), (48, 4), (260, 1)]


def planted_columns(dim):
    """a column of the first lane, the last column of the first tile (the group's last lane that has columns) and,
    where there is one, a column of the second column tile"""
    return [0, min(dim, 256) - 1] + ([257] if dim > 256 else [])


def _normal_codes(rng, shape):
    """finite bfloat16 codes of standard-normal values, truncated (any finite code serves)"""
    return (rng.standard_normal(shape).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def special_table(dim, col, seed, finite=False):
    """codes[TABLE_ROWS, dim]: row i < 16 holds SPECIAL_CODES[i] at column col (finite: FINITE_CODE), everything else
    is finite; the finite rows hold at most 0.5 in that column, so that no product with the largest finite code
    overflows in float32 where the float64 reference stays finite"""
    codes = _normal_codes(np.random.default_rng(1000 * dim + seed), (TABLE_ROWS, dim))
    codes[NUM_SPECIAL:, col] = np.array([0x3F00, 0xBE80, 0x3EC0, 0xBF00], np.uint16)  # 0.5, -0.25, 0.375, -0.5
    codes[:NUM_SPECIAL, col] = FINITE_CODE if finite else np.array(SPECIAL_CODES, np.uint16)
    return codes


def weighted_request(dim, heads, col):
    """(rows[60], w[60, heads], cnt[20], grad_out[20, dim]): segment s < 16 is the special row s (weight
    SPECIAL_FACTORS[s] in the planted column's head), a finite row and a row outside the table; 4 segments of finite
    rows; grad_out[s, col] = SPECIAL_FACTORS rotated by 5, so grad_w meets other pairings"""
    rng = np.random.default_rng(dim * 8 + heads)
    S = NUM_SPECIAL + 4
    rows = np.empty((S, 3), np.int64)
    rows[:, 0] = np.arange(S)
    rows[:, 1] = NUM_SPECIAL + np.arange(S) % NUM_FINITE
    rows[:, 2] = np.where(np.arange(S) % 2 == 0, -1, TABLE_ROWS)
    w = rng.standard_normal((S, 3, heads)).astype(np.float32)
    head = col // (dim // heads)
    w[:NUM_SPECIAL, 0, head] = SPECIAL_FACTORS
    grad_out = rng.standard_normal((S, dim)).astype(np.float32)
    grad_out[:NUM_SPECIAL, col] = np.roll(SPECIAL_FACTORS, 5)
    return rows.reshape(-1), w.reshape(S * 3, heads), np.full(S, 3, np.int32), grad_out


def pair_request(dim, heads, col):
    """(ia[36], ib[36], g[36, heads]): pair p < 16 joins special row p of xa with a finite row of xb, pair 16 + p a
    finite row of xa with special row p of xb, the last four have an index outside a table; g of the first 32 is
    SPECIAL_FACTORS in the planted column's head"""
    rng = np.random.default_rng(dim * 8 + heads + 1)
    sp, fin = np.arange(NUM_SPECIAL), NUM_SPECIAL + np.arange(NUM_SPECIAL) % NUM_FINITE
    ia = np.concatenate([sp, fin, [-1, 3, TABLE_ROWS, 17]]).astype(np.int64)
    ib = np.concatenate([fin, sp, [16, TABLE_ROWS, 18, -1]]).astype(np.int64)
    g = rng.standard_normal((len(ib), heads)).astype(np.float32)
    head = col // (dim // heads)
    g[:2 * NUM_SPECIAL, head] = np.tile(SPECIAL_FACTORS, 2)
    return ia, ib, g


# ---- one rounding ----------------------------------------------------------------------------------------------------
# (the float32 terms one row receives, in ascending position; the bfloat16 code of their float32 sum)
ROUNDING_CASES = b16.ROUNDING_CASES + [
    ([P(-135), P(-135)], 0x0000),                    # 2^-134, half the smallest bfloat16 subnormal: a tie: +0.0
    ([P(-134), P(-149)], 0x0001),                    # one float32 ulp above it: up
    ([np.float32(-(1.0 + 3 * 2.0 ** -8))], 0xBF82),  # a negative tie: to even, away from zero
    ([f32(0x7F7F0000), f32(0x7B000000)], 0x7F80),    # two finite terms, the finite sum 0x7F7F8000: +inf
    ([np.float32(-0.0)], 0x0000),                    # planted as a product of a negative weight and +0.0: +0.0 + -0.0
]
ACCUMULATION_CASE = 2  # its code needs the float32 sum: see per_add_rounding_code
NUM_CASES = len(ROUNDING_CASES)
ROUNDING_SHAPES = [(6, 2), (12, 1)]  # (dim, heads): the 2-byte stores of VEC 1 and the packed 8-byte store of VEC 4


def fold(terms):
    """the float32 sum of `terms`, folded left to right from +0.0 as the kernels do"""
    acc = np.float32(0.0)
    with np.errstate(all="ignore"):
        for t in terms:
            acc = np.float32(acc + np.float32(t))
    return acc


def rounding_sums():
    return np.array([fold(terms) for terms, _ in ROUNDING_CASES], np.float32)


def rounding_codes():
    return np.array([code for _, code in ROUNDING_CASES], np.uint16)


def per_add_rounding_code(terms, to_bf16):
    """the code a kernel that rounded its accumulator to bfloat16 after every add would store"""
    acc = np.float32(0.0)
    for t in terms:
        with np.errstate(all="ignore"):
            acc = b16.upcast(to_bf16(np.array([np.float32(acc + t)], np.float32)))[0]
    return int(to_bf16(np.array([acc], np.float32))[0])


def _bf16_exact(v):
    """v is a float32 whose low 16 bits are clear: a bfloat16 value (NaN: any)"""
    v = np.float32(v)
    return bool(np.isnan(v) or (np.array([v]).view(np.uint32)[0] & 0xFFFF) == 0)


def _same(a, b):
    a, b = np.array([a], np.float32), np.array([b], np.float32)
    return bool((np.isnan(a[0]) and np.isnan(b[0])) or a.view(np.uint32)[0] == b.view(np.uint32)[0])


def power_of_two_factor(t, need_bf16=False):
    """(w, v) with w a power of two (negative for the small terms: -0.0 becomes -0.5 x +0.0), w * v == t exactly in
    float32 and, if need_bf16, v a bfloat16 value; None where no such pair exists"""
    t = np.float32(t)
    big = not np.isfinite(t) or abs(t) >= 1.0
    with np.errstate(all="ignore"):
        for w in ([np.float32(2.0), P(16)] if big else [np.float32(-0.5), -P(-16), -P(-20)]):
            v = np.float32(t / w)
            if _same(np.float32(w * v), t) and (not need_bf16 or _bf16_exact(v)):
                return w, v
    return None


def split_bf16_terms(t):
    """t as a list of float32 terms of at most 8 significant bits each, leading bits first: every prefix sum is exact,
    and each term is a power of two times a bfloat16 value"""
    t = np.float32(t)
    if not np.isfinite(t) or t == 0:
        return [t]
    out = []
    rest = np.float64(t)
    while rest != 0:
        m, e = np.frexp(abs(rest))
        hi = np.copysign(np.floor(m * 256.0) / 256.0 * 2.0 ** e, rest)
        assert np.float64(np.float32(hi)) == hi
        out.append(np.float32(hi))
        rest = rest - hi
    return out


def split_below(t, limit_exp=126):
    """t as float32 terms all below 2^limit_exp in magnitude whose prefix sums are exact: seven of 2^(limit_exp - 1)
    and the rest -- for a kernel that reaches a term only as a quotient by 4"""
    t = np.float32(t)
    if not np.isfinite(t) or abs(t) < 2.0 ** limit_exp:
        return [t]
    step = np.copysign(P(limit_exp - 1), t)
    rest = np.float32(np.float64(t) - 7.0 * np.float64(step))
    assert np.float64(rest) + 7.0 * np.float64(step) == np.float64(t) and abs(rest) < 2.0 ** limit_exp
    return [step] * 7 + [rest]


def _expected(dim, cols=None):
    """(codes[NUM_CASES + 1, dim], float32 sums of the same shape): case r in row r (in `cols` only), a last row that
    nobody refers to"""
    codes = np.zeros((NUM_CASES + 1, dim), np.uint16)
    sums = np.zeros((NUM_CASES + 1, dim), np.float32)
    cols = slice(None) if cols is None else cols
    codes[:NUM_CASES, cols] = rounding_codes()[:, None]
    sums[:NUM_CASES, cols] = rounding_sums()[:, None]
    return codes, sums


def weighted_backward_x_rounding(op, dim, heads):
    """dict(rows, w, cnt, grad_out, num_rows, codes, sums) for glx_aggregate_weighted_backward_x.  Sum: one position per
    segment, w = 2 or -0.5 and grad_out = term / w.  Mean: the term's position opens a segment of 2 (w = 2) or 4
    (w = -0.5) positions whose others name no row, grad_out = term / w * count."""
    rows, w, cnt, go = [], [], [], []
    for r, (terms, _) in enumerate(ROUNDING_CASES):
        for t in terms:
            wt, v = power_of_two_factor(t)
            count = 1 if op == ref.SUM else (2 if wt > 0 else 4)
            rows += [r] + [-1] * (count - 1)
            w += [wt] + [np.float32(1.0)] * (count - 1)
            cnt.append(count)
            with np.errstate(all="ignore"):
                go.append(np.float32(v * np.float32(count)))
    codes, sums = _expected(dim)
    return dict(rows=np.array(rows, np.int64), w=np.repeat(np.array(w, np.float32)[:, None], heads, axis=1),
                cnt=np.array(cnt, np.int32), grad_out=np.repeat(np.array(go, np.float32)[:, None], dim, axis=1),
                num_rows=NUM_CASES + 1, codes=codes, sums=sums)


def pair_dot_backward_rounding(side, repeat, dim, heads):
    """dict(ia, ib, g, x_other (codes), num_rows, codes, sums) for glx_pair_dot_backward: every term is g, a power of
    two, times a bfloat16 value that fills its own row of x_other; the terms that need more than 8 bits are split.  Row
    0 of x_other is zeros: it pads side 0's groups of `repeat` pairs with +0.0 terms."""
    own, g, vals = [], [], [np.float32(0.0)]
    for r, (terms, _) in enumerate(ROUNDING_CASES):
        for t in terms:
            for piece in split_bf16_terms(t):
                gt, v = power_of_two_factor(piece, need_bf16=True)
                own.append(r)
                g.append(gt)
                vals.append(v)
    n = len(own)
    x_other = np.repeat((np.array(vals, np.float32).view(np.uint32) >> 16).astype(np.uint16)[:, None], dim, axis=1)
    if side == 1:  # the own side is ib: entry e of ia names term e's row, the first of its `repeat` pairs is the term
        ia = 1 + np.arange(n, dtype=np.int64)
        ib = np.full((n, repeat), -1, np.int64)
        ib[:, 0] = own
        gg = np.ones((n, repeat), np.float32)
        gg[:, 0] = g
    else:  # the own side is ia: a case's terms fill ceil(len / repeat) entries, padded with the row of zeros
        ia, ib, gg = [], [], []
        for r in range(NUM_CASES):
            mine = [k for k in range(n) if own[k] == r]
            while len(mine) % repeat:
                mine.append(-1)
            ia += [r] * (len(mine) // repeat)
            ib += [0 if k < 0 else 1 + k for k in mine]
            gg += [np.float32(1.0) if k < 0 else g[k] for k in mine]
        ia, ib, gg = np.array(ia, np.int64), np.array(ib, np.int64), np.array(gg, np.float32)
    codes, sums = _expected(dim)
    return dict(ia=ia, ib=np.ascontiguousarray(ib).reshape(-1),
                g=np.repeat(np.ascontiguousarray(gg).reshape(-1)[:, None], heads, axis=1), x_other=x_other,
                num_rows=NUM_CASES + 1, codes=codes, sums=sums)


def aggregate_backward_rounding(op, dim):
    """dict(rows, cnt, arg, grad_out, num_rows, codes, sums) for glx_aggregate_backward.  Sum: one position per segment.
    Mean: segments of count 4 whose first position is the term's and whose others name no row, grad_out = 4 * term (a
    term of 2^126 or more in eight pieces).  Max / Min: segments of two positions, the first the term's row and the
    second no row; arg routes the even columns to the first and the odd ones to the second, so a one-term case is one
    segment routing to its row and the others are two or more."""
    rows, cnt, go = [], [], []
    for r, (terms, _) in enumerate(ROUNDING_CASES):
        for t in terms:
            for piece in (split_below(t) if op == ref.MEAN else [t]):
                count = {ref.SUM: 1, ref.MEAN: 4}.get(op, 2)
                rows += [r] + [-1] * (count - 1)
                cnt.append(count)
                with np.errstate(all="ignore"):
                    go.append(np.float32(piece * np.float32(4.0)) if op == ref.MEAN else np.float32(piece))
    S = len(cnt)
    arg, cols = None, None
    if op in (ref.MAX, ref.MIN):
        arg = np.empty((S, dim), np.int32)
        arg[:, 0::2] = 2 * np.arange(S, dtype=np.int32)[:, None]
        arg[:, 1::2] = 2 * np.arange(S, dtype=np.int32)[:, None] + 1
        cols = slice(0, None, 2)
    codes, sums = _expected(dim, cols)
    return dict(rows=np.array(rows, np.int64), cnt=np.array(cnt, np.int32), arg=arg,
                grad_out=np.repeat(np.array(go, np.float32)[:, None], dim, axis=1), num_rows=NUM_CASES + 1, codes=codes,
                sums=sums)
