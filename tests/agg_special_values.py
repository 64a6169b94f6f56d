"""Special-value inputs for the aggregation reduce and the lookup (tests/test_agg_special_values_cpu.py,
tests/test_gpu_agg_special_values.py, tests/golden/make_golden.py gen_agg_special).

Feature tables and segments built on purpose -- not drawn at random -- so that every case below is actually reduced:
NaNs (both signs, several payloads, first / middle / last in a segment, segments of NaNs only), infinities of both
signs together and next to 0, signed zeros in both orders, subnormal elements, sums and means of subnormals, products
that underflow into the subnormal range, sums and products that overflow, and values on both sides of Max's -37
initialiser.  Plus a plain sequential float32 model of the reference's InitFunc / AggFunc / FinalFunc and of
AggregatingResponse::Stitch, and the comparison rule the tests apply to NaNs.  Test infrastructure only."""
import numpy as np

AGGREGATORS = ["SumAggregator", "MeanAggregator", "MaxAggregator", "MinAggregator", "ProdAggregator"]
F32 = np.finfo(np.float32)
FLT_MAX = float(F32.max)


def f32(u):
    """float32 values of uint32 bit patterns."""
    return np.array(u, np.uint32).view(np.float32)


# quiet NaNs: both signs, several payloads
NANS = f32([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC0BEEF, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FD00001, 0xFFE54321])
NAN = [float(x) for x in NANS]  # the Python floats keep the bits (they round-trip through float64 and back exactly)
INF = float("inf")
SUB = float(F32.smallest_subnormal)   # 2^-149
SUB_BIG = float(f32(0x007FFFFF))      # the largest subnormal
SUB_MID = float(f32(0x00012345))
TINY = float(F32.tiny)                # 2^-126, the smallest normal
BELOW_37 = float(np.nextafter(np.float32(-37.0), np.float32(-np.inf)))
ABOVE_37 = float(np.nextafter(np.float32(-37.0), np.float32(0.0)))
# default_attr values the special-value tests use for unknown ids and empty segments
DEFAULTS = [NAN[2], -INF, -0.0, SUB_MID]

# Every scenario is the sequence of one column's values down a segment, in fold order.
SCENARIOS = [
    # NaN
    [NAN[0]], [1.0, NAN[1], 2.0], [NAN[2], 3.0, -4.0], [5.0, -6.0, NAN[3]], [NAN[4], NAN[5], NAN[6]],
    [NAN[7], 7.5], [-8.0, NAN[1]], [INF, NAN[2]], [NAN[0], -INF], [-INF, NAN[3], INF], [0.0, NAN[5], -0.0],
    [SUB, NAN[6]], [NAN[1], NAN[0]],
    # infinities
    [INF, -INF], [-INF, INF], [INF, 0.0], [-0.0, -INF], [INF], [-INF], [INF, 1.0], [-INF, -1.0], [INF, INF],
    [-INF, -INF, 2.0], [FLT_MAX, INF], [-FLT_MAX, -INF],
    # signed zero
    [0.0, -0.0], [-0.0, 0.0], [-0.0], [0.0], [-0.0, -0.0], [-0.0, 5.0], [-1.0, -0.0], [-0.0, 2.0], [3.0, -3.0],
    [-0.0, -0.0, -0.0], [-0.0, -40.0], [-40.0, -0.0], [0.0, -40.0, -0.0],
    # subnormals
    [SUB], [-SUB], [SUB, SUB, SUB], [SUB_BIG, SUB_BIG], [SUB_MID, -SUB_MID], [SUB_MID, SUB, -SUB_BIG],
    [1e-20, 1e-20], [1e-30, 1e-10, 1e-5], [SUB, 0.5], [3 * SUB, 0.5], [SUB_BIG, 2.0], [TINY, -SUB], [TINY, -TINY * 0.75],
    [1e-38, 1e-38, 1e-38], [-SUB_MID, -SUB_MID, SUB], [SUB, -0.0], [1e-45, 1e-45],
    # overflow
    [FLT_MAX, FLT_MAX], [FLT_MAX, FLT_MAX, -FLT_MAX], [-FLT_MAX, -FLT_MAX], [1e20, 1e20], [-FLT_MAX, 2.0],
    [1e30, 1e30, 0.0], [FLT_MAX, -FLT_MAX], [3e38, 3e38, 3e38],
    # around Max's -37 start
    [BELOW_37], [ABOVE_37], [-37.0], [-37.0, BELOW_37], [BELOW_37, ABOVE_37], [-50.0, -38.0], [-100.0, ABOVE_37, -36.0],
    # plain values between them
    [1.5, -2.25, 3.0], [0.1, 0.2, 0.3, 0.4], [-7.0, 11.0, 13.5, -0.5, 2.0],
]

# one pool of single values, for the rows drawn at random
POOL = sorted({float(v) for s in SCENARIOS for v in s if v == v}, key=lambda v: (v, np.copysign(1.0, v))) + NAN


def _as32(seq):
    return np.array(seq, np.float32)


def build_case(D, seed, default_attr, blocks=2, random_segments=80, empty=True):
    """A feature table [V, D] float32, a request (ids, segment ids, number of segments) and its default_attr.

    Scenario block: for each scenario length n, the scenarios of that length fill the columns of n fresh rows in turn
    (column j of a block takes scenario (j + offset) % count, several offsets), one segment takes those n rows in order -- so
    every scenario is reduced in several lanes and vector slots.  Then segments of random rows of special values
    (random lengths, unknown ids for default_attr, empty segments).  Dense ids (row = id)."""
    rng = np.random.default_rng(seed)
    by_len = {}
    for s in SCENARIOS:
        by_len.setdefault(len(s), []).append(_as32(s))
    rows, seg_rows = [], []
    for n in sorted(by_len):
        group = by_len[n]
        cover = -(-len(group) // D)  # blocks until every scenario of this length has a column
        for off in [k * D for k in range(cover)] + [k * (D + 7) + 1 for k in range(1, blocks)]:
            block = np.stack([group[(j + off) % len(group)] for j in range(D)], axis=1)
            base = sum(r.shape[0] for r in rows)
            rows.append(block)
            seg_rows.append(list(range(base, base + n)))
    n_fixed = sum(r.shape[0] for r in rows)
    pool = _as32(POOL)
    R = max(64, 2 * D)
    rnd = pool[rng.integers(0, pool.shape[0], (R, D))]
    normal = rng.random((R, D)) < 0.3
    rnd[normal] = (rng.standard_normal(int(normal.sum())) * 4).astype(np.float32)
    rows.append(rnd)
    X = np.concatenate(rows).astype(np.float32)
    V = X.shape[0]
    segs = list(seg_rows)
    for _ in range(random_segments):
        L = int(rng.integers(0 if empty else 1, 9))
        ids = list(n_fixed + rng.integers(0, R, L))
        for i in range(L):
            u = rng.random()
            if u < 0.08:
                ids[i] = 10 ** 9          # unknown id: the default row
            elif u < 0.12:
                ids[i] = -1
            elif u < 0.3:
                ids[i] = int(rng.integers(0, n_fixed))  # a scenario row
        segs.append(ids)
    if empty:
        segs.insert(len(seg_rows) // 2, [])
        segs.append([])
        segs.append([10 ** 9])  # only unknown ids: Sum folds default_attr into 0.0
    order = rng.permutation(len(segs) - len(seg_rows)) + len(seg_rows)
    segs = segs[:len(seg_rows)] + [segs[i] for i in order]
    Sg = len(segs)
    ids = np.array([i for s in segs for i in s], np.int64)
    seg = np.repeat(np.arange(Sg, dtype=np.int32), [len(s) for s in segs])
    return X, ids, seg, Sg, np.float32(default_attr)


# ---- a plain model of the reference's operator, written from aggregator.cc / {sum,mean,max,min,prod}_aggregator.cc
def model_aggregate(X, op, ids, seg, Sg, default_attr, raw=None):
    """Sequential float32 fold: the reference's Aggregator::Aggregate, with its segment cursor (ids are consumed in
    order while their segment id equals the current segment; the first that does not stalls the cursor)."""
    X = np.asarray(X, np.float32)
    D = X.shape[1]
    index = {int(r): i for i, r in enumerate(raw)} if raw is not None else None
    dflt = np.full(D, default_attr, np.float32)
    init = {"MaxAggregator": -37.0, "MinAggregator": FLT_MAX, "ProdAggregator": 1.0}.get(op, 0.0)
    emb = np.zeros((Sg, D), np.float32)
    cnt = np.zeros(Sg, np.int32)
    cur = 0
    with np.errstate(all="ignore"):
        for s in range(Sg):
            acc = np.full(D, init, np.float32)
            n = 0
            while cur < len(ids) and seg[cur] == s:
                i = int(ids[cur])
                row = index.get(i, -1) if index is not None else (i if 0 <= i < X.shape[0] else -1)
                a = X[row] if row >= 0 else dflt
                cur += 1
                n += 1
                if op in ("SumAggregator", "MeanAggregator"):
                    acc = acc + a
                elif op == "MaxAggregator":
                    acc = np.where(acc < a, a, acc)   # std::max(l, r)
                elif op == "MinAggregator":
                    acc = np.where(a < acc, a, acc)   # std::min(l, r)
                else:
                    acc = acc * a
            if n == 0:
                acc = dflt.copy()
            elif op == "MeanAggregator":
                acc = acc / np.float32(n)
            emb[s], cnt[s] = acc, n
    return emb, cnt


def model_stitch(op, parts, cnts, default_attr, reference_fold=False):
    """AggregatingResponse::Stitch: fold the partial responses in shard order from InitFunc's value (Mean:
    left += right * cnt), skipping the partials of count 0 unless reference_fold; then FinalFunc on the total."""
    P, Sg, D = parts.shape
    init = {"MaxAggregator": -37.0, "MinAggregator": FLT_MAX, "ProdAggregator": 1.0}.get(op, 0.0)
    emb = np.zeros((Sg, D), np.float32)
    cnt = np.zeros(Sg, np.int32)
    with np.errstate(all="ignore"):
        for s in range(Sg):
            acc = np.full(D, init, np.float32)
            total = 0
            for p in range(P):
                c, a = int(cnts[p, s]), parts[p, s]
                if c == 0 and not reference_fold:
                    continue
                if op == "SumAggregator":
                    acc = acc + a
                elif op == "MeanAggregator":
                    acc = acc + a * np.float32(c)
                elif op == "MaxAggregator":
                    acc = np.where(acc < a, a, acc)
                elif op == "MinAggregator":
                    acc = np.where(a < acc, a, acc)
                else:
                    acc = acc * a
                total += c
            if total == 0:
                acc = np.full(D, default_attr, np.float32)
            elif op == "MeanAggregator":
                acc = acc / np.float32(total)
            emb[s], cnt[s] = acc, total
    return emb, cnt


# ---- half tables ----------------------------------------------------------------------------------------------------
def half_upcast(X, dtype):
    """The float32 values a table uploaded as `dtype` ("bfloat16" / "float16") holds: each element rounded to nearest
    even (inf on overflow, half subnormals kept), NaNs as the upload stores them -- bfloat16 0xFFFF; float16 the sign,
    the quiet bit and the top ten payload bits -- then widened exactly.  Plain integer / numpy arithmetic, so the
    expectation does not depend on which of torch's conversion loops (vectorised, or the scalar one for chunk tails,
    which drops float16 payloads) handled an element."""
    X = np.ascontiguousarray(X, np.float32)
    u = X.view(np.uint32).astype(np.uint64)
    nan = np.isnan(X)
    if dtype == "bfloat16":
        b = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
        b[nan] = 0xFFFF
        return (b << 16).astype(np.uint32).view(np.float32)
    assert dtype == "float16", dtype
    with np.errstate(all="ignore"):
        h = X.astype(np.float16).view(np.uint16).astype(np.uint64)
    h[nan] = (((u >> 16) & 0x8000) | 0x7E00 | ((u >> 13) & 0x3FF))[nan]
    out = h.astype(np.uint16).view(np.float16).astype(np.float32)
    out.view(np.uint32)[nan] = (((h & 0x8000) << 16) | 0x7F800000 | ((h & 0x3FF) << 13))[nan].astype(np.uint32)
    return out


# ---- comparison ------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mismatch(got, want, op, cnt=None):
    """Empty string when `got` equals `want` under the special-value rule, else a description of the first differences.
    Non-NaN elements: the same bits (sign of zero included).  NaN positions: the same.  NaN payloads: only where the
    output is a move -- whatever Max / Min select and the default_attr fills of empty segments (cnt == 0)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    gb, wb = bits(got), bits(want)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & (gb != wb))
    if op in ("MaxAggregator", "MinAggregator", "lookup"):
        bad |= gb != wb
    elif cnt is not None:
        bad[np.asarray(cnt) == 0] |= (gb != wb)[np.asarray(cnt) == 0]
    if not bad.any():
        return ""
    idx = np.argwhere(bad)
    out = ["%d of %d elements differ" % (len(idx), bad.size)]
    for i in idx[:8]:
        i = tuple(i)
        out.append("  at %s: got %08x (%r) want %08x (%r)" % (i, gb[i], float(got[i]), wb[i], float(want[i])))
    return "\n".join(out)


def nan_payloads_equal(got, want):
    """True when every NaN of `want` has the same bits in `got` (reported, not asserted, for arithmetic results)."""
    wn = np.isnan(np.asarray(want, np.float32))
    return bool(np.array_equal(bits(got)[wn], bits(want)[wn]))
