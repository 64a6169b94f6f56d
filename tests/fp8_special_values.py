"""Special-value inputs for FP8 feature tables (tests/test_fp8_special_values_cpu.py,
tests/test_gpu_fp8_special_values.py): the float8 counterpart of tests/agg_special_values.py.

A float32 special-value table uploaded as float8 collapses into something else -- most of its values are no float8
numbers -- so the tables here are built from float8 CODES: every scenario value is a number of the type, a NaN entry is
one of the type's NaN codes (all of them in turn), and the table that reaches the kernel is the uint8 code matrix
itself, uploaded as a torch float8 tensor with no rounding in between.  What a kernel must compute is the result of the
float32 table of the upcast values, `upcast(codes, tdt)` -- torch's CPU conversion -- through the oracle.

Per type: NaN codes first / middle / last / alone, signed zeros, the smallest subnormal (a float32 normal after the
upcast), the neighbours of Max's -37 start, the largest number, products of the largest number that overflow float32
(15 factors of 448, 9 of 57344), products of the smallest subnormal that end subnormal (15 of 2^-9, 8 of 2^-16) and at
zero (17 and 10), and -- e5m2 only -- the infinities.  Test infrastructure only."""
import numpy as np

import agg_special_values as sv

NAMES = ["float8_e4m3fn", "float8_e5m2"]
NAN_CODES = {"float8_e4m3fn": [0x7F, 0xFF], "float8_e5m2": [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]}
NEG_ZERO = 0x80
HI = {"float8_e4m3fn": 448.0, "float8_e5m2": 57344.0}            # the largest number
SUB = {"float8_e4m3fn": 2.0 ** -9, "float8_e5m2": 2.0 ** -16}    # the smallest subnormal
ABOVE_37 = {"float8_e4m3fn": -36.0, "float8_e5m2": -32.0}        # the neighbours of Max's -37 start; -40 lies below in both
OVERFLOW_FACTORS = {"float8_e4m3fn": 15, "float8_e5m2": 9}       # HI ** n is beyond FLT_MAX from here on
SUBNORMAL_FACTORS = {"float8_e4m3fn": 15, "float8_e5m2": 8}      # SUB ** n is a float32 subnormal from here on ...
ZERO_FACTORS = {"float8_e4m3fn": 17, "float8_e5m2": 10}          # ... and rounds to zero from here on
NAN = float("nan")
INF = float("inf")


def name_of(tdt):
    return str(tdt).replace("torch.", "")


def torch_dtype(name):
    import torch
    return getattr(torch, name)


def upcast(codes, tdt):
    """The float32 table of a uint8 code table: torch's CPU conversion."""
    import torch
    codes = np.ascontiguousarray(codes, np.uint8)
    return torch.from_numpy(codes).view(tdt).float().numpy()


def nan_mask(codes, name):
    return np.isin(codes, NAN_CODES[name])


_DECODE = {}


def code_of(values, tdt):
    """uint8 codes of float values that are numbers of the type (anything else raises): looked up in the upcast of all
    256 codes by float32 bit pattern, so no rounding takes part.  NaNs are not accepted here (encode() places them)."""
    name = name_of(tdt)
    if name not in _DECODE:
        table = sv.bits(upcast(np.arange(256, dtype=np.uint8), tdt))
        _DECODE[name] = {int(b): c for c, b in enumerate(table) if c not in NAN_CODES[name]}
    out = np.empty(len(values), np.uint8)
    for i, b in enumerate(sv.bits(np.array(values, np.float32))):
        if int(b) not in _DECODE[name]:
            raise ValueError("%r is no %s number" % (float(np.array(values, np.float32)[i]), name))
        out[i] = _DECODE[name][int(b)]
    return out


class _NanCodes:
    """hands out the type's NaN codes in turn"""

    def __init__(self, name, start=0):
        self.codes, self.at = NAN_CODES[name], start

    def next(self):
        c = self.codes[self.at % len(self.codes)]
        self.at += 1
        return c


def encode(seq, tdt, nans):
    """one scenario as codes: numbers by code_of, each NaN entry the next NaN code of `nans`"""
    seq = np.array(seq, np.float32)
    isnan = np.isnan(seq)
    out = np.zeros(len(seq), np.uint8)
    out[~isnan] = code_of(seq[~isnan], tdt)
    for i in np.flatnonzero(isnan):
        out[i] = nans.next()
    return out


def scenarios(tdt):
    """Per-type column scenarios, each the sequence of one column's values down a segment in fold order.  Every number is
    one of the type; NAN entries stand for a NaN code (build_case rotates through all of them)."""
    name = name_of(tdt)
    hi, sub, above = HI[name], SUB[name], ABOVE_37[name]
    n_over, n_sub, n_zero = OVERFLOW_FACTORS[name], SUBNORMAL_FACTORS[name], ZERO_FACTORS[name]
    s = [
        # NaN codes: first, middle, last, alone, all; next to -0 and to the smallest subnormal
        [NAN, 3.0, -4.0], [1.0, NAN, 2.0], [5.0, -6.0, NAN], [NAN], [NAN, NAN, NAN], [NAN, NAN], [NAN, 7.0], [-8.0, NAN],
        [-0.0, NAN], [NAN, -0.0], [0.0, NAN, -0.0], [sub, NAN], [NAN, -sub], [NAN] * 7, [NAN, NAN, 1.5, NAN, NAN, NAN],
        # signed zeros
        [0.0, -0.0], [-0.0, 0.0], [-0.0], [0.0], [-0.0, -0.0], [-0.0, -0.0, -0.0], [-0.0, 5.0], [-1.0, -0.0], [3.0, -3.0],
        [-0.0, -40.0], [-40.0, -0.0], [0.0, -40.0, -0.0],
        # the smallest subnormal, both signs
        [sub], [-sub], [sub, sub, sub], [-sub, -sub, -sub], [sub, -sub], [-sub, sub], [sub, 0.5], [-sub, 0.5],
        [sub, -0.0], [-0.0, -sub], [2 * sub, -sub],
        # around Max's -37 start
        [-40.0], [above], [-40.0, -48.0], [-48.0, above], [above, -40.0], [-40.0, -40.0, -40.0], [-48.0, -40.0],
        [-48.0, hi], [hi, -40.0],
        # the largest number, both signs
        [hi], [-hi], [hi, hi], [-hi, -hi], [hi, -hi], [-hi, hi],
        # products that overflow float32 (and the last ones that do not), padded with 1.0 and 2.0
        [hi] * n_over, [-hi] * n_over, [1.0] + [hi] * n_over + [2.0], [-hi] * (n_over - 1) + [1.0, hi, 2.0],
        [hi] * (n_over - 1), [hi] * (n_over - 1) + [2.0, 2.0, 1.0], [2.0, -hi, 1.0] + [hi] * (n_over - 1),
        # products of the smallest subnormal: the last float32 normal, subnormal results, zero
        [sub] * (n_sub - 1), [sub] * n_sub, [-sub] * n_sub, [sub] * (n_sub + 1), [1.0] + [sub] * n_sub + [2.0],
        [sub] * n_zero, [-sub] * n_zero, [-sub] + [sub] * (n_zero - 1), [sub] * (n_zero - 1),
        # plain sequences
        [1.5, -2.0, 3.0], [0.5, 0.25, 0.125, 0.0625], [-7.0, 12.0, 14.0, -0.5, 2.0], [1.0] * 17, [-1.0] * 16,
    ]
    if name == "float8_e5m2":  # the inf set of agg_special_values.SCENARIOS
        s += [[INF, -INF], [-INF, INF], [INF, 0.0], [-0.0, -INF], [INF, -0.0], [INF], [-INF], [INF, 1.0], [-INF, -1.0],
              [INF, INF], [-INF, -INF, 2.0], [hi, INF], [-hi, -INF], [INF, NAN], [NAN, -INF], [-INF, NAN, INF]]
    return s


def pool(tdt):
    """the codes of every single value of scenarios(tdt), plus every NaN code"""
    name = name_of(tdt)
    vals = sorted({(float(v), bool(np.signbit(v))) for s in scenarios(tdt) for v in s if v == v})
    return np.concatenate([code_of([v for v, _ in vals], tdt), np.array(NAN_CODES[name], np.uint8)])


def build_case(tdt, D, seed, default_attr, blocks=2, random_segments=80, empty=True):
    """A uint8 code table [V, D], a request (ids, segment ids, number of segments) and its default_attr: the layout of
    agg_special_values.build_case.

    Scenario blocks: for each scenario length n, the scenarios of that length fill the columns of n fresh rows in turn
    (column j of a block takes scenario (j + offset) % count, several offsets) and one segment takes those n rows in
    order -- so every scenario is reduced in several lanes and vector slots.  Then segments of random rows drawn from
    the type's special codes (with some arbitrary codes among them), random lengths, unknown ids, -1, empty segments and
    a segment of unknown ids only.  Dense ids (row = id)."""
    name = name_of(tdt)
    rng = np.random.default_rng(seed)
    nans = _NanCodes(name, seed)
    by_len = {}
    for s in scenarios(tdt):
        by_len.setdefault(len(s), []).append(s)
    rows, seg_rows = [], []
    for n in sorted(by_len):
        group = by_len[n]
        cover = -(-len(group) // D)  # blocks until every scenario of this length has a column
        for off in [k * D for k in range(cover)] + [k * (D + 7) + 1 for k in range(1, blocks)]:
            block = np.stack([encode(group[(j + off) % len(group)], tdt, nans) for j in range(D)], axis=1)
            base = sum(r.shape[0] for r in rows)
            rows.append(block)
            seg_rows.append(list(range(base, base + n)))
    n_fixed = sum(r.shape[0] for r in rows)
    special = pool(tdt)
    R = max(64, 2 * D)
    rnd = special[rng.integers(0, special.shape[0], (R, D))]
    anycode = rng.random((R, D)) < 0.3
    rnd[anycode] = rng.integers(0, 256, int(anycode.sum())).astype(np.uint8)
    rows.append(rnd)
    codes = np.ascontiguousarray(np.concatenate(rows), np.uint8)
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
    return codes, ids, seg, Sg, np.float32(default_attr)


def circulant(D=256):
    """codes[r, c] = (r + c) % 256: every code sits in every column -- in every byte of a dword, every lane slot"""
    r = np.arange(256, dtype=np.int64)[:, None]
    c = np.arange(D, dtype=np.int64)[None, :]
    return ((r + c) % 256).astype(np.uint8)


def mismatch(got, want, op, cnt=None):
    """Empty string when `got` equals `want` under the FP8 rule, else a description of the first differences.

    Max, Min and the emb of aggregate_arg: every bit (the select never picks a NaN, so no output is a table NaN; an
    empty segment's default_attr is a move).  Sum, Mean, Prod: agg_special_values.mismatch unchanged -- non-NaN bits,
    NaN positions, payloads only where cnt == 0.  "lookup": the same rule with cnt[r] = 0 for the rows that are
    default_attr fills (every bit) and nonzero for table rows -- non-NaN elements every bit, NaN exactly where `want`
    (the upcast) has one, which is exactly at the NaN codes; the payload of an upcast NaN code is the hardware's."""
    if op == "lookup":
        assert cnt is not None
        return sv.mismatch(got, want, "SumAggregator", cnt)
    return sv.mismatch(got, want, op, cnt)
