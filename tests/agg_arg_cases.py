"""The cases of the recording forward's tests (glx_aggregate_arg: tests/test_agg_arg_cpu.py, tests/test_gpu_agg_arg.py):
a restatement of the kernel's launch rule, the enumerated shapes that reach every launch path, the tables and requests
they run on, and a vectorised statement of the contract that shares no code with agg_backward_ref.fold_arg.
numpy only; fixed seeds; nothing here is drawn at test time."""
import functools

import numpy as np

MAX, MIN = 2, 3
FLT_MAX = np.float32(np.finfo(np.float32).max)
START = {MAX: np.float32(-37.0), MIN: FLT_MAX}  # the fold's start values (max_aggregator.cc:28, min_aggregator.cc:28)
WORKGROUP = 256
UNROLL = 4  # kArgU: rows in flight per lane

# ---- the launch rule of launch_arg_fwd ----------------------------------------------------------------------
def launch_rule(dim, pitch=None, table_aligned=True, out_aligned=True):
    """(VEC, G, tiles) of one call: vec4 iff dim and the row pitch are multiples of 4, the table is aligned to 4 elements
    and emb / arg to 16 bytes; G = the smallest power of two >= the lanes a row needs, at most 64; tiles = the column
    tiles one group walks.  Pins coverage only: no GPU assertion depends on it."""
    pitch = dim if pitch is None else pitch
    vec4 = dim % 4 == 0 and pitch % 4 == 0 and table_aligned and out_aligned
    lanes = dim // 4 if vec4 else dim
    G = 1
    while G < 64 and G < lanes:
        G *= 2
    return (4 if vec4 else 1), G, -(-lanes // G)


def segments_per_workgroup(G):
    return WORKGROUP // G


def segment_counts(G):
    """S at the workgroup edges: one segment, a partial workgroup, exactly one, one segment into the second, two and one"""
    P = segments_per_workgroup(G)
    return sorted({s for s in (1, P - 1, P, P + 1, 2 * P + 1) if s > 0})


DIMS = [1, 2, 3, 4, 5, 8, 12, 16, 32, 33, 64, 65, 100, 128, 129, 252, 256, 260, 512, 516]
MISALIGNED_DIMS = [d for d in DIMS if d % 4 == 0]  # run again with a mis-aligned pointer: the scalar path
# every (VEC, G, min(tiles, 3)) the rule can produce: one tile below 64 lanes, up to three and more at G = 64
ALL_PATHS = {(v, g, 1) for v in (1, 4) for g in (1, 2, 4, 8, 16, 32, 64)} | {(v, 64, t) for v in (1, 4) for t in (2, 3)}

FANOUTS = [1, 3, 4, 5, 25]
RAGGED_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1000]
UNROLL_DIMS = [4, 100, 260]  # G = 1, G = 32, two column tiles
DEFAULT_ATTR = 0.25
WINNING_DEFAULT = 5.0  # above every table entry: an unknown id wins its segment's columns
SMALL_V = 64

OWNED_ROWS = [4096 + 37, 8192 + 5]  # swizzled blocks of 4096 rows plus an unswizzled tail
OWNED_DIMS = [3, 12, 100, 256]
SWIZZLE_BLOCK = 4096


def reached_paths():
    """the (VEC, G, min(tiles, 3)) triples of the case lists: DIMS aligned, MISALIGNED_DIMS forced to the scalar path"""
    got = set()
    for d in DIMS:
        v, g, t = launch_rule(d)
        got.add((v, g, min(t, 3)))
    for d in MISALIGNED_DIMS:
        v, g, t = launch_rule(d, out_aligned=False)
        got.add((v, g, min(t, 3)))
    return got


# ---- tables -------------------------------------------------------------------------------------------------
def band_rows(V):
    """the rows whose entries lie in [-40, -36], on both sides of Max's start value"""
    return np.arange(3, V, 4)


@functools.lru_cache(maxsize=None)
def _table(V, dim, seed):
    rng = np.random.default_rng([seed, V, dim])
    X = rng.integers(-3, 4, (V, dim)).astype(np.float32)  # ties everywhere, exact in bfloat16 and float16
    band = band_rows(V)
    X[band] = rng.integers(-40, -35, (len(band), dim)).astype(np.float32)
    return X


class Case:
    """One request: `rows` are table rows (-1 and V: unknown ids), `seg` the segment_ids (None: the implied layout)."""

    def __init__(self, name, dim, S, V, rows, seg=None, default_attr=DEFAULT_ATTR, seed=0):
        self.name, self.dim, self.S, self.V, self.seed = name, dim, S, V, seed
        self.rows = np.ascontiguousarray(rows, np.int64)
        self.seg = None if seg is None else np.ascontiguousarray(seg, np.int32)
        self.default_attr = default_attr

    def table(self, op):
        """float32 [V, dim]; Min runs on the mirror image (the same positions win, as test_gpu_agg_backward._arg_case)"""
        X = _table(self.V, self.dim, self.seed)
        return X if op == MAX else -X

    def default(self, op):
        return self.default_attr if op == MAX else -self.default_attr

    def starts(self):
        """start[S + 1] of the segments (every case here is a valid request: no cursor stall)"""
        if self.seg is None:
            return np.arange(self.S + 1, dtype=np.int64) * (len(self.rows) // self.S)
        assert np.all(np.diff(self.seg) >= 0) and (len(self.seg) == 0 or (self.seg[0] >= 0 and self.seg[-1] < self.S))
        return np.searchsorted(self.seg, np.arange(self.S + 1), side="left").astype(np.int64)

    def __repr__(self):
        return self.name


def _request_rows(rng, V, seg_of, blocks=False):
    """rows of one request: drawn over [-1, V] (or, blocks=True, from every 4096-row block and the tail in turn); every
    fifth segment takes band rows only, so Max never leaves its start value there; -1 and V are always present."""
    n = len(seg_of)
    if blocks:
        nb = -(-V // SWIZZLE_BLOCK)
        lo = (np.arange(n) % nb) * SWIZZLE_BLOCK
        hi = np.minimum(lo + SWIZZLE_BLOCK, V)
        rows = lo + (rng.random(n) * (hi - lo)).astype(np.int64)
    else:
        rows = rng.integers(-1, V + 1, n)
    band = band_rows(V)
    in_band = seg_of % 5 == 2
    rows[in_band] = band[rng.integers(0, len(band), int(in_band.sum()))]
    if n >= 8:
        rows[1], rows[n - 2] = -1, V
    return rows.astype(np.int64)


def implied_case(dim, S, fanout, V=SMALL_V, default_attr=DEFAULT_ATTR, blocks=False, seed=1):
    rng = np.random.default_rng([seed, dim, S, fanout, V])
    seg_of = np.repeat(np.arange(S), fanout)
    name = "implied-d%d-S%d-f%d-V%d-s%d" % (dim, S, fanout, V, seed)
    return Case(name, dim, S, V, _request_rows(rng, V, seg_of, blocks), None, default_attr, seed)


def ragged_case(dim, lengths, V=SMALL_V, default_attr=DEFAULT_ATTR, blocks=False, seed=2, tag="ragged"):
    lengths = np.asarray(lengths, np.int64)
    S = len(lengths)
    rng = np.random.default_rng([seed, dim, S, int(lengths.sum()), V])
    seg_of = np.repeat(np.arange(S), lengths)
    name = "%s-d%d-S%d-n%d-V%d-s%d" % (tag, dim, S, len(seg_of), V, seed)
    return Case(name, dim, S, V, _request_rows(rng, V, seg_of, blocks), seg_of.astype(np.int32), default_attr, seed)


def edge_lengths(S, seed=3):
    """lengths 0..9 for S segments; the first and the last segment are empty once there are three"""
    lengths = np.random.default_rng([seed, S]).integers(0, 10, S)
    if S >= 3:
        lengths[0] = lengths[-1] = 0
        lengths[1] = 6  # never all empty
    else:
        lengths[-1] = 3
    return lengths


def long_lengths(seed=4):
    """RAGGED_LENGTHS shuffled, behind and in front of an empty segment"""
    mid = np.array(RAGGED_LENGTHS)
    np.random.default_rng(seed).shuffle(mid)
    return np.concatenate([[0], mid, [0]])


# ---- the case lists -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def launch_path_cases(dim, misaligned=False):
    """every S of this dim's G, implied (fan-out 5) and ragged; misaligned: the G of the forced scalar path"""
    _, G, _ = launch_rule(dim, out_aligned=not misaligned)
    cases = []
    for S in segment_counts(G):
        cases.append(implied_case(dim, S, 5))
        cases.append(ragged_case(dim, edge_lengths(S)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def unroll_cases(dim):
    """the ragged length list and the five implied fan-outs; the ragged request's default_attr wins columns"""
    _, G, _ = launch_rule(dim)
    S = segments_per_workgroup(G) + 1
    cases = [ragged_case(dim, long_lengths(), default_attr=WINNING_DEFAULT, tag="long")]
    cases += [implied_case(dim, S, f) for f in FANOUTS]
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def owned_case(V, dim):
    """ids from every 4096-row block, the tail, -1 and V; more than two workgroups of segments at every dim"""
    _, G, _ = launch_rule(dim)
    return implied_case(dim, max(2 * segments_per_workgroup(G) + 1, 131), 5, V=V, blocks=True, seed=5)


@functools.lru_cache(maxsize=None)
def chain_cases(dim):
    _, G, _ = launch_rule(dim)
    S = 2 * segments_per_workgroup(G) + 1
    return (implied_case(dim, S, 5, seed=6), ragged_case(dim, edge_lengths(S, seed=7), seed=6))


@functools.lru_cache(maxsize=None)
def stream_case():
    return implied_case(128, 2000, 25, V=1024, seed=8)


def all_cases():
    out = []
    for d in DIMS:
        out += launch_path_cases(d)
    for d in MISALIGNED_DIMS:
        out += launch_path_cases(d, True)
    for d in UNROLL_DIMS:
        out += unroll_cases(d)
        out += chain_cases(d) if d != 4 else ()
    for V in OWNED_ROWS:
        for d in OWNED_DIMS:
            out.append(owned_case(V, d))
    out.append(stream_case())
    seen, uniq = set(), []
    for c in out:
        if c.name not in seen:
            seen.add(c.name)
            uniq.append(c)
    return uniq


# ---- the contract, stated a second time ---------------------------------------------------------------------
def extreme_arg(op, X, rows, start, default_attr):
    """(emb, arg) by the rule, not by a fold: per segment and column ignore NaN and let m be the extreme of the rest; if
    m beats the start value, arg is the first position holding m and emb that element, else emb is the start value and
    arg -1; an empty segment gives default_attr and -1.  One padded [S, longest, D] block, no loop over positions."""
    X = np.asarray(X, np.float32)
    rows = np.asarray(rows, np.int64)
    start = np.asarray(start, np.int64)
    S, D = len(start) - 1, X.shape[1]
    length = start[1:] - start[:-1]
    L = max(int(length.max()) if S else 0, 1)
    slot = np.arange(L)[None, :]
    live = slot < length[:, None]                                  # [S, L]
    pos = np.where(live, start[:-1, None] + slot, 0)
    r = rows[pos] if len(rows) else np.zeros_like(pos)
    known = (r >= 0) & (r < X.shape[0])
    vals = np.where(known[:, :, None], X[np.where(known, r, 0)], np.float32(default_attr)).astype(np.float32)
    key = vals if op == MAX else -vals                             # Min is Max of the negation (exact)
    usable = live[:, :, None] & ~np.isnan(key)
    key = np.where(usable, key, -np.inf)
    m = key.max(axis=1)                                            # [S, D]
    init = START[op] if op == MAX else -START[op]
    beats = usable.any(axis=1) & (m > init)
    first = np.argmax(usable & (key == m[:, None, :]), axis=1)     # +0.0 == -0.0: the first of a tie
    picked = np.take_along_axis(vals, first[:, None, :], axis=1)[:, 0, :]
    emb = np.where(beats, picked, START[op]).astype(np.float32)
    arg = np.where(beats, start[:-1, None] + first, -1).astype(np.int32)
    empty = length == 0
    emb[empty] = np.float32(default_attr)
    arg[empty] = -1
    return emb, arg
