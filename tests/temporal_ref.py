"""numpy restatement of the temporal sampling contract (include/glx.h, "temporal neighbour sampling").

A graph is a dict: row_ptr[V + 1], col[E], eid[E], ts[E] (per CSR slot, ascending inside every row) and optionally
ids[V] (raw id of row r; absent: raw id v is row v).  Test infrastructure only.
"""
import numpy as np

RECENT, UNIFORM = 0, 1
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

_DRAWS = {}  # (seed, cc) -> {row stream: [draw 0, draw 1, ...]} of the oracle's draw64, as Python integers


def draws(orc, seed, cc, rr, k):
    """draw j < k of row stream rr under (seed, cc): oracle_bindings' draw64, memoised"""
    have = _DRAWS.setdefault((int(seed), int(cc)), {}).setdefault(int(rr), [])
    while len(have) < k:
        have.append(int(orc.draw64(int(seed), int(cc), int(rr) & 0xffffffff, len(have))))
    return have[:k]


def rows_of(g, src):
    """row index of every raw id, -1 for an unknown one"""
    src = np.asarray(src, np.int64)
    V = g["row_ptr"].shape[0] - 1
    ids = g.get("ids")
    if ids is None:
        return np.where((src >= 0) & (src < V), src, -1)
    order = np.argsort(ids, kind="stable")
    pos = np.searchsorted(ids[order], src)
    pos = np.minimum(pos, V - 1) if V else np.zeros_like(pos)
    hit = (ids[order][pos] == src) if V else np.zeros(src.shape, bool)
    return np.where(hit, order[pos], -1)


def prefix_lengths(g, src, cutoff, inclusive):
    """(start, c) per request row: c slots of the row lie before the cutoff (np.searchsorted per row)"""
    rows = rows_of(g, src)
    start = np.zeros(len(rows), np.int64)
    c = np.zeros(len(rows), np.int64)
    side = "right" if inclusive else "left"
    for i, r in enumerate(rows):
        if r < 0:
            continue
        a, b = int(g["row_ptr"][r]), int(g["row_ptr"][r + 1])
        start[i] = a
        c[i] = np.searchsorted(g["ts"][a:b], np.int64(cutoff[i]), side=side)
    return start, c


def sample_temporal(g, src, cutoff, k, strategy=RECENT, inclusive=False, seed=0, call_counter=0, default_neighbor_id=0,
                    default_timestamp=-1, rng_rows=None, live=None, orc=None):
    """-> (nbr[B, k], eid[B, k], ts[B, k] int64, cnt[B] int32).  live (optional, bool[B]): a False row is default-filled
    with cnt = 0 whatever its id (a hop's request row whose parent slot holds no edge)."""
    src = np.asarray(src, np.int64)
    cutoff = np.asarray(cutoff, np.int64)
    B = src.shape[0]
    start, c = prefix_lengths(g, src, cutoff, inclusive)
    if live is not None:
        c = np.where(np.asarray(live, bool), c, 0)
    j = np.arange(k, dtype=np.int64)[None, :]
    if strategy == RECENT:
        pick = np.where(j < c[:, None], c[:, None] - 1 - j, -1)
        cnt = np.minimum(c, k).astype(np.int32)
    else:
        pick = np.full((B, k), -1, np.int64)
        for i in np.flatnonzero(c > 0):
            rr = i if rng_rows is None else int(rng_rows[i])
            ci = int(c[i])
            pick[i] = [(u * ci) >> 64 for u in draws(orc, seed, call_counter, rr, k)]
        cnt = np.where(c > 0, k, 0).astype(np.int32)
    valid = pick >= 0
    slot = np.where(valid, start[:, None] + pick, 0)
    E = g["col"].shape[0]
    if E == 0:
        return (np.full((B, k), default_neighbor_id, np.int64), np.full((B, k), -1, np.int64),
                np.full((B, k), default_timestamp, np.int64), cnt)
    nbr = np.where(valid, g["col"][slot], default_neighbor_id).astype(np.int64)
    eid = np.where(valid, g["eid"][slot], -1).astype(np.int64)
    ts = np.where(valid, g["ts"][slot], default_timestamp).astype(np.int64)
    return nbr, eid, ts, cnt


def sample_temporal_hops(graphs, seeds, cutoff, fanouts, strategy=RECENT, inclusive=False, seed=0, call_counter=0,
                         default_neighbor_id=0, default_timestamp=-1, orc=None):
    """The hops rule: request row r of hop h >= 1 is slot r of hop h - 1 (id = its neighbour, cutoff = its edge
    timestamp), live only where that slot holds a sampled edge; stream (seed, call_counter + h)."""
    outs, src, cut, live = [], np.asarray(seeds, np.int64), np.asarray(cutoff, np.int64), None
    for h, (g, k) in enumerate(zip(graphs, fanouts)):
        nbr, eid, ts, cnt = sample_temporal(g, src, cut, k, strategy, inclusive, seed, call_counter + h,
                                            default_neighbor_id, default_timestamp, None, live, orc)
        outs.append((nbr, eid, ts, cnt))
        live = (np.arange(k)[None, :] < cnt[:, None]).reshape(-1)
        src, cut = nbr.reshape(-1), ts.reshape(-1)
    return outs


def prefix_graph(g, src, cutoff, inclusive):
    """The derived graph whose vertex i is request row i's prefix: what RandomSampler draws from for UNIFORM."""
    start, c = prefix_lengths(g, src, cutoff, inclusive)
    row_ptr = np.zeros(len(c) + 1, np.int64)
    np.cumsum(c, out=row_ptr[1:])
    take = np.concatenate([np.arange(s, s + n) for s, n in zip(start, c)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return dict(row_ptr=row_ptr, col=np.ascontiguousarray(g["col"][take]), eid=np.ascontiguousarray(g["eid"][take]))


def tie_run_timestamps(rng, n, lo=-1000):
    """n ascending timestamps, negative and positive, in runs of ties of length 1 .. 130 (a run straddles the probe
    positions of every search width, half of the runs short so that rows of a few slots hold several values);
    consecutive runs differ by at least 2, so t - 1 and t + 1 are no slot's value"""
    out = np.empty(n, np.int64)
    at, t = 0, lo
    while at < n:
        run = int(rng.integers(1, 5)) if rng.random() < 0.5 else int(rng.integers(1, 131))
        out[at:at + run] = t
        at += run
        t += int(rng.integers(2, 40))
    return out


def build_graph(degrees, seed=0, ids=None, num_dst=997):
    """One row per entry of `degrees`, every row timestamp-ascending with tie runs; edge ids are a permutation."""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, np.int64)
    row_ptr = np.zeros(len(degrees) + 1, np.int64)
    np.cumsum(degrees, out=row_ptr[1:])
    E = int(row_ptr[-1])
    ts = np.empty(E, np.int64)
    for r, d in enumerate(degrees):
        ts[row_ptr[r]:row_ptr[r + 1]] = tie_run_timestamps(rng, int(d), lo=-int(rng.integers(0, 3000)))
    g = dict(row_ptr=row_ptr, col=rng.integers(0, num_dst, E).astype(np.int64), eid=rng.permutation(E).astype(np.int64),
             ts=ts)
    if ids is not None:
        g["ids"] = np.asarray(ids, np.int64)
    return g
