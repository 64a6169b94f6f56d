"""Lines the C3 hop-2 sampling launch fetches for its id -> (start, deg) lookup under three layouts, predicted on the host
from the live request before the launch timings are read (host only, numpy; in the style of scripts/r17/ew_lines_model.py).

  python scripts/r21/row_dir_lines_model.py [IN.npz] [OUT.txt]
      IN.npz: scripts/r21/row_dir_probe.py --dump (default build/r21/hop2_lookup.npz); OUT: profiles/r21/row_dir_lines_model.txt

Layouts:
  (a) today's: keys[h] (8 B, every slot probed) -> vals[h] (4 B) -> row_ptr[row], row_ptr[row + 1] (8 B each);
  (b) direct: one 8-byte entry at index id;
  (c) hashed16: one 16-byte slot per probe, at the slots of (a).
The request-id line (src[i], 8 B a row) is in every stream.  The stream is in launch order, one access per (wave, request
row): a thread is one slot pair of a row (kpairs = 5 for k = 10), so the 5 threads of a row repeat its lookup inside one
wave (two waves where the row straddles them) and the loads of a wave to one line are one request.  L2 model: 8 private
LRUs of 4 MiB, 128-byte lines, fully associative, workgroup b (256 threads) on XCD b mod 8, as in round 17.  The record
gather of the same launch competes for the same L2s and is left out here: its modelled fetch is round 17's figure,
981.2 MB for the 20-byte records (profiles/r17/ew_lines_model.txt).

The hash table is rebuilt on the host from the store's row ids (ascending insertion, linear probing, glx_mix64, the
capacity of glx_idmap_build); the device inserts in no fixed order, so runs of colliding keys may be permuted -- the
probe lengths have the same distribution."""
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEFAULT_NPZ = os.path.join(ROOT, "build", "r21", "hop2_lookup.npz")
DEFAULT_TXT = os.path.join(ROOT, "profiles", "r21", "row_dir_lines_model.txt")
K2, XCDS, L2_LINES, LINE, BLOCK, WAVE = 10, 8, (4 << 20) // 128, 128, 256, 64
RECORD_MB_R17 = 981.2
EMPTY = np.int64(-2 ** 63)


def mix64(x):
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def build_table(uniq):
    """keys[cap] (EMPTY = free) and the slot of every row: linear probing, done in vector rounds."""
    cap = 64
    while cap < 2 * uniq.shape[0]:
        cap <<= 1
    mask = np.uint64(cap - 1)
    keys = np.full(cap, EMPTY, np.int64)
    slot_of = np.empty(uniq.shape[0], np.int64)
    todo = np.arange(uniq.shape[0])
    h = (mix64(uniq) & mask).astype(np.int64)
    while todo.shape[0]:
        free = keys[h] == EMPTY
        # of the rows that want the same free slot this round, the first (smallest index) takes it
        cand = np.nonzero(free)[0]
        _, first = np.unique(h[cand], return_index=True)
        win = cand[first]
        keys[h[win]] = uniq[todo[win]]
        slot_of[todo[win]] = h[win]
        keep = np.ones(todo.shape[0], bool)
        keep[win] = False
        h = ((h + 1) & (cap - 1))[keep]  # everyone else found its slot taken (before, or by this round's winner)
        todo = todo[keep]
    return keys, slot_of, cap


def lru_misses(lines, xcd):
    misses = 0
    for x in range(XCDS):
        lru = OrderedDict()
        for line in lines[xcd == x].tolist():
            if line in lru:
                lru.move_to_end(line)
            else:
                misses += 1
                lru[line] = None
                if len(lru) > L2_LINES:
                    lru.popitem(last=False)
    return misses


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_NPZ
    out = sys.argv[2] if len(sys.argv) > 2 else DEFAULT_TXT
    z = np.load(path)
    ids, uniq = z["ids"].astype(np.int64), z["uniq"].astype(np.int64)
    batch, kpairs = ids.shape[0], (K2 + 1) // 2
    keys, slot_of, cap = build_table(uniq)
    assert (keys != EMPTY).sum() == uniq.shape[0] and (keys[slot_of] == uniq).all()
    max_id = int(uniq[-1])
    # every request row: known?, its row, the slots its probe walks
    row = np.minimum(np.searchsorted(uniq, ids), uniq.shape[0] - 1)
    known = uniq[row] == ids
    home = (mix64(ids) & np.uint64(cap - 1)).astype(np.int64)
    last = np.where(known, slot_of[row], -1)
    unk = np.nonzero(~known)[0]
    h = home[unk].copy()
    while True:  # an unknown id walks to the first free slot
        busy = keys[h] != EMPTY
        if not busy.any():
            break
        h = np.where(busy, (h + 1) & (cap - 1), h)
    last[unk] = h
    probes = ((last - home) & (cap - 1)) + 1
    # (wave, row) pairs in launch order: the waves a row's kpairs threads fall in
    t0 = np.arange(batch, dtype=np.int64) * kpairs
    w_first, w_last = t0 // WAVE, (t0 + kpairs - 1) // WAVE
    two = w_last > w_first
    pair_row = np.concatenate([np.arange(batch), np.nonzero(two)[0]])
    pair_wave = np.concatenate([w_first, w_last[two]])
    o = np.lexsort((pair_row, pair_wave))
    pair_row, pair_wave = pair_row[o], pair_wave[o]
    pair_xcd = ((pair_wave // (BLOCK // WAVE)) % XCDS).astype(np.int8)
    TAG = 1 << 40  # one address space per table

    def stream(parts):
        """parts: list of (lines[n_pairs], valid[n_pairs]) in the order a thread issues them -> (lines, xcd)"""
        n = pair_row.shape[0]
        lines = np.stack([p[0] for p in parts], 1).reshape(-1)
        valid = np.stack([p[1] for p in parts], 1).reshape(-1)
        xcd = np.repeat(pair_xcd, len(parts))
        assert lines.shape[0] == n * len(parts)
        return lines[valid], xcd[valid]

    pr = pair_row
    yes = np.ones(pr.shape[0], bool)
    src_part = (0 * TAG + pr * 8 // LINE, yes)
    max_p = int(probes.max())
    key_parts = [(1 * TAG + ((home[pr] + j) & (cap - 1)) * 8 // LINE, probes[pr] > j) for j in range(max_p)]
    val_part = (2 * TAG + last[pr] * 4 // LINE, known[pr])
    rp0 = (3 * TAG + row[pr] * 8 // LINE, known[pr])
    rp1 = (3 * TAG + (row[pr] + 1) * 8 // LINE, known[pr])
    in_range = (ids >= 0) & (ids <= max_id)
    dir_part = (4 * TAG + ids[pr] * 8 // LINE, in_range[pr])
    slot_parts = [(5 * TAG + ((home[pr] + j) & (cap - 1)) * 16 // LINE, probes[pr] > j) for j in range(max_p)]
    layouts = {
        "(a) keys + vals + row_ptr": [src_part] + key_parts + [val_part, rp0, rp1],
        "(b) direct, 8-byte entries": [src_part, dir_part],
        "(c) hashed16, 16-byte slots": [src_part] + slot_parts,
    }
    tables = {"(a)": cap * 12 + (uniq.shape[0] + 1) * 8, "(b)": (max_id + 1) * 8, "(c)": cap * 16}
    lines_out = []

    def say(s):
        print(s, flush=True)
        lines_out.append(s)

    say("# C3 hop-2 sampling request: %d rows (%d unknown ids), %d distinct ids; store: %d rows, id map capacity %d "
        "(load %.2f), max id %d" % (batch, int((~known).sum()), np.unique(ids).shape[0], uniq.shape[0], cap,
                                    uniq.shape[0] / cap, max_id))
    say("# probes per lookup: mean %.3f, max %d; (wave, row) pairs: %d" % (probes.mean(), max_p, pr.shape[0]))
    src_only = lru_misses(*stream([src_part]))
    say("# request-id lines alone: %d fetches (%.1f MB)" % (src_only, src_only * LINE / 1e6))
    say("# layout  tables MB  dependent steps  distinct lookup lines  modelled L2 line fetches incl. request ids (8 x 4 MiB LRU)  lookup MB  vs (a)  share of the launch's modelled fetch (lookup + request ids + %.1f MB records)" % RECORD_MB_R17)
    base = None
    for name, parts in layouts.items():
        ln, xc = stream(parts)
        miss = lru_misses(ln, xc)
        distinct = np.unique(ln[ln >= TAG]).shape[0]
        mb = (miss - src_only) * LINE / 1e6
        if base is None:
            base = mb
        launch_a = base + src_only * LINE / 1e6 + RECORD_MB_R17
        say("%-30s %.1f  %s  %d  %d  %.1f  %+.1f %%  %+.1f %%" % (
            name, tables[name[:3]] / 1e6, {"(a)": "3 + probes", "(b)": "1", "(c)": "probes"}[name[:3]], distinct, miss, mb,
            100.0 * (mb - base) / base, 100.0 * (mb - base) / launch_a))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines_out) + "\n")


if __name__ == "__main__":
    main()
