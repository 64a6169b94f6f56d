"""The samplers' row directory restated in Python (csrc/glx_common.h: GlxRowDirEntry, GlxRowDirSlot,
glx_row_dir_form_rule, glx_row_span; csrc/glx_graph.hip: glx_idmap_build's capacity and glx_row_dir_fill_kernel)."""
import numpy as np

NONE, DIRECT, HASHED16 = 0, 1, 2
FORM_NAMES = {NONE: None, DIRECT: "direct", HASHED16: "hashed16"}
ABSENT = 0xFFFFFFFF          # GLX_ROW_DIR_ABSENT: `start` of a direct entry whose id is no row
EMPTY_KEY = -2 ** 63         # GLX_EMPTY_KEY: the key of a free hashed16 slot (never a legal id)
E_LIMIT = 2 ** 32 - 1        # graphs with this many edges or more keep no directory
ENTRY = np.dtype([("start", "<u4"), ("deg", "<u4")])
SLOT = np.dtype([("key", "<i8"), ("start", "<u4"), ("deg", "<u4")])
M64 = (1 << 64) - 1


def mix64(x):
    """glx_mix64 on the two's-complement bits of x."""
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def capacity(num_rows):
    """glx_idmap_build: the smallest power of two >= max(64, 2 * num_rows)."""
    cap = 64
    while cap < 2 * num_rows:
        cap <<= 1
    return cap


def home_slot(id_, cap):
    return mix64(id_) & (cap - 1)


DEFAULT_ON = True           # kRowDirDefaultOn: what an unset GLX_ROW_DIR means


def form(num_rows, num_edges, min_id, max_id, cap, env=None):
    """glx_row_dir_form_rule."""
    if num_rows <= 0 or cap == 0 or ((env[:1] == "0") if env is not None else not DEFAULT_ON):
        return NONE
    if num_edges >= E_LIMIT:
        return NONE
    if env != "hash" and min_id >= 0 and (max_id + 1) * ENTRY.itemsize <= cap * SLOT.itemsize:
        return DIRECT
    return HASHED16


def table_bytes(which, max_id, cap):
    return {NONE: 0, DIRECT: (max_id + 1) * ENTRY.itemsize, HASHED16: cap * SLOT.itemsize}[which]


def build_direct(ids, start, deg):
    t = np.empty(int(max(ids)) + 1, ENTRY)
    t["start"], t["deg"] = ABSENT, ABSENT  # the build fills the table with 0xff bytes
    for i, s, d in zip(ids, start, deg):
        t[int(i)] = (s, d)
    return t


def build_hashed16(ids, start, deg, cap):
    """Linear probing from home_slot, in the order given (the device inserts in any order: which colliding id gets
    which slot of a run may differ, what a lookup answers may not)."""
    t = np.zeros(cap, SLOT)
    t["key"] = EMPTY_KEY
    for i, s, d in zip(ids, start, deg):
        h = home_slot(int(i), cap)
        while t["key"][h] != EMPTY_KEY:
            assert t["key"][h] != i, "ids are distinct"
            h = (h + 1) & (cap - 1)
        t[h] = (i, s, d)
    return t


def lookup(table, which, id_):
    """glx_row_span on a directory -> (known, start, deg, slots probed)."""
    if which == DIRECT:
        if id_ < 0 or id_ >= table.shape[0] or table["start"][id_] == ABSENT:
            return False, 0, 0, 0 if (id_ < 0 or id_ >= table.shape[0]) else 1
        return True, int(table["start"][id_]), int(table["deg"][id_]), 1
    if id_ == EMPTY_KEY:
        return False, 0, 0, 0
    cap = table.shape[0]
    h, probes = home_slot(id_, cap), 0
    while True:
        probes += 1
        k = int(table["key"][h])
        if k == id_:
            return True, int(table["start"][h]), int(table["deg"][h]), probes
        if k == EMPTY_KEY:
            return False, 0, 0, probes
        h = (h + 1) & (cap - 1)


def colliding_ids(cap, slot, count, first=0):
    """`count` ids >= first whose home slot is `slot`."""
    out, i = [], first
    while len(out) < count:
        if home_slot(i, cap) == slot:
            out.append(i)
        i += 1
    return out
