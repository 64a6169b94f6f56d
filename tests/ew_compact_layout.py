"""The compact EdgeWeight record table (csrc/glx_common.h GlxEwRec20), restated in Python integers.

20-byte records {prob, eid_self, eid_alias, nbr_self, nbr_alias}, three to a 64-byte sector: CSR slot g lives at byte
(g // 3) * 64 + (g % 3) * 20, the last 4 bytes of every sector are unused, and a table of E slots holds
ceil(E / 3) * 64 bytes.  record_bytes() is the selection rule of glx_graph_build_alias as a pure function."""
RECORD_BYTES = 20
SECTOR_BYTES = 64
PER_SECTOR = 3
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def offset(g):
    return (g // PER_SECTOR) * SECTOR_BYTES + (g % PER_SECTOR) * RECORD_BYTES


def table_bytes(E):
    return (E + PER_SECTOR - 1) // PER_SECTOR * SECTOR_BYTES


def fits_int32(lo, hi):
    return INT32_MIN <= lo and hi <= INT32_MAX


def record_bytes(eid_min, eid_max, nbr_min, nbr_max, E, env):
    """Bytes per record a weighted graph keeps: 20, 32 or 0.  env: GLX_EW_PACKED at the build, None when unset."""
    if E <= 0 or (env is not None and env[:1] == "0"):
        return 0
    if not fits_int32(eid_min, eid_max):
        return 0
    if env != "32" and fits_int32(nbr_min, nbr_max) and E <= 2 ** 31:
        return 20
    return 32
