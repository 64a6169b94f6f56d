"""A Python restatement of how glx_seg_scan_kernel (graph-learn_amd/csrc/glx_aggregate.hip) divides a request of
segment ids among workgroups, tiles, load instructions and lanes, of what each quad then does, and of the fix-up behind
it -- with every size a parameter, so that a test can shrink the tile until a handful of ids crosses every boundary.

The kernel's own sizes are read from its source (kernel_partition): a test that restates them would not notice a change.
"""
import os
import re

import numpy as np

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graph-learn_amd", "csrc", "glx_aggregate.hip")


class Partition:
    """quad ids per thread per load instruction, `wave` lanes, `threads` per workgroup, `loads` instructions per tile,
    `grid` workgroups, a run of more than `run_max` empty segments is left to the fix-up"""

    def __init__(self, quad, wave, threads, loads, grid, run_max):
        assert threads % wave == 0
        self.quad, self.wave, self.threads, self.loads, self.grid, self.run_max = quad, wave, threads, loads, grid, run_max
        self.span = threads * quad          # ids one load instruction of a workgroup covers
        self.tile = self.span * loads       # ids per tile
        self.stride = grid * self.tile      # from a workgroup's tile to its next


def kernel_partition(grid):
    """the sizes the kernel is built with, from its source text"""
    text = open(SOURCE).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, name
        return int(m.group(1))

    threads, loads, run_max = const("kSegScanThreads"), const("kSegScanLoads"), const("kSegRunMax")
    assert re.search(r"constexpr\s+int32_t\s+kSegScanSpan\s*=\s*kSegScanThreads\s*\*\s*4\s*;", text)
    assert re.search(r"constexpr\s+int32_t\s+kSegScanTile\s*=\s*kSegScanSpan\s*\*\s*kSegScanLoads\s*;", text)
    return Partition(4, 64, threads, loads, grid, run_max)


def scan(seg, num_segments, p):
    """-> dict(level, valid_len, writes, sources, counters_ok)
    level      what the scan raises (the host's floor -- 1 when the ids do not divide evenly -- is not in it)
    valid_len  n minus the largest n - i a wave raised
    writes     list of (segment, value, position of the quad's first id) in the order of the walk
    sources    {position of a quad's first id: "lane" | "memory" | "none"}: where the id before the quad came from
    """
    seg = [int(x) for x in seg]
    n = len(seg)
    f = n // num_segments if (num_segments > 0 and n > 0 and n % num_segments == 0) else 0
    writes, sources = [], {}
    level, raised = 0, 0  # raised = the largest n - bad_at
    counters_ok = True
    span_q, span_r = (p.span // f, p.span % f) if f else (0, 0)
    wrap = p.stride - (p.loads - 1) * p.span
    wrap_q, wrap_r = (wrap // f, wrap % f) if f else (0, 0)

    def advance(quo, rem, dq, dr):
        quo, rem = quo + dq, rem + dr
        if rem >= f:
            quo, rem = quo + 1, rem - f
        return quo, rem

    for b in range(p.grid):
        # per-thread state that lives across the tiles of a workgroup
        t_level = [0] * p.threads
        t_bad = [n] * p.threads
        t_cnt = [((b * p.tile + t * p.quad) // f, (b * p.tile + t * p.quad) % f) if f else (0, 0) for t in range(p.threads)]
        t0 = b * p.tile
        while t0 < n:
            for L in range(p.loads):
                # what every thread's load instruction returned: ids past the end read as 0
                loaded = [[seg[i] if i < n else 0 for i in range(t0 + L * p.span + t * p.quad, t0 + L * p.span + (t + 1) * p.quad)]
                          for t in range(p.threads)]
                for t in range(p.threads):
                    i0 = t0 + L * p.span + t * p.quad
                    m = max(0, min(p.quad, n - i0))
                    lane = t % p.wave
                    if lane == 0:
                        prev = seg[i0 - 1] if 0 < i0 < n else -1
                        src = "memory" if 0 < i0 < n else "none"
                    else:
                        prev, src = loaded[t - 1][p.quad - 1], "lane"
                    if m > 0:
                        sources[i0] = src
                    live = m > 0 and not (i0 > 0 and (prev < 0 or prev >= num_segments))
                    # the straight-line path: behind an id in range, every id its predecessor or the segment after it
                    # (differences as 32-bit unsigned), the last id in range, not the request's last quad
                    d = [(b - a) & 0xFFFFFFFF for a, b in zip([prev] + loaded[t][:-1], loaded[t])]
                    plain_quad = (0 <= prev < num_segments and 0 <= loaded[t][-1] < num_segments and all(x <= 1 for x in d)
                                  and i0 + p.quad < n)
                    if plain_quad:
                        q, r = t_cnt[t]
                        counters_ok &= (not f) or (q, r) == (i0 // f, i0 % f)
                        nonuniform = False
                        for j in range(p.quad):
                            if d[j]:
                                writes.append((loaded[t][j], i0 + j, i0))
                            if f:
                                nonuniform |= loaded[t][j] != q
                                r += 1
                                if r == f:
                                    q, r = q + 1, 0
                        if nonuniform:
                            t_level[t] = max(t_level[t], 1)
                    elif live:
                        q, r = t_cnt[t]
                        counters_ok &= (not f) or (q, r) == (i0 // f, i0 % f)
                        nonuniform = incomplete = False
                        bad = n
                        for j in range(m):
                            i, cur = i0 + j, loaded[t][j]
                            if cur < 0 or cur >= num_segments or cur < prev:
                                bad = i
                                break
                            if cur != prev:
                                if cur - prev > p.run_max:
                                    incomplete = True
                                else:
                                    writes.extend((s, i, i0) for s in range(prev + 1, cur + 1))
                            if f:
                                nonuniform |= cur != q
                                r += 1
                                if r == f:
                                    q, r = q + 1, 0
                            prev = cur
                        if bad == n and i0 + m == n:
                            if num_segments - prev > p.run_max:
                                incomplete = True
                            else:
                                writes.extend((s, n, i0) for s in range(prev + 1, num_segments + 1))
                        t_bad[t] = min(t_bad[t], bad)
                        t_level[t] = max(t_level[t], 2 if (incomplete or bad < n) else (1 if nonuniform else 0))
                    if f:
                        t_cnt[t] = advance(*t_cnt[t], *((span_q, span_r) if L + 1 < p.loads else (wrap_q, wrap_r)))
            t0 += p.stride
        for w in range(0, p.threads, p.wave):  # once per wave, behind the walk
            wl = max(t_level[w:w + p.wave])
            wb = min(t_bad[w:w + p.wave])
            if wl and wb < n:
                raised = max(raised, n - wb)
            level = max(level, wl)
    return dict(level=level, valid_len=n - raised, writes=writes, sources=sources, counters_ok=counters_ok)


def seg_start_after(seg, num_segments, p, canary=-7):
    """(level, valid_len, seg_start) as the reduce finds them: the scan's writes in walk order, then the fix-up"""
    r = scan(seg, num_segments, p)
    start = np.full(num_segments + 1, canary, np.int64)
    for s, value, _ in r["writes"]:
        start[s] = value
    if r["level"] == 2:
        start[:] = np.searchsorted(np.asarray(seg[:r["valid_len"]], np.int64), np.arange(num_segments + 1), side="left")
    return r["level"], r["valid_len"], start


def plain(seg, num_segments, run_max):
    """(level, valid_len, seg_start) with no partition at all: the first violation, a searchsorted, and the three levels"""
    seg = np.asarray(seg, np.int64)
    n = len(seg)
    prev = np.concatenate(([-1], seg[:-1]))
    bad = np.nonzero((seg < 0) | (seg >= num_segments) | (seg < prev))[0]
    valid_len = int(bad[0]) if len(bad) else n
    start = np.searchsorted(seg[:valid_len], np.arange(num_segments + 1), side="left")
    f = n // num_segments if (num_segments > 0 and n > 0 and n % num_segments == 0) else 0
    if valid_len < n:
        level = 2
    elif n > 0 and np.any(np.diff(np.concatenate(([-1], seg, [num_segments]))) > run_max):
        level = 2
    elif f and np.any(seg != np.arange(n) // f):
        level = 1
    else:
        level = 0
    return level, valid_len, start
