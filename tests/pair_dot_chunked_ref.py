"""The CHUNKED order of glx_pair_dot_backward_chunked restated in numpy from existing
pieces: pair_dot_ref's term of every pair, in ascending pair per own row, fed to agg_chunked_ref.chunked_sum -- a row's
run of pairs is its list, so chunks count PAIRS, wherever an entry's `repeat` pairs begin and end."""
import numpy as np

import agg_chunked_ref as cref
import pair_dot_ref as pref


def backward(side, ia, ib, g, x_other, num_rows_self, repeat=1, default_attr=0.0):
    ia, ib = np.asarray(ia, np.int64).reshape(-1), np.asarray(ib, np.int64).reshape(-1)
    n, D = len(ib), x_other.shape[1]
    g = np.asarray(g, np.float32).reshape(n, -1)
    own, other = (np.repeat(ia, repeat), ib) if side == 0 else (ib, np.repeat(ia, repeat))
    with np.errstate(all="ignore"):
        term = np.stack([(np.repeat(g[p], D // g.shape[1]) * pref._row(x_other, other[p], default_attr, np.float32))
                         .astype(np.float32) for p in range(n)])
    keep = (own >= 0) & (own < num_rows_self)
    return cref.chunked_sum(own[keep], term[keep], np.ones(term[keep].shape, bool), num_rows_self)
