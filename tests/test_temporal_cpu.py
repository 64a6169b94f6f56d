"""CPU tests of temporal sampling: the numpy restatement (tests/temporal_ref.py) is pinned to the oracle's own
RandomSampler, and the three entry points exist, are listed and validate their arguments without a GPU."""
import ctypes

import numpy as np

import glx
import temporal_ref as tr
from oracle_bindings import Oracle


def _requests(g, rng, n):
    """n request rows over every row of g (unknown ids included), cutoffs at, just below and just above slot values"""
    V = g["row_ptr"].shape[0] - 1
    src = rng.integers(-1, V + 2, n).astype(np.int64)
    cut = g["ts"][rng.integers(0, g["ts"].shape[0], n)] + rng.integers(-1, 2, n)
    cut[:4] = [tr.I64_MIN, tr.I64_MAX, tr.I64_MIN, tr.I64_MAX]
    return src, cut.astype(np.int64)


def test_uniform_restatement_is_the_oracles_random_sampler_on_the_prefix_graph():
    """UNIFORM of the restatement == the oracle's RandomSampler on the derived graph whose vertex i is request row i's
    prefix: the restatement's draws, bounding and default fill are the oracle's, not its own."""
    orc = Oracle()
    rng = np.random.default_rng(3)
    g = tr.build_graph([0, 1, 2, 7, 9, 33, 65, 130, 700], seed=5)
    src, cut = _requests(g, rng, 150)
    for inclusive in (False, True):
        for k in (1, 2, 5, 9, 33):
            for default_id in (0, -7):
                nbr, eid, ts, cnt = tr.sample_temporal(g, src, cut, k, tr.UNIFORM, inclusive, seed=11, call_counter=4,
                                                       default_neighbor_id=default_id, default_timestamp=-(1 << 40),
                                                       orc=orc)
                derived = tr.prefix_graph(g, src, cut, inclusive)
                onbr, oeid = orc.sample(derived, "RandomSampler", np.arange(len(src), dtype=np.int64), k, seed=11,
                                        call_counter=4, padding_mode=1, default_neighbor_id=default_id)
                assert np.array_equal(nbr, onbr) and np.array_equal(eid, oeid), (inclusive, k)
                c = np.diff(derived["row_ptr"])
                assert np.array_equal(cnt, np.where(c > 0, k, 0))
                assert (ts[c == 0] == -(1 << 40)).all() and (ts[c > 0] > -(1 << 40)).all()


def test_uniform_restatement_follows_rng_rows():
    orc = Oracle()
    rng = np.random.default_rng(4)
    g = tr.build_graph([3, 40, 5], seed=6)
    src, cut = _requests(g, rng, 40)
    rows = rng.permutation(1000)[:40].astype(np.int64)
    nbr, eid, _, _ = tr.sample_temporal(g, src, cut, 6, tr.UNIFORM, True, seed=2, call_counter=9, rng_rows=rows, orc=orc)
    derived = tr.prefix_graph(g, src, cut, True)
    onbr, oeid = orc.sample(derived, "RandomSampler", np.arange(40, dtype=np.int64), 6, seed=2, call_counter=9,
                            rng_rows=rows)
    assert np.array_equal(nbr, onbr) and np.array_equal(eid, oeid)


def test_recent_restatement_on_a_row_written_out_by_hand():
    g = dict(row_ptr=np.array([0, 5], np.int64), col=np.array([10, 11, 12, 13, 14], np.int64),
             eid=np.array([4, 3, 2, 1, 0], np.int64), ts=np.array([-5, 0, 0, 7, 9], np.int64))
    src = np.zeros(6, np.int64)
    cut = np.array([0, 1, 7, 100, -5, tr.I64_MAX], np.int64)
    nbr, eid, ts, cnt = tr.sample_temporal(g, src, cut, 3, tr.RECENT, False, default_neighbor_id=-1, default_timestamp=-9)
    assert nbr.tolist() == [[10, -1, -1], [12, 11, 10], [12, 11, 10], [14, 13, 12], [-1, -1, -1], [14, 13, 12]]
    assert eid.tolist() == [[4, -1, -1], [2, 3, 4], [2, 3, 4], [0, 1, 2], [-1, -1, -1], [0, 1, 2]]
    assert ts.tolist() == [[-5, -9, -9], [0, 0, -5], [0, 0, -5], [9, 7, 0], [-9, -9, -9], [9, 7, 0]]
    assert cnt.tolist() == [1, 3, 3, 3, 0, 3]
    nbr, _, _, cnt = tr.sample_temporal(g, src, cut, 3, tr.RECENT, True, default_neighbor_id=-1)
    assert nbr.tolist() == [[12, 11, 10], [12, 11, 10], [13, 12, 11], [14, 13, 12], [10, -1, -1], [14, 13, 12]]
    assert cnt.tolist() == [3, 3, 3, 3, 1, 3]


def test_hops_restatement_never_samples_a_default_filled_slot():
    """default_neighbor_id = 0 while vertex 0 is real and has history: a default-filled parent slot stays dead"""
    g = tr.build_graph([6, 2, 9], seed=8, num_dst=3)
    seeds = np.array([0, 1, 2, 7], np.int64)
    cut = np.array([tr.I64_MAX, g["ts"][6], g["ts"][10], 5], np.int64)
    outs = tr.sample_temporal_hops([g, g], seeds, cut, [3, 2], tr.RECENT, default_neighbor_id=0)
    (n0, e0, t0, c0), (n1, e1, t1, c1) = outs
    assert c0.tolist()[1] == 0 and c0.tolist()[3] == 0  # strictly before the row's first slot / an unknown id
    dead = (e0 == -1).reshape(-1)
    assert dead.any() and (c1[dead] == 0).all() and (e1[dead] == -1).all() and (n1[dead] == 0).all()
    for r in np.flatnonzero(~dead):  # a neighbour's history before the interaction that reached it
        assert (t1[r, :c1[r]] < t0.reshape(-1)[r]).all()


def test_entry_points_validate_arguments_without_a_gpu():
    L = glx.lib()
    assert L.glx_sample_temporal(None, 0, None, None, None, 1, 1, 0, 0, -1, 0, 0, None, None, None, None, 0, None) == 3
    assert b"NULL" in L.glx_last_error()
    assert L.glx_sample_temporal_hops(None, 1, 0, None, None, 1, None, 0, 0, -1, 0, 0, None, None, None, None, 0,
                                      None) == 3
    assert b"NULL" in L.glx_last_error()
    graphs = (ctypes.c_void_p * 1)(None)
    fan = (ctypes.c_int32 * 1)(2)
    out = (ctypes.c_void_p * 1)(None)
    assert L.glx_sample_temporal_hops(graphs, 1, 0, None, None, 1, fan, 0, 0, -1, 0, 0, out, None, None, None, 0,
                                      None) == 3
    has = ctypes.c_int(-1)
    assert L.glx_graph_has_timestamps(None, ctypes.byref(has)) == 3


def test_symbols_are_exported_and_listed():
    L = ctypes.CDLL(glx.LIB_PATH)
    for name in ("glx_graph_has_timestamps", "glx_sample_temporal", "glx_sample_temporal_hops"):
        assert name in glx.EXPORTS
        assert hasattr(L, name)
    assert glx.TEMPORAL_STRATEGIES == {"recent": 0, "uniform": 1}
