"""CPU tests of the TGN memory: the restatement (tgn_memory_ref.py) on a stream written out by hand and against the
contract's own sentence, the four entry points at the drop-in boundary, and the input recipe of the GPU tolerance test."""
import ctypes

import numpy as np

import glx
import tgn_memory_ref as tref

NAMES = ["glx_tgn_store_update", "glx_tgn_message", "glx_tgn_message_backward", "glx_tgn_memory_write"]


def test_dict_store_on_a_stream_written_out_by_hand():
    """N = 5.  Call 1: (0 -> 1, t 10), (2 -> 2, t 10: a self loop), (0 -> 3, t 10: a tie in t with event 0 at node 0),
    (7 -> 4, t 12: src outside the table, node 4 seen only as dst).  Call 2: (1 -> 0, t 12), (-1 -> 1, t 12)."""
    s = tref.DictStore(5, 2)
    raw1 = np.arange(8, dtype=np.float32).reshape(4, 2)
    s.update([0, 2, 0, 7], [1, 2, 3, 4], [10, 10, 10, 12], raw1)
    pt, ps, po, pr = s.arrays()
    assert pt.tolist() == [10, 10, 10, 10, 12]
    assert ps.tolist() == [2, 0, 1, 2, 3]  # node 0: events 0 and 2 tie in t, the larger seq wins
    assert po.tolist() == [3, 0, 2, 0, 7]  # the self loop's other end point is itself; node 4 remembers the id outside
    assert np.array_equal(pr, raw1[[2, 0, 1, 2, 3]])
    raw2 = -np.ones((2, 2), np.float32)
    s.update([1, -1], [0, 1], [12, 12], raw2)
    pt, ps, po, pr = s.arrays()
    assert pt.tolist() == [12, 12, 10, 10, 12]
    assert ps.tolist() == [4, 5, 1, 2, 3]  # node 1: src of event 4 and dst of event 5, one timestamp: seq 5 wins
    assert po.tolist() == [1, -1, 2, 0, 7]
    assert np.array_equal(pr[:2], raw2) and np.array_equal(pr[2:], raw1[[1, 2, 3]])
    # nobody is stored for an id outside the table
    assert 7 not in s.msg_s and -1 not in s.msg_s


def test_dict_form_and_latest_event_per_node_agree_on_time_ordered_streams():
    rng = np.random.default_rng(5)
    for trial in range(6):
        N, R = int(rng.integers(1, 30)), int(rng.integers(0, 4))
        d, log = tref.DictStore(N, R), tref.EventLog(N, R)
        t0 = int(rng.integers(-50, 50))
        for call in range(5):
            B = int(rng.integers(0, 40))
            src, dst = rng.integers(-1, N + 1, B), rng.integers(-1, N + 1, B)
            t = t0 + np.sort(rng.integers(0, 4, B))  # ascending, with runs of ties; the next call starts at its end
            t0 = int(t[-1]) if B else t0
            raw = rng.standard_normal((B, R)).astype(np.float32)
            d.update(src, dst, t, raw)
            log.update(src, dst, t, raw)
            for a, b in zip(d.arrays(), log.arrays()):
                assert np.array_equal(a, b), (trial, call)


def test_a_stream_that_is_not_time_ordered_differs_from_the_dict_form():
    """the contract keeps the latest event; torch_geometric's stores let the later call overwrite the role's list"""
    d, log = tref.DictStore(2, 0), tref.EventLog(2, 0)
    for src, dst, t in (([0], [1], [9]), ([0], [1], [3])):
        d.update(src, dst, t, np.zeros((1, 0), np.float32))
        log.update(src, dst, t, np.zeros((1, 0), np.float32))
    assert log.arrays()[0].tolist() == [9, 9] and log.arrays()[1].tolist() == [0, 0]
    assert d.arrays()[0].tolist() == [3, 3] and d.arrays()[1].tolist() == [1, 1]


def test_message_of_the_restatement():
    memory = np.array([[1.0, -0.0], [np.nan, 2.0], [3.0, 4.0]], np.float32)
    last_update = np.array([5, 0, 7], np.int64)
    pend = (np.array([9, tref.INT64_MIN, 7], np.int64), np.array([0, -1, 3], np.int64), np.array([1, -1, 8], np.int64),
            np.array([[0.5], [0.0], [-2.0]], np.float32))
    w, b = np.array([0.5, 0.0], np.float32), np.array([0.0, 1.0], np.float32)
    h, has, t_out, dt, copied, x, enc = tref.message(memory, last_update, pend, w, b, [0, 1, 2, 3, -1, 0])
    assert has.tolist() == [1, 0, 1, 0, 0, 1] and t_out.tolist() == [9, 0, 7, 0, 0, 9] and dt.tolist() == [4, 0, 0, 0, 0, 4]
    assert np.array_equal(h.view(np.uint32)[:3], memory.view(np.uint32)) and not h[3:5].any()
    assert np.array_equal(copied[0].view(np.uint32), np.array([1.0, -0.0, np.nan, 2.0, 0.5], np.float32).view(np.uint32))
    assert copied[2].tolist() == [3.0, 4.0, 0.0, 0.0, -2.0]  # other end point 8 is outside the table
    assert not copied[1].any() and not enc[1].any()
    assert np.allclose(enc[0], np.cos([2.0, 1.0])) and np.allclose(enc[2], np.cos([0.0, 1.0]))
    gw, gb, _, _, _, _ = tref.time_gradients(np.ones((6, 2), np.float32), dt, has, w, b)
    assert np.allclose(gb, [-2 * np.sin(2.0) - np.sin(0.0), -3 * np.sin(1.0)])
    assert np.allclose(gw, [-8 * np.sin(2.0), -8 * np.sin(1.0)])


def test_entry_points_are_exported_and_listed():
    L = ctypes.CDLL(glx.LIB_PATH)
    for name in NAMES:
        assert name in glx.EXPORTS and hasattr(L, name), name
    assert glx.tgn_backward_depth(1) == 73 and glx.tgn_backward_depth(16384) == 73 and glx.tgn_backward_depth(16385) == 74


def _calls(p):
    L = glx.lib()
    return [L.glx_tgn_store_update(0, 4, 1, p, p, p, p, 1, 0, p, p, p, p, None),
            L.glx_tgn_message(0, 4, 2, 1, 1, p, p, p, p, p, p, p, p, p, 1, p, p, p, p, p, None),
            L.glx_tgn_message_backward(0, 1, 6, 5, 1, p, p, p, p, p, p, p, None),
            L.glx_tgn_memory_write(0, 4, 2, p, 1, p, p, p, p, None)]


def test_null_arguments_are_invalid():
    assert _calls(None) == [3, 3, 3, 3]
    assert b"NULL" in glx.lib().glx_last_error()
    L = glx.lib()
    assert L.glx_tgn_store_update(0, -1, 1, None, None, None, None, 0, 0, None, None, None, None, None) == 3
    assert L.glx_tgn_message_backward(0, 0, 4, 3, 2, None, None, None, None, None, None, None, None) == 3  # columns past the row


def test_unavailable_without_a_gpu():
    n = ctypes.c_int(-1)
    if glx.lib().glx_device_count(ctypes.byref(n)) == 0:
        return  # a GPU is visible: the GPU tests run the entry points
    buf = np.zeros(64, np.int64)  # never read: the device check comes first
    assert _calls(ctypes.c_void_p(buf.ctypes.data)) == [14, 14, 14, 14]


def test_tolerance_recipe_keeps_its_cap():
    """at least 90 % of the elements the GPU tolerance test checks have a bound of at most 2^-10 (Et at its floor of 1)"""
    for n, T in ((300, 100), (65, 8), (63, 7)):
        w, b, dt = tref.time_recipe(np.random.default_rng(n), n, T)
        assert np.all(np.abs(b) <= 1) and np.allclose(w[0], 1.0) and np.allclose(w[-1], 1e-3)
        assert np.mean((dt >= 0) & (dt <= 4096)) >= 0.95 and dt.max() < 2 ** 40
        x = tref.fma32(w[None, :], dt.astype(np.float32)[:, None], b[None, :])
        bound = tref.encoding_bound(x, 1)
        assert np.mean(bound <= 2.0 ** -10) >= 0.9
