"""CPU tests of glx_unique's argument checks: every one of them answers before any device use, so they hold with
and without a GPU; without one a well-formed call answers UNAVAILABLE like every other entry point."""
import ctypes

import numpy as np
import pytest

import glx

INVALID_ARGUMENT, UNAVAILABLE = 3, 14


def _call(parts, lens, num_parts=None, nodes=True, part_end=True, kind=glx.PTR_HOST):
    """parts: numpy arrays, raw addresses (int) or None per entry -- or None for a NULL `parts` argument."""
    L = glx.lib()
    P = len(lens) if num_parts is None else num_parts
    keep = []
    pp = None
    if parts is not None:
        addr = []
        for p in parts:
            if isinstance(p, np.ndarray):
                keep.append(p)
                addr.append(p.ctypes.data)
            else:
                addr.append(p)
        pp = (ctypes.c_void_p * max(len(addr), 1))(*addr)
    pl = (ctypes.c_int64 * max(len(lens), 1))(*lens) if lens is not None else None
    n = min(sum(max(int(k), 0) for k in lens), 1 << 10) if lens else 0
    out_nodes = np.empty(max(n, 1), np.int64)
    out_end = np.empty(max(P, 1), np.int64)
    return L.glx_unique(0, pp, pl, P, ctypes.c_void_p(out_nodes.ctypes.data) if nodes else None, None,
                        ctypes.c_void_p(out_end.ctypes.data) if part_end else None, kind, None)


def test_null_parts_is_invalid():
    a = np.arange(4, dtype=np.int64)
    assert _call(None, [4]) == INVALID_ARGUMENT
    assert b"NULL" in glx.lib().glx_last_error()
    assert _call([a], None, num_parts=1) == INVALID_ARGUMENT
    assert _call([a], [4], part_end=False) == INVALID_ARGUMENT
    assert _call([a], [4], nodes=False) == INVALID_ARGUMENT
    assert _call([None], [4]) == INVALID_ARGUMENT  # a NULL part that claims ids
    assert b"NULL" in glx.lib().glx_last_error()


@pytest.mark.parametrize("num_parts", [0, 17, -1])
def test_num_parts_outside_1_to_16_is_invalid(num_parts):
    a = np.arange(4, dtype=np.int64)
    assert _call([a] * 17, [4] * 17, num_parts=num_parts) == INVALID_ARGUMENT
    assert b"num_parts" in glx.lib().glx_last_error()


def test_negative_length_is_invalid():
    a = np.arange(4, dtype=np.int64)
    assert _call([a, a], [4, -1]) == INVALID_ARGUMENT
    assert b"negative" in glx.lib().glx_last_error()


@pytest.mark.parametrize("lens", [[1 << 31], [(1 << 31) - 1, 1], [1 << 30, 1 << 30], [1 << 62, 1 << 62, 1 << 62]])
def test_total_above_int32_max_is_invalid_and_names_the_limit(lens):
    """The pointers are bogus addresses: the size check must come before anything reads them."""
    assert _call([0x1000] * len(lens), lens) == INVALID_ARGUMENT
    assert b"2^31 - 1" in glx.lib().glx_last_error()
    assert _call([0x1000] * len(lens), lens, kind=glx.PTR_DEVICE) == INVALID_ARGUMENT


def test_bad_ptr_kind_is_invalid():
    a = np.arange(4, dtype=np.int64)
    assert _call([a], [4], kind=7) == INVALID_ARGUMENT


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_unavailable_without_a_device():
    a = np.array([3, 1, 3], np.int64)
    assert _call([a], [3]) == UNAVAILABLE
    assert _call([a, None], [3, 0]) == UNAVAILABLE
    assert _call([None], [0]) == UNAVAILABLE  # n == 0 still needs the device for a device-pointer caller's counts
    with pytest.raises(glx.GlxError) as e:
        glx.unique([a])
    assert e.value.code == UNAVAILABLE


def test_loader_takes_the_dedup_keyword():
    import inspect
    import graphlearn as gl
    from graphlearn import loader
    assert inspect.signature(gl.NeighborLoader.__init__).parameters["dedup"].default is False
    assert hasattr(loader, "CompactBatch")
