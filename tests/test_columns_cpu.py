"""glx_columns without a GPU: the entry points validate their arguments before they touch the device, refuse loudly
when there is none, and the record layout glx.columns_layout documents is the one DESIGN.md section 2 describes."""
import ctypes
import itertools

import numpy as np
import pytest

import glx


def _no_gpu():
    n = ctypes.c_int(-1)
    return glx.lib().glx_device_count(ctypes.byref(n)) != 0


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_argument_validation_needs_no_gpu():
    L = glx.lib()
    h = ctypes.c_void_p(1)
    ids = np.arange(4, dtype=np.int64)
    ia = np.zeros((4, 2), np.int64)
    other = np.zeros(64, np.int64)  # stands in for a glx_features*: the call must refuse before it looks at it
    assert L.glx_columns_create(0, 4, 0, None, None, None, None, _p(ids), _p(other), 0, None, ctypes.byref(h)) == 3
    assert b"both ids and map_of" in L.glx_last_error() and not h.value
    assert L.glx_columns_create(0, 4, -1, None, None, None, None, None, None, 0, None, ctypes.byref(h)) == 3
    assert b"negative i_num" in L.glx_last_error()
    assert L.glx_columns_create(0, 4, 0, None, None, None, _p(ia), None, None, 0, None, ctypes.byref(h)) == 3
    assert b"int_attrs given with i_num == 0" in L.glx_last_error()
    assert L.glx_columns_create(0, 4, 2, None, None, None, None, None, None, 0, None, ctypes.byref(h)) == 3
    assert b"int_attrs is NULL" in L.glx_last_error()
    assert L.glx_columns_create(0, -1, 0, None, None, None, None, None, None, 0, None, ctypes.byref(h)) == 3
    assert L.glx_columns_create(0, 4, 0, None, None, None, None, None, None, 2, None, ctypes.byref(h)) == 3
    assert L.glx_columns_create(0, 4, 0, None, None, None, None, None, None, 0, None, None) == 3
    assert L.glx_columns_lookup(None, _p(ids), 4, 0.0, 0, 0, 0, None, None, None, None, 0, None) == 3
    assert b"NULL" in L.glx_last_error()
    assert L.glx_columns_info(None, None, None, None, None, None, None, None, None) == 3
    L.glx_columns_destroy(None)  # a no-op


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is visible")
def test_create_is_unavailable_without_gpu():
    h = ctypes.c_void_p()
    w = np.ones(3, np.float32)
    assert glx.lib().glx_columns_create(0, 3, 0, _p(w), None, None, None, None, None, 0, None, ctypes.byref(h)) == 14
    assert not h.value and b"no CPU fallback" in glx.lib().glx_last_error()
    with pytest.raises(glx.GlxError) as e:
        glx.Columns(3, weights=w)
    assert e.value.code == 14


def test_record_layout():
    lay = glx.columns_layout
    # the documented cases: 4 B of payload pads to 8; 16 B and longer pad to a multiple of 16
    assert lay(0) == {"int_attrs": None, "timestamps": None, "weights": None, "labels": None, "record_bytes": 0}
    assert lay(0, has_label=True) == {"int_attrs": None, "timestamps": None, "weights": None, "labels": 0, "record_bytes": 8}
    assert lay(0, True, True)["labels"] == 4 and lay(0, True, True)["record_bytes"] == 8
    assert lay(0, True, True, True) == {"int_attrs": None, "timestamps": 0, "weights": 8, "labels": 12, "record_bytes": 16}
    assert lay(1, has_label=True) == {"int_attrs": 0, "timestamps": None, "weights": None, "labels": 8, "record_bytes": 16}
    assert lay(1, True, True, True)["record_bytes"] == 32  # 24 B of fields
    assert lay(3, True, True, True) == {"int_attrs": 0, "timestamps": 24, "weights": 32, "labels": 36, "record_bytes": 48}
    for i_num in (0, 1, 3, 15, 16, 17, 40, 130):
        for w, l, t in itertools.product((False, True), repeat=3):
            got = lay(i_num, w, l, t)
            raw = 8 * i_num + 8 * t + 4 * w + 4 * l
            rb = got["record_bytes"]
            assert rb >= raw and rb % 8 == 0 and (rb < 16 or rb % 16 == 0) and rb - raw < 16
            assert (rb == 0) == (raw == 0)
            # 8-byte fields first, every field naturally aligned, no overlap
            spans = []
            if i_num:
                spans.append((got["int_attrs"], 8 * i_num, 8))
            for name, on, size in (("timestamps", t, 8), ("weights", w, 4), ("labels", l, 4)):
                assert (got[name] is not None) == on
                if on:
                    spans.append((got[name], size, size))
            at = 0
            for off, size, align in spans:
                assert off == at and off % align == 0
                at += size
            assert at == raw
