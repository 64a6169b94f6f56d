"""Argument validation of half-precision feature tables that needs no GPU: the storage-type checks of
glx_features_create_ex / glx_features_view_ex run before the device is touched (like the shape checks of
glx_features_create), and the Python layers refuse unknown dtype names before they reach the library."""
import ctypes
import os
import sys

import numpy as np
import pytest

import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

INVALID_ARGUMENT = 3


def test_header_and_exports_list_the_entry_points():
    text = open(os.path.join(ROOT, "include", "glx.h")).read()
    for name in ("glx_features_create_ex", "glx_features_view_ex", "glx_features_dtype"):
        assert name in glx.EXPORTS and ("GLX_API int %s(" % name) in text
    for line in ("#define GLX_DTYPE_F32 0", "#define GLX_DTYPE_BF16 1", "#define GLX_DTYPE_F16 2"):
        assert line in text
    assert glx.FEATURE_DTYPES == {"float32": 0, "bfloat16": 1, "float16": 2}


@pytest.mark.parametrize("x_dtype,store_dtype", [(1, 0), (2, 0), (1, 2), (2, 1), (3, 0), (0, 3), (-1, 0), (0, 7)])
def test_create_ex_refuses_unknown_dtypes_and_pairs_without_a_gpu(x_dtype, store_dtype):
    L = glx.lib()
    x = np.zeros((4, 8), np.float32)
    h = ctypes.c_void_p(0)
    rc = L.glx_features_create_ex(0, 4, 8, x.ctypes.data, x_dtype, store_dtype, None, glx.PTR_HOST, None,
                                  ctypes.byref(h))
    assert rc == INVALID_ARGUMENT and not h.value
    assert b"dtype" in L.glx_last_error() or b"stored as" in L.glx_last_error()


@pytest.mark.parametrize("dtype", [-1, 3, 100])
def test_view_ex_refuses_unknown_dtypes_without_a_gpu(dtype):
    L = glx.lib()
    h = ctypes.c_void_p(0)
    assert L.glx_features_view_ex(0, 4, 8, ctypes.c_void_p(256), dtype, ctypes.byref(h)) == INVALID_ARGUMENT
    assert not h.value


def test_features_dtype_of_null_handle():
    L = glx.lib()
    d = ctypes.c_int(-1)
    assert L.glx_features_dtype(None, ctypes.byref(d)) == INVALID_ARGUMENT
    assert L.glx_features_dtype(None, None) == INVALID_ARGUMENT


def test_glx_features_refuses_bad_dtypes():
    with pytest.raises(ValueError):
        glx.Features(np.zeros((4, 8), np.float32), dtype="half")
    with pytest.raises(ValueError):
        glx.Features(np.zeros((4, 8), np.float32), dtype="int8")
    with pytest.raises(ValueError):  # only float32 input converts
        glx.Features(np.zeros((4, 8), np.float16), dtype="bfloat16")
    with pytest.raises(ValueError):  # not a feature element type
        glx.Features(np.zeros((4, 8), np.float64))


def test_settings_refuse_bad_feature_dtypes():
    from graphlearn import settings
    for bad in ("half", "bf16", "float64", 1, None):
        with pytest.raises(ValueError):
            settings.set_feature_dtype(bad)
    assert settings._MIRROR["feature_dtype"] == "float32"  # pylint: disable=protected-access
    assert "set_feature_dtype" in settings.__all__
