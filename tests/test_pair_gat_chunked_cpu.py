"""glx_pair_dot_backward_chunked and glx_gat_attention_backward_chunked without a GPU: declared, exported, listed, and
refusing a bad dtype, side or head count before they touch a device; the ABI version stays 5."""
import ctypes
import os

import numpy as np
import pytest

import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 3
NEW = ["glx_pair_dot_backward_chunked", "glx_gat_attention_backward_chunked"]


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_exported_and_listed(name):
    header = open(os.path.join(ROOT, "include", "glx.h")).read()
    assert "GLX_API int {}(".format(name) in header
    assert name in glx.EXPORTS
    assert hasattr(ctypes.CDLL(glx.LIB_PATH), name)
    assert glx.lib().glx_abi_version() == 5


def _pair(side, dt):
    """a well-formed one-pair request with host pointers, but for `side` and the dtype id"""
    i, f = np.zeros(1, np.int64), np.zeros(4, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    return glx.lib().glx_pair_dot_backward_chunked(0, side, p(i), p(i), 1, 1, p(f), 1, p(f), 1, 4, 1, 0.0, p(f), dt,
                                                   glx.PTR_HOST, None)


def test_pair_dot_refuses_a_bad_dtype_or_side_before_any_device_use():
    dt = glx.FEATURE_DTYPES["float16"]
    assert _pair(0, dt) == INVALID_ARGUMENT
    msg = glx.lib().glx_last_error().decode()
    assert "glx_pair_dot_backward_chunked" in msg and "bfloat16" in msg and str(dt) in msg, msg
    assert _pair(2, glx.FEATURE_DTYPES["float32"]) == INVALID_ARGUMENT
    assert "side" in glx.lib().glx_last_error().decode()
    with pytest.raises(ValueError):
        glx.pair_dot_backward(0, np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros((1, 1), np.float32),
                              np.zeros((1, 4), np.float16), 1, chunked=True)


def test_gat_attention_refuses_bad_heads_before_any_device_use():
    i, f = np.zeros(1, np.int64), np.zeros(1, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = glx.lib().glx_gat_attention_backward_chunked(0, p(f), p(f), p(f), p(f), 1, p(i), 0, None, 1, 1, 0.2, 0.0, 0.0, 0,
                                                      0, p(f), p(f), p(f), glx.PTR_HOST, None)
    assert rc == INVALID_ARGUMENT and "heads" in glx.lib().glx_last_error().decode()
