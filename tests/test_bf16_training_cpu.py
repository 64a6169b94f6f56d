"""The bfloat16 training path without a GPU: the six _ex entry points exist in the header, in glx.EXPORTS and in
libglx.so under ABI version 5, each refuses every dtype but float32 / bfloat16 before it touches a device, and the
rounding the row-gradient kernels use -- glx_features_convert_host is the same code on the host -- gives the codes the
contract names for the planted values of the GPU rounding test."""
import ctypes
import os
import re

import numpy as np
import pytest

import bf16_training_ref as b16
import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 3
EX = ["glx_aggregate_backward_ex", "glx_aggregate_weighted_ex", "glx_aggregate_weighted_backward_x_ex",
      "glx_aggregate_weighted_backward_w_ex", "glx_pair_dot_ex", "glx_pair_dot_backward_ex"]
BAD_DTYPES = [glx.FEATURE_DTYPES["float16"], glx.FP8_FEATURE_DTYPES["float8_e4m3fn"],
              glx.FP8_FEATURE_DTYPES["float8_e5m2"], 7]


def _header():
    return open(os.path.join(ROOT, "include", "glx.h")).read()


@pytest.mark.parametrize("name", EX)
def test_entry_point_is_declared_exported_and_listed(name):
    assert "GLX_API int {}(".format(name) in _header()
    assert name in glx.EXPORTS
    assert hasattr(ctypes.CDLL(glx.LIB_PATH), name)


def test_abi_version_is_still_5():
    assert re.search(r"^#define GLX_ABI_VERSION 5$", _header(), flags=re.M)
    assert glx.lib().glx_abi_version() == 5


def _call(name, dt):
    """a well-formed one-row request with host pointers, but for the dtype id"""
    L = glx.lib()
    rows = np.zeros(1, np.int64)
    f4 = np.zeros(4, np.float32)
    tab = np.zeros(4, np.float32)  # 16 bytes: room for any element type
    w = np.ones(1, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    H = glx.PTR_HOST
    if name == "glx_aggregate_backward_ex":
        return L.glx_aggregate_backward_ex(0, glx.SUM, p(rows), None, None, 1, 1, 1, 4, p(f4), p(tab), dt, H, None)
    if name == "glx_aggregate_weighted_ex":
        return L.glx_aggregate_weighted_ex(0, glx.SUM, p(tab), dt, 1, 4, p(rows), p(w), 1, None, 1, 1, 0.0, p(f4), H, None)
    if name == "glx_aggregate_weighted_backward_x_ex":
        return L.glx_aggregate_weighted_backward_x_ex(0, glx.SUM, p(rows), p(w), 1, None, 1, 1, 1, 4, p(f4), p(tab), dt,
                                                      H, None)
    if name == "glx_aggregate_weighted_backward_w_ex":
        return L.glx_aggregate_weighted_backward_w_ex(0, glx.SUM, p(tab), dt, 1, 4, p(rows), 1, None, 1, 1, 0.0, p(f4),
                                                      p(w), H, None)
    if name == "glx_pair_dot_ex":
        return L.glx_pair_dot_ex(0, p(tab), 1, p(tab), 1, dt, 4, 1, p(rows), p(rows), 1, 1, 0.0, p(w), H, None)
    return L.glx_pair_dot_backward_ex(0, 0, p(rows), p(rows), 1, 1, p(w), 1, p(tab), 1, 4, 1, 0.0, p(f4), dt, H, None)


@pytest.mark.parametrize("dt", BAD_DTYPES)
@pytest.mark.parametrize("name", EX)
def test_other_dtypes_are_refused_before_any_device_use(name, dt):
    assert _call(name, dt) == INVALID_ARGUMENT
    msg = glx.lib().glx_last_error().decode()
    assert "bfloat16" in msg and str(dt) in msg, msg


def test_planted_values_round_to_the_contract_codes():
    sums = b16.rounding_sums()
    assert b16.to_bf16(sums).tolist() == [code for _, code in b16.ROUNDING_CASES]
    # the three-term case really needs the float32 sum: rounding after every add stays at 1.0
    acc = np.float32(0.0)
    for t in b16.ROUNDING_CASES[2][0]:
        acc = b16.upcast(b16.to_bf16(np.array([np.float32(acc + t)], np.float32)))[0]
    assert b16.to_bf16(np.array([acc], np.float32)).tolist() == [0x3F80]


def test_upcast_inverts_the_rounding_on_every_code():
    codes = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    back = b16.to_bf16(b16.upcast(codes))
    nan = np.isnan(b16.upcast(codes))
    assert np.array_equal(back[~nan], codes[~nan]) and (back[nan] == 0xFFFF).all()


def test_wrappers_refuse_other_dtypes_before_the_call():
    rows = np.zeros(1, np.int64)
    w = np.ones(1, np.float32)
    g = np.zeros((1, 4), np.float32)
    for bad in (np.zeros((1, 4), np.float16), np.zeros((1, 4), np.float64), np.zeros((1, 4), np.uint8)):
        with pytest.raises(ValueError):
            glx.aggregate_weighted(glx.SUM, bad, rows, w, 1)
        with pytest.raises(ValueError):
            glx.aggregate_weighted_backward_w(glx.SUM, bad, rows, 1, None, g)
        with pytest.raises(ValueError):
            glx.pair_dot(bad, rows, bad, rows)
        with pytest.raises(ValueError):
            glx.pair_dot_backward(0, rows, rows, w, bad, 1)
        with pytest.raises(ValueError):
            glx.aggregate_backward(glx.SUM, rows, None, g, 1, out=bad)
    with pytest.raises(ValueError):
        glx.pair_dot(np.zeros((1, 4), np.float32), rows, np.zeros((1, 4), np.uint16), rows)
    with pytest.raises(ValueError):
        glx.aggregate_backward(glx.SUM, rows, None, g, 1, out_dtype="float16")
