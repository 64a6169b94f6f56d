"""FP8 feature tables (GLX_DTYPE_F8E4M3 / GLX_DTYPE_F8E5M2), the part that needs no GPU: the names, the float32 ->
storage conversion through glx_features_convert_host -- the very functions the upload kernel runs -- against torch's CPU
.to() bit for bit, and the argument validation that runs before the device is touched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import glx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

INVALID_ARGUMENT = 3
FP8 = [("float8_e4m3fn", torch.float8_e4m3fn), ("float8_e5m2", torch.float8_e5m2)]
HALF = [("bfloat16", torch.bfloat16), ("float16", torch.float16)]


def test_header_and_names():
    text = open(os.path.join(ROOT, "include", "glx.h")).read()
    for line in ("#define GLX_DTYPE_F8E4M3 8", "#define GLX_DTYPE_F8E5M2 9"):
        assert line in text
    assert glx.FP8_FEATURE_DTYPES == {"float8_e4m3fn": 8, "float8_e5m2": 9}
    assert glx.FEATURE_DTYPES == {"float32": 0, "bfloat16": 1, "float16": 2}
    assert "glx_features_convert_host" in glx.EXPORTS
    assert "GLX_API int glx_features_convert_host(" in text


def fp8_adversarial(tdt):
    """float32 inputs at which a float32 -> `tdt` conversion can go wrong (tdt: one of the two torch FP8 types)."""
    codes = torch.arange(256, dtype=torch.uint8).view(tdt).float().numpy()  # every code's own value (NaN, inf included)
    pos = np.sort(codes[:128][np.isfinite(codes[:128])]).astype(np.float64)  # the finite codes of the positive half
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)  # exact: a few mantissa bits each
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    near = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    e4 = tdt == torch.float8_e4m3fn
    edge = [448.0, 464.0, 465.0, 480.0] if e4 else [57344.0, 61440.0, 61441.0, 65536.0]
    edge = np.array(edge, np.float32)
    edge = np.concatenate([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(np.inf))])
    tiny = np.float32(2.0 ** (-10 if e4 else -17))  # half the smallest subnormal: a tie, to even = zero
    tiny = np.array([tiny, np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1))], np.float32)
    f32 = np.finfo(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, f32.max, f32.min, f32.tiny, f32.smallest_subnormal, 1e-40, -1e-40],
                       np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000, 0x7FC12345,
                     0xFFC12345, 0xFF923456], np.uint32).view(np.float32)
    rnd = np.random.default_rng(29).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    parts = [codes, near, -near, edge, -edge, tiny, -tiny, special, nans, rnd]
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32, copy=False))


def convert_host(x, code, itemsize):
    out = np.empty(x.shape[0] * itemsize, np.uint8)
    assert glx.lib().glx_features_convert_host(x.ctypes.data, x.shape[0], code, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("name,tdt", FP8)
def test_convert_host_equals_torch_fp8(name, tdt):
    for src in FP8:  # both types' adversarial sets through this type's conversion
        x = fp8_adversarial(src[1])
        want = torch.from_numpy(x).contiguous().to(tdt).view(torch.uint8).numpy()
        got = convert_host(x, glx.FP8_FEATURE_DTYPES[name], 1)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, [(hex(int(x[i:i + 1].view(np.uint32)[0])), hex(got[i]), hex(want[i])) for i in bad[:8]])


@pytest.mark.parametrize("name,tdt", FP8)
def test_convert_host_probed_values(name, tdt):
    """The values the rule is stated with (include/glx.h): e4m3 overflows to NaN, e5m2 to inf."""
    if name == "float8_e4m3fn":
        x = [448.0, 464.0, 465.0, np.inf, np.nan, 0.0, -0.0, 2.0 ** -10, np.nextafter(np.float32(2.0 ** -10), np.float32(1)), 0.0]
        want = [0x7E, 0x7E, 0x7F, 0x7F, 0x7F, 0x00, 0x80, 0x00, 0x01, 0xFF]
    else:
        x = [57344.0, 61440.0, 65536.0, 1e30, np.nan, np.inf, -np.inf, 0.0]
        want = [0x7B, 0x7C, 0x7C, 0x7C, 0x7F, 0x7C, 0xFC, 0xFF]
    x = np.array(x, np.float32)
    x.view(np.uint32)[-1] = 0xFFC00000  # a negative NaN
    assert convert_host(x, glx.FP8_FEATURE_DTYPES[name], 1).tolist() == want


@pytest.mark.parametrize("name,tdt", HALF)
def test_convert_host_equals_torch_half(name, tdt):
    for src in FP8:
        x = fp8_adversarial(src[1])
        want = torch.from_numpy(x).contiguous().to(tdt).view(torch.int16).numpy().view(np.uint16)
        got = convert_host(x, glx.FEATURE_DTYPES[name], 2).view(np.uint16)
        assert np.array_equal(got, want), name


def test_convert_host_float32_copies_and_refuses_unknown_types():
    x = fp8_adversarial(torch.float8_e5m2)[:4096]
    assert np.array_equal(convert_host(x, 0, 4).view(np.uint32), x.view(np.uint32))
    L = glx.lib()
    out = np.zeros(16, np.uint8)
    for bad in (3, 7, 10, -1):
        assert L.glx_features_convert_host(x.ctypes.data, 4, bad, out.ctypes.data) == INVALID_ARGUMENT
        assert b"dtype" in L.glx_last_error()
    assert L.glx_features_convert_host(None, 4, 8, out.ctypes.data) == INVALID_ARGUMENT
    assert L.glx_features_convert_host(None, 0, 8, None) == 0
    assert not out.any()


@pytest.mark.parametrize("x_dtype,store_dtype", [(8, 0), (9, 0), (8, 9), (9, 8), (1, 8), (2, 9), (8, 1)])
def test_create_ex_refuses_fp8_pairs_without_a_gpu(x_dtype, store_dtype):
    L = glx.lib()
    x = np.zeros((4, 8), np.float32)
    h = ctypes.c_void_p(0)
    rc = L.glx_features_create_ex(0, 4, 8, x.ctypes.data, x_dtype, store_dtype, None, glx.PTR_HOST, None,
                                  ctypes.byref(h))
    assert rc == INVALID_ARGUMENT and not h.value
    assert b"dtype" in L.glx_last_error() or b"stored as" in L.glx_last_error()


@pytest.mark.parametrize("dtype", [6, 10])
def test_view_ex_refuses_the_codes_around_fp8_without_a_gpu(dtype):
    L = glx.lib()
    h = ctypes.c_void_p(0)
    assert L.glx_features_view_ex(0, 4, 8, ctypes.c_void_p(256), dtype, ctypes.byref(h)) == INVALID_ARGUMENT
    assert not h.value


def test_python_layers_refuse_bad_fp8_names():
    from graphlearn import settings
    for bad in ("float8", "fp8", "e4m3", "float8_e4m3fnuz"):
        with pytest.raises(ValueError):
            settings.set_feature_dtype(bad)
        with pytest.raises(ValueError):
            glx.Features(np.zeros((4, 8), np.float32), dtype=bad)
    with pytest.raises(ValueError):  # numpy has no FP8 type: a uint8 matrix is not a feature matrix
        glx.Features(np.zeros((4, 8), np.uint8))
    with pytest.raises(ValueError):  # only float32 input converts
        glx.Features(torch.zeros((4, 8)).to(torch.float8_e4m3fn), dtype="bfloat16")
    with pytest.raises(ValueError):
        glx.Features(torch.zeros((4, 8)).to(torch.float8_e4m3fn), dtype="float8_e5m2")
    assert settings._MIRROR["feature_dtype"] == "float32"  # pylint: disable=protected-access
