"""What the bfloat16 training-path tests share (test_bf16_training_cpu.py, test_gpu_bf16_training.py): the float32 ->
bfloat16 rounding through glx_features_convert_host -- the very function the row-gradient kernels run --, the exact
upcast, and the planted values of the one-rounding test with the codes the contract gives them."""
import numpy as np

import glx

BF16 = glx.FEATURE_DTYPES["bfloat16"]


def to_bf16(x):
    """the uint16 codes of a float32 array rounded by glx_features_convert_host (round to nearest even, NaN -> 0xFFFF)"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.uint16)
    flat = x.reshape(-1)
    assert glx.lib().glx_features_convert_host(flat.ctypes.data, flat.shape[0], BF16, out.ctypes.data) == 0
    return out


def upcast(codes):
    """the float32 array of bfloat16 codes: exact"""
    return (np.ascontiguousarray(codes).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# (the float32 terms one row receives, in ascending position; the bfloat16 code of their float32 sum)
ROUNDING_CASES = [
    ([np.float32(1.0 + 2.0 ** -8)], 0x3F80),                 # a tie: to even, down
    ([np.float32(1.0 + 3 * 2.0 ** -8)], 0x3F82),             # a tie: to even, up
    ([np.float32(1.0)] + [np.float32(2.0 ** -9)] * 3, 0x3F81),  # summed in float32; a bfloat16 accumulator stays at 0x3F80
    ([f32(0x7F7F7FFF)], 0x7F7F),                             # just below half-way to the binade past FLT_MAX's
    ([f32(0x7F7F8000)], 0x7F80),                             # half-way: to even = +inf
    ([np.float32(np.inf)], 0x7F80),
    ([np.float32(-np.inf)], 0xFF80),
    ([np.float32(np.nan)], 0xFFFF),
    ([np.float32(2.0 ** -133)], 0x0001),                     # a bfloat16 subnormal is kept
    ([np.float32(-0.0)], 0x0000),                            # +0.0 + -0.0 = +0.0
]


def rounding_sums():
    """the float32 sum of each case's terms, folded left to right from +0.0 as the kernels do"""
    sums = []
    with np.errstate(all="ignore"):
        for terms, _ in ROUNDING_CASES:
            acc = np.float32(0.0)
            for t in terms:
                acc = np.float32(acc + t)
            sums.append(acc)
    return np.array(sums, np.float32)
