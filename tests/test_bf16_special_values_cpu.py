"""The planted cases of bf16_special_values.py without a GPU.  Every code written in ROUNDING_CASES is confirmed three
ways, for the bare terms and for every kernel's planted request: the numpy restatement of that kernel gives the case's
float32 sum, glx_features_convert_host (the row-gradient kernels' own rounding, on the host) gives the code, and so does
torch's float32 -> bfloat16 conversion of a contiguous CPU tensor, which shares no code with glx.  The exact upcast of
the sixteen special codes is checked against torch's bfloat16 -> float32."""
import numpy as np
import pytest
import torch

import agg_backward_ref as ref
import agg_weighted_ref as wref
import bf16_special_values as sv
import bf16_training_ref as b16
import pair_dot_ref as pref


def _torch_codes(x):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _confirm(got, case):
    """the restatement's float32 gradient `got` is the case's sums, and both conversions of it are its codes"""
    assert wref.same_bits(got, case["sums"])
    assert np.array_equal(b16.to_bf16(got), case["codes"])
    assert np.array_equal(_torch_codes(got), case["codes"])
    assert not case["codes"][-1].any()  # the row nobody refers to


def test_the_bare_terms_give_the_codes_in_the_table():
    sums = sv.rounding_sums()
    # the first ten are the cases of bf16_training_ref
    assert np.array_equal(sums.view(np.uint32)[:10], b16.rounding_sums().view(np.uint32))
    assert b16.to_bf16(sums).tolist() == sv.rounding_codes().tolist()
    assert _torch_codes(sums).tolist() == sv.rounding_codes().tolist()
    bits = sums.view(np.uint32)
    assert bits[10] == 0x00008000 and bits[11] == 0x00008001  # 2^-134 and the float32 above it
    assert bits[13] == 0x7F7F8000 and all(np.isfinite(t) for t in sv.ROUNDING_CASES[13][0])
    assert bits[14] == 0x00000000  # +0.0 + -0.0: the restatement gives +0.0
    w, v = sv.power_of_two_factor(np.float32(-0.0))
    assert w < 0 and v == 0 and not np.signbit(v)  # -0.0 is planted as a negative weight times +0.0


def test_the_accumulation_case_needs_the_float32_sum():
    terms, code = sv.ROUNDING_CASES[sv.ACCUMULATION_CASE]
    assert code == 0x3F81 and sv.per_add_rounding_code(terms, b16.to_bf16) == 0x3F80


def test_split_terms_are_bfloat16_values_and_sum_exactly():
    for terms, _ in sv.ROUNDING_CASES:
        for t in terms:
            pieces = sv.split_bf16_terms(t)
            assert wref.same_bits(sv.fold(pieces), sv.fold([t]))
            for p in pieces:
                g, v = sv.power_of_two_factor(p, need_bf16=True)
                assert np.frexp(abs(np.float64(g)))[0] == 0.5  # a power of two
                if not np.isnan(v):
                    assert b16.upcast(b16.to_bf16(np.array([v], np.float32)))[0].tobytes() == np.float32(v).tobytes()
            assert wref.same_bits(sv.fold(sv.split_below(t)), sv.fold([t]))
            assert all(not np.isfinite(p) or abs(p) * 4 <= np.finfo(np.float32).max for p in sv.split_below(t))


@pytest.mark.parametrize("dim,heads", sv.ROUNDING_SHAPES)
@pytest.mark.parametrize("op", ["sum", "mean"])
def test_weighted_backward_x_cases(op, dim, heads):
    case = sv.weighted_backward_x_rounding({"sum": ref.SUM, "mean": ref.MEAN}[op], dim, heads)
    w = case["w"][:, 0]
    used = w[case["rows"] >= 0]
    assert set(np.abs(used).tolist()) == {0.5, 2.0} and (used == 2.0).any() and (used == -0.5).any()
    if op == "mean":
        assert set(case["cnt"].tolist()) == {2, 4}
    got = wref.backward_x(wref.MEAN if op == "mean" else wref.SUM, case["rows"], case["w"], case["cnt"],
                          case["grad_out"], case["num_rows"])
    _confirm(got, case)


@pytest.mark.parametrize("dim,heads", sv.ROUNDING_SHAPES)
@pytest.mark.parametrize("repeat", [1, 3])
@pytest.mark.parametrize("side", [0, 1])
def test_pair_dot_backward_cases(side, repeat, dim, heads):
    case = sv.pair_dot_backward_rounding(side, repeat, dim, heads)
    assert len(case["ib"]) == len(case["ia"]) * repeat and case["x_other"].dtype == np.uint16
    assert case["x_other"].shape[0] <= 45
    got = pref.backward(side, case["ia"], case["ib"], case["g"], b16.upcast(case["x_other"]), case["num_rows"], repeat)
    _confirm(got, case)


@pytest.mark.parametrize("dim", [6, 12])
@pytest.mark.parametrize("op", ["sum", "mean", "max", "min"])
def test_aggregate_backward_cases(op, dim):
    op = {"sum": ref.SUM, "mean": ref.MEAN, "max": ref.MAX, "min": ref.MIN}[op]
    case = sv.aggregate_backward_rounding(op, dim)
    got = ref.backward(op, case["rows"], case["cnt"], case["grad_out"], case["num_rows"], case["arg"])
    _confirm(got, case)
    if op in (ref.MAX, ref.MIN):
        assert not case["codes"][:, 1::2].any() and case["codes"][:, 0::2].any()
    if op == ref.MEAN:
        assert set(case["cnt"].tolist()) == {4}


def test_upcast_of_the_special_codes_is_torchs():
    codes = np.array(sv.SPECIAL_CODES, np.uint16)
    want = torch.from_numpy(codes.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(b16.upcast(codes).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(b16.upcast(codes).view(np.uint32), codes.astype(np.uint32) << 16)
    assert len(set(sv.SPECIAL_CODES)) == 16 and len(sv.SPECIAL_FACTORS) == 16


@pytest.mark.parametrize("dim,heads", sv.SPECIAL_SHAPES)
def test_special_tables_plant_one_code_per_row(dim, heads):
    for col in sv.planted_columns(dim):
        codes, twin = sv.special_table(dim, col, 0), sv.special_table(dim, col, 0, finite=True)
        differ = codes != twin
        assert differ[:sv.NUM_SPECIAL, col].all() and differ.sum() == sv.NUM_SPECIAL
        assert np.isfinite(b16.upcast(twin)).all()
        assert codes[:sv.NUM_SPECIAL, col].tolist() == sv.SPECIAL_CODES
    assert sv.planted_columns(260) == [0, 255, 257] and sv.planted_columns(6) == [0, 5]
