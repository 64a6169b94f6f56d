"""CPU tests of the chunked order of dot-product attention (glx_dot_attention_chunked and
glx_dot_attention_backward_chunked): the library carries the entry points, they find the default entry points' argument
errors before any device use, glx.dot_attention(chunked=True) reaches them, and the numpy restatement
(dot_attention_chunked_ref.py) is the default restatement where no segment is long and another order where one is."""
import ctypes

import numpy as np
import pytest

import dot_attention_chunked_ref as cref
import dot_attention_ref as dref
import glx
from test_dot_attention_cpu import COMMON_ERRORS, INVALID, OWN_ERRORS, _p

SHAPES = [(6, 2), (12, 1), (16, 4), (256, 4), (260, 4), (520, 2)]  # test_gpu_dot_attention_chunked.py's


def test_the_library_exports_both_entry_points():
    assert "glx_dot_attention_chunked" in glx.EXPORTS and "glx_dot_attention_backward_chunked" in glx.EXPORTS
    L = ctypes.CDLL(glx.LIB_PATH)
    assert hasattr(L, "glx_dot_attention_chunked") and hasattr(L, "glx_dot_attention_backward_chunked")


def _call(entry, num_ids=4, num_segments=2, dim=4, heads=2, num_rows=3, scale=0.5, drop_p=0.0, ptr_kind=glx.PTR_HOST,
          **null):
    """test_dot_attention_cpu._call through the chunked entry points"""
    keep = {
        "q": np.ones((2, 4), np.float32), "k": np.ones((3, 4), np.float32), "v": np.ones((3, 4), np.float32),
        "rows": np.zeros(4, np.int64), "edge": np.ones((4, 4), np.float32), "cnt": np.array([2, 2], np.int32),
        "logit_out": np.zeros((4, 2), np.float32), "soft_out": np.zeros((4, 2), np.float32),
        "out": np.zeros((2, 4), np.float32), "soft": np.full((4, 2), 0.5, np.float32),
        "grad_out": np.ones((2, 4), np.float32), "grad_e": np.zeros((4, 2), np.float32),
        "grad_q": np.zeros((2, 4), np.float32), "grad_k": np.zeros((3, 4), np.float32),
        "grad_v": np.zeros((3, 4), np.float32), "grad_edge": np.zeros((4, 4), np.float32),
    }
    ptr = {k: (None if k in null else _p(v)) for k, v in keep.items()}
    L = glx.lib()
    if entry == "forward":
        rc = L.glx_dot_attention_chunked(0, ptr["q"], ptr["k"], ptr["v"], num_rows, dim, heads, ptr["rows"],
                                         ptr["edge"], ptr["cnt"], num_ids, num_segments, scale, 0.0, drop_p, 1, 2,
                                         ptr["logit_out"], ptr["soft_out"], ptr["out"], ptr_kind, None)
    else:
        rc = L.glx_dot_attention_backward_chunked(0, ptr["q"], ptr["k"], ptr["v"], num_rows, dim, heads, ptr["rows"],
                                                  ptr["edge"], ptr["cnt"], num_ids, num_segments, scale, 0.0, drop_p, 1,
                                                  2, ptr["soft"], ptr["grad_out"], ptr["grad_e"], ptr["grad_q"],
                                                  ptr["grad_k"], ptr["grad_v"], ptr["grad_edge"], ptr_kind, None)
    return rc, L.glx_last_error().decode()


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_argument_errors_need_no_gpu(entry):
    """every check of the default entry points, with the same words"""
    for kwargs, word in COMMON_ERRORS + OWN_ERRORS[entry]:
        rc, msg = _call(entry, **kwargs)
        assert rc == INVALID and word in msg, (entry, kwargs, rc, msg)


class _Recorder:
    """stands in for a ctypes entry point: records that it was called and answers GLX_OK"""

    def __init__(self):
        self.calls = 0

    def __call__(self, *args):
        self.calls += 1
        return 0


def test_the_python_flag_selects_the_entry_point(monkeypatch):
    L = glx.lib()
    names = ["glx_dot_attention", "glx_dot_attention_chunked", "glx_dot_attention_backward",
             "glx_dot_attention_backward_chunked"]
    rec = {name: _Recorder() for name in names}
    for name in names:
        monkeypatch.setattr(L, name, rec[name])
    r = cref.implied_request(8, 2, True, 1, 3, 4)
    soft = np.full((r.n, 2), 0.25, np.float32)

    def counts():
        return [rec[name].calls for name in names]

    glx.dot_attention(r.q, r.k, r.v, r.rows, edge=r.edge, heads=2)
    assert counts() == [1, 0, 0, 0]
    glx.dot_attention(r.q, r.k, r.v, r.rows, edge=r.edge, heads=2, chunked=True)
    assert counts() == [1, 1, 0, 0]
    glx.dot_attention_backward(soft, r.g, r.q, r.k, r.v, r.rows, edge=r.edge, heads=2)
    assert counts() == [1, 1, 1, 0]
    glx.dot_attention_backward(soft, r.g, r.q, r.k, r.v, r.rows, edge=r.edge, heads=2, chunked=True)
    assert counts() == [1, 1, 1, 1]


def _weights(r, seed):
    """stand-ins for the engine's alpha and grad_e: any float32 [n, heads] shows the order of the sums"""
    rng = np.random.default_rng(seed)
    alpha = rng.random((r.n, r.heads)).astype(np.float32)
    grad_e = rng.standard_normal((r.n, r.heads)).astype(np.float32)
    return alpha, grad_e


def test_without_a_long_segment_the_restatement_is_the_default_one():
    cnt = np.array([0, 256, 1, 255, 0, 40, 256], np.int32)
    n = int(cnt.sum()) + 3
    r = cref.Request(12, 3, cnt, n, len(cnt), 31, 5, with_edge=True)
    assert not cref.long_segments(cnt, n, len(cnt)).any()
    alpha, grad_e = _weights(r, 6)
    kk, vv = dref.gathered(r.k, r.rows, r.edge), dref.gathered(r.v, r.rows, r.edge)
    assert dref.same_bits(cref.out(alpha, vv, cnt, r.S), dref.out(alpha, vv, cnt, r.S))
    assert dref.same_bits(cref.grad_q(grad_e, kk, cnt, r.S), dref.grad_q(grad_e, kk, cnt, r.S))
    # and with every row named at most 256 times the chunked row gradient is the default one
    assert dref.same_bits(cref.grad_rows(alpha, r.rows, cnt, r.g, r.num_rows),
                          dref.grad_rows(alpha, r.rows, cnt, r.g, r.num_rows))


@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("dim,heads", SHAPES)
def test_on_the_gpu_tests_request_the_two_orders_differ(dim, heads, with_edge):
    """otherwise test_gpu_dot_attention_chunked.py could not tell them apart: out and grad_q of the segments of 512,
    513 and 700 positions each differ somewhere.  (257 positions need not: (0 + P0) + t is the default fold.)  Short
    segments and the list lengths of the planted rows are as the GPU test assumes."""
    r = cref.hub_request(dim, heads, with_edge, cref.hub_seed(dim, heads, with_edge))
    alpha, grad_e = _weights(r, 7)
    kk, vv = dref.gathered(r.k, r.rows, r.edge), dref.gathered(r.v, r.rows, r.edge)
    long_ = cref.long_segments(r.cnt, r.n, r.S)
    assert np.flatnonzero(long_).tolist() == [cref.SEG_257, cref.SEG_512, cref.SEG_513, cref.SEG_700, cref.SEG_ZERO,
                                              cref.SEG_NAN, cref.SEG_INF]
    for name, a, b in (("out", cref.out(alpha, vv, r.cnt, r.S), dref.out(alpha, vv, r.cnt, r.S)),
                       ("grad_q", cref.grad_q(grad_e, kk, r.cnt, r.S), dref.grad_q(grad_e, kk, r.cnt, r.S))):
        assert dref.same_bits(a[~long_], b[~long_]), name
        for sg in (cref.SEG_512, cref.SEG_513, cref.SEG_700):
            assert not dref.same_bits(a[sg], b[sg]), (name, sg)
    used = r.rows[:int(r.cnt.sum())]
    lengths = np.bincount(used[(used >= 0) & (used < r.num_rows)], minlength=r.num_rows)
    assert lengths[cref.ROW_257] == 257 and lengths[cref.ROW_700] == 700 and lengths[:56].max() <= 256
    assert (used == -1).sum() == 1 and (used == r.num_rows).sum() == 1


def test_a_chunk_of_minus_zero_terms_is_plus_zero():
    """every term of a 600-position segment is -0.0f (alpha +0.0f, vv negative): a partial that began with its first
    term, or a combine that began with its first partial, would give -0.0f"""
    n, D = 600, 4
    alpha = np.zeros((n, 1), np.float32)
    vv = np.full((n, D), -2.0, np.float32)
    assert np.signbit((alpha * vv).astype(np.float32)).all()
    got = cref.out(alpha, vv, np.array([n], np.int32), 1)
    assert dref.same_bits(got, np.zeros((1, D), np.float32)) and not np.signbit(got).any()


def test_a_dropped_chunk_adds_plus_zero():
    """chunk 1 of three has every alpha +0.0f: its partial is +0.0f and the result is (+0.0f + P0) + +0.0f + P2"""
    rng = np.random.default_rng(3)
    n, D = 700, 6
    alpha = rng.random((n, 2)).astype(np.float32)
    alpha[256:512] = 0.0
    vv = rng.standard_normal((n, D)).astype(np.float32)
    got = cref.out(alpha, vv, np.array([n], np.int32), 1)
    p0 = dref.out(alpha[:256], vv[:256], None, 1)[0]
    p2 = dref.out(alpha[512:], vv[512:], None, 1)[0]
    assert dref.same_bits(got[0], ((np.float32(0) + p0) + np.float32(0)) + p2)
    # a first chunk that cancels to -0.0f terms only leaves the sign of the sum to the later chunks
    alpha[:256] = 0.0
    vv[:256] = -1.0
    got = cref.out(alpha, vv, np.array([n], np.int32), 1)
    assert dref.same_bits(got[0], p2)
