"""glx_knn_ivf_search_prec without a GPU: the name is in glx.EXPORTS, in the header and in the built library, and a NULL
index is refused before anything touches a device."""
import os
import re

import glx

NAME = "glx_knn_ivf_search_prec"
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "glx.h")


def test_the_entry_point_is_exported_and_declared():
    assert NAME in glx.EXPORTS
    with open(HEADER) as f:
        assert re.search(r"GLX_API int %s\(" % NAME, f.read())
    assert hasattr(glx.lib(), NAME)


def test_a_null_index_is_an_invalid_argument():
    L = glx.lib()
    for precision in (0, 1):
        assert L.glx_knn_ivf_search_prec(None, 1, None, 0, 1, 1, 1, precision, 0, None, None, 0, None) == 3
        assert b"index is NULL" in L.glx_last_error()
