"""The half-precision KNN scan's surface, without a GPU: the symbol, the constants and the NULL-table check."""
import glx


def test_surface_exists_and_rejects_a_null_table():
    assert "glx_knn_search_ex" in glx.EXPORTS
    assert glx.KNN_PRECISIONS == {"float32": 0, "half": 1}
    L = glx.lib()
    for precision in (0, 1):
        assert L.glx_knn_search_ex(None, 1, None, 1, 1, precision, 0, None, None, 0, None) == 3
        assert b"NULL" in L.glx_last_error()
