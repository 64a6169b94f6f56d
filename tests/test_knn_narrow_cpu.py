"""The narrow KNN tile's surface, without a GPU: the symbol, the tile check and the Python argument."""
import numpy as np
import pytest

import glx


def test_surface_exists_and_rejects_a_bad_tile():
    assert "glx_knn_search_tiled" in glx.EXPORTS and glx.KNN_TILES == {"wide": 0, "narrow": 1}
    L = glx.lib()
    for tile in (2, -1):
        assert L.glx_knn_search_tiled(None, 1, None, 1, 1, 0, 0, tile, None, None, 0, None) == 3
        assert b"tile" in L.glx_last_error()
    with pytest.raises(ValueError, match="tile"):
        glx.Features.search(None, np.zeros((1, 4), np.float32), 1, tile="thin")
