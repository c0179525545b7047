"""CPU-side checks of the code-map inference layer: tile placement, the decode ABI's argument checks (no HIP call is made) and the
ctypes bindings of the new entry points."""
import ctypes

import numpy as np
import pytest

from frl_hip import _lib
from frl_hip.inference import place_tiles


def test_place_tiles_places_and_crops():
    raster = np.full((5, 7), -1, dtype=np.int32)
    t = 4
    tiles = [np.arange(t * t, dtype=np.int32).reshape(t, t) + 100 * i for i in range(4)]
    wins = [(0, 0, 4, 4), (0, 4, 4, 3), (4, 0, 1, 4), (4, 4, 1, 3)]            # a 5 x 7 raster cut into 4 x 4 tiles: three are partial
    place_tiles(raster, wins, tiles)
    assert (raster >= 0).all()                                                 # every pixel written
    np.testing.assert_array_equal(raster[:4, :4], tiles[0])
    np.testing.assert_array_equal(raster[:4, 4:], tiles[1][:, :3])
    np.testing.assert_array_equal(raster[4:, :4], tiles[2][:1, :])
    np.testing.assert_array_equal(raster[4:, 4:], tiles[3][:1, :3])


def test_place_tiles_leading_axes():
    raster = np.zeros((2, 3, 3), dtype=np.int32)                               # [T, Y, X]
    v = np.arange(2 * 4 * 4, dtype=np.int32).reshape(2, 4, 4)
    place_tiles(raster, [(1, 1, 2, 2)], [v])
    np.testing.assert_array_equal(raster[:, 1:, 1:], v[:, :2, :2])
    assert (raster[:, 0, :] == 0).all() and (raster[:, :, 0] == 0).all()


def test_new_symbols_resolve_with_recorded_arity():
    lib = _lib.load()
    for name in ("frl_decode_codes", "frl_tcn_chain_fwd"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
    assert len(_lib.SIGNATURES["frl_decode_codes"][1]) == 9


def _decode(idx, table, out, p, k, f, dtype):
    lib = _lib.load()
    vp = ctypes.c_void_p
    return lib.frl_decode_codes(vp(idx), vp(table), vp(out), p, k, f, dtype, None, None)


@pytest.mark.parametrize("args, word", [
    ((1, 1, 1, 10, 0, 64, _lib.BF16), "K"),
    ((1, 1, 1, 10, -3, 64, _lib.F32), "K"),
    ((1, 1, 1, -1, 16, 64, _lib.BF16), "P"),
    ((1, 1, 1, 10, 16, 0, _lib.BF16), "F"),
    ((1, 1, 1, 10, 16, 64, 7), "dtype"),
    ((0, 1, 1, 10, 16, 64, _lib.BF16), "null"),
    ((1, 0, 1, 10, 16, 64, _lib.F32), "null"),
    ((1, 1, 0, 10, 16, 64, _lib.F32), "null"),
])
def test_decode_codes_argument_errors(args, word):
    """Bad arguments return a negative code with a message before any HIP call (the pointers here are not even valid addresses: a
    kernel launch or memory access would fail or crash; on a machine without a GPU any HIP call would fail too)."""
    rc = _decode(*args)
    assert rc < 0
    assert word.lower() in _lib.load().frl_last_error().decode().lower()


def test_decode_codes_empty_is_noop():
    assert _decode(0, 0, 0, 0, 16, 64, _lib.BF16) == 0
