"""Band-first raster tiles, the parts that need no device: ``normalize_band_tile`` (every accepted form, every refusal,
the dtype conversions), the ``layout`` argument of the four streamed calls, the restatement (tests/_planes.py) against
plain numpy, and the argument checks of the new C entry points, which answer before any device call."""

from __future__ import annotations

import ctypes
import inspect

import numpy as np
import pytest

import _planes as PL


# ---------------------------------------------------------------------------------------------------------------------
# normalize_band_tile
# ---------------------------------------------------------------------------------------------------------------------
def _check(bands, n, want, dtype):
    assert n == want.shape[1] and len(bands) == want.shape[0]
    for j, b in enumerate(bands):
        assert b.ndim == 1 and b.flags.c_contiguous and b.dtype == dtype
        np.testing.assert_array_equal(b, want[j])


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16, np.uint16, np.uint8, np.int32])
def test_accepted_forms_share_the_tile_s_memory(dtype):
    from sknnr_amd._base import normalize_band_tile

    cube = (np.arange(3 * 4 * 5) % 251).astype(dtype).reshape(3, 4, 5)
    want = cube.reshape(3, 20)
    for tile in (cube, cube.reshape(3, 20), cube.reshape(3, 2, 2, 5), [cube[0], cube[1], cube[2]],
                 tuple(cube[j].reshape(-1) for j in range(3))):
        bands, n = normalize_band_tile(tile, 3)
        _check(bands, n, want, dtype)
        assert all(np.shares_memory(b, cube) for b in bands), "a contiguous band of a device dtype is a view, not a copy"


def test_separate_band_arrays_and_empty_tiles():
    from sknnr_amd._base import normalize_band_tile

    a, b = np.arange(6, dtype=np.int16).reshape(2, 3), np.arange(6, 12, dtype=np.int16).reshape(2, 3)
    bands, n = normalize_band_tile([a, b], 2)
    _check(bands, n, np.stack([a.reshape(-1), b.reshape(-1)]), np.int16)
    bands, n = normalize_band_tile(np.empty((4, 0, 7), dtype=np.float32), 4)
    assert n == 0 and len(bands) == 4


def test_strided_bands_are_copied_band_by_band_in_c_order():
    from sknnr_amd._base import normalize_band_tile

    big = np.arange(3 * 6 * 8, dtype=np.uint16).reshape(3, 6, 8)
    win = big[:, 1:5, 2:7]  # a window whose raster lines are strided
    bands, n = normalize_band_tile(win, 3)
    _check(bands, n, np.stack([win[j].reshape(-1) for j in range(3)]), np.uint16)
    pixel_major = np.moveaxis(big, 0, -1)[:, :, :]  # (h, w, bands): band j is [..., j]
    bands, n = normalize_band_tile([pixel_major[..., j] for j in range(3)], 3)
    _check(bands, n, big.reshape(3, -1), np.uint16)


@pytest.mark.parametrize("dtype, forest, want", [
    (np.int64, False, np.float64), (np.uint64, False, np.float64), (np.int64, True, np.float32),
    (np.uint64, True, np.float32), (np.bool_, False, np.float64), (np.float16, True, np.float64), (np.int8, False, np.float64),
    (np.uint32, True, np.float64), (np.int16, True, np.int16), (np.float32, True, np.float32)])
def test_dtype_conversions(dtype, forest, want):
    from sknnr_amd._base import normalize_band_tile

    cube = (np.arange(24) % 2).astype(dtype).reshape(2, 3, 4)
    bands, n = normalize_band_tile(cube, 2, forest=forest)
    _check(bands, n, cube.reshape(2, 12).astype(want), want)
    # 2^53 + 1 is not a double: a 64-bit integer reaches float32 in ONE rounding for forests, as ``apply`` converts it
    if forest and dtype == np.int64:
        v = np.array([[2**53 + 1, 16777217]], dtype=np.int64)
        np.testing.assert_array_equal(normalize_band_tile(v, 1, forest=True)[0][0], v[0].astype(np.float32))


def test_refusals():
    from sknnr_amd._base import normalize_band_tile

    cube = np.zeros((3, 4, 5), dtype=np.float32)
    with pytest.raises(ValueError, match=r"X has 3 features, but RawKNNRegressor is expecting 7 features as input\."):
        normalize_band_tile(cube, 7, estimator="RawKNNRegressor")
    with pytest.raises(ValueError, match=r"X has 2 features, but .* is expecting 3 features"):
        normalize_band_tile([cube[0], cube[1]], 3)
    with pytest.raises(ValueError, match="array \\(bands, \\.\\.\\.\\)"):
        normalize_band_tile(np.zeros(5), 5)
    with pytest.raises(ValueError, match="array \\(bands, \\.\\.\\.\\)"):
        normalize_band_tile(5, 5)
    with pytest.raises(ValueError, match="share one shape and dtype"):
        normalize_band_tile([np.zeros(4), np.zeros(5)], 2)
    with pytest.raises(ValueError, match="share one shape and dtype"):
        normalize_band_tile([np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.int16)], 2)


# ---------------------------------------------------------------------------------------------------------------------
# the public signatures and the refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_is_in_the_four_public_signatures():
    from sknnr_amd._base import RawKNNRegressor, TransformedKNeighborsRegressor

    for cls in (RawKNNRegressor, TransformedKNeighborsRegressor):
        for name in ("kneighbors_chunks", "predict_chunks"):
            par = inspect.signature(getattr(cls, name)).parameters
            assert "layout" in par and par["layout"].default == "rows", f"{cls.__name__}.{name}"


@pytest.mark.parametrize("layout", ["columns", "BANDS", None, 0])
def test_unknown_layout_is_refused_before_anything_else(layout):
    from sknnr_amd import EuclideanKNNRegressor, RawKNNRegressor

    for est in (RawKNNRegressor(), EuclideanKNNRegressor()):
        with pytest.raises(ValueError, match="layout must be 'rows' or 'bands'"):
            est.kneighbors_chunks([], layout=layout)
        with pytest.raises(ValueError, match="layout must be 'rows' or 'bands'"):
            est.predict_chunks([], layout=layout)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esz", [1, 2, 4, 8])
@pytest.mark.parametrize("n, c, pad", [(1, 1, 0), (5, 3, 0), (5, 3, 2), (257, 7, 13)])
def test_restatement_is_plain_indexing(esz, n, c, pad):
    rng = np.random.default_rng(n * 100 + c)
    stride = n + pad
    src = rng.integers(0, 256, size=c * stride * esz, dtype=np.uint8).view(PL.UINT[esz])
    rows = PL.planes_to_rows(src, n, c, stride)
    assert rows.shape == (n, c) and rows.flags.c_contiguous
    for j in range(c):
        np.testing.assert_array_equal(rows[:, j], src[j * stride:j * stride + n])
    dst = np.full(c * stride + 3, 77, dtype=PL.UINT[esz])
    PL.rows_to_planes(rows, dst, stride)
    for j in range(c):
        np.testing.assert_array_equal(dst[j * stride:j * stride + n], rows[:, j])
        assert (dst[j * stride + n:(j + 1) * stride] == 77).all(), "the gap between planes is left alone"
    assert (dst[c * stride:] == 77).all()


def test_chunk_choice_against_a_table_written_by_hand():
    for esz, cols in PL.CHUNK_TABLE.items():
        assert PL.chunk_cols(esz) == cols


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: exported, bound, and refusing bad arguments without a device
# ---------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ("sknnr_planes_to_rows", "sknnr_rows_to_planes", "sknnr_stream_push_planes", "sknnr_debug_last_planes")


def test_new_entry_points_are_exported_and_bound():
    from sknnr_amd import _native

    lib = _native.load(build_if_missing=True)
    assert lib.sknnr_abi_version() == 5
    for name in NEW_ENTRY_POINTS:
        assert name in _native.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None, f"{name} has no prototype in _native.load()"


def test_argument_errors_without_touching_a_device():
    from sknnr_amd import _native

    lib = _native.load(build_if_missing=True)
    INV, OK = _native.ERR_INVALID, 0
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # sknnr_planes_to_rows(src, n, c, elem_bytes, src_stride, dst, device, stream)
    for esz in (0, 3, 5, 16, -1):
        assert lib.sknnr_planes_to_rows(p, 4, 2, esz, 4, p, 0, None) == INV and b"elem_bytes" in lib.sknnr_last_error()
    assert lib.sknnr_planes_to_rows(None, 4, 2, 2, 4, p, 0, None) == INV and b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_planes_to_rows(p, 4, 2, 2, 4, None, 0, None) == INV and b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_planes_to_rows(p, 4, 2, 2, 3, p, 0, None) == INV and b"stride" in lib.sknnr_last_error()
    assert lib.sknnr_planes_to_rows(p, 4, 0, 2, 4, p, 0, None) == INV
    assert lib.sknnr_planes_to_rows(p, 4, -3, 2, 4, p, 0, None) == INV
    assert lib.sknnr_planes_to_rows(p, 4, 65537, 2, 4, p, 0, None) == INV
    assert lib.sknnr_planes_to_rows(p, -1, 2, 2, 4, p, 0, None) == INV
    assert lib.sknnr_planes_to_rows(p, 0, 2, 2, 0, p, 0, None) == OK
    assert lib.sknnr_planes_to_rows(p, 0, 2, 3, 0, p, 0, None) == INV, "n == 0 does not excuse a bad element size"
    # sknnr_rows_to_planes(src, n, c, dst, dst_stride, device, stream)
    assert lib.sknnr_rows_to_planes(None, 4, 2, p, 4, 0, None) == INV and b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_rows_to_planes(p, 4, 2, None, 4, 0, None) == INV and b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_rows_to_planes(p, 4, 2, p, 3, 0, None) == INV and b"stride" in lib.sknnr_last_error()
    assert lib.sknnr_rows_to_planes(p, 4, 0, p, 4, 0, None) == INV
    assert lib.sknnr_rows_to_planes(p, -1, 2, p, 4, 0, None) == INV
    assert lib.sknnr_rows_to_planes(p, 0, 2, p, 0, 0, None) == OK
    # the handle entry points
    assert lib.sknnr_stream_push_planes(None, p, 4, None, p, None, 4) == INV and b"stream is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_debug_last_planes(None, (ctypes.c_int64 * 8)()) == INV
