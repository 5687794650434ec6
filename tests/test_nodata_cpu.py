"""Nodata handling, the parts that need no GPU: the argument checks of ``normalize_nodata``, the host restatement of the
mask / compaction / expansion kernels (tests/_nodata.py) against plain boolean indexing, and the new C entry points in
the built library and the ctypes binding."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import _nodata as ND

NEW_SYMBOLS = ("sknnr_mask_rows", "sknnr_kneighbors_masked", "sknnr_predict_masked", "sknnr_stream_set_nodata",
               "sknnr_stream_valid_rows", "sknnr_debug_last_mask", "sknnr_debug_mask_compact", "sknnr_debug_expand_rows")


def test_normalize_nodata():
    from sknnr_amd._base import normalize_nodata

    out = normalize_nodata(-32768, 4, np.int16)
    assert out.dtype == np.float64 and out.shape == (4,) and (out == -32768.0).all() and out.flags.c_contiguous
    np.testing.assert_array_equal(normalize_nodata([0, 255, 7], 3, np.uint8), [0.0, 255.0, 7.0])
    np.testing.assert_array_equal(normalize_nodata(np.array([1.5, np.nan]), 2, np.float32), [1.5, np.nan])
    assert np.isnan(normalize_nodata(np.nan, 3, np.float64)).all()
    np.testing.assert_array_equal(normalize_nodata(np.int16(-1), 2, np.float64), [-1.0, -1.0])
    for bad in ([1, 2], [1, 2, 3, 4], [[1, 2, 3]], []):
        with pytest.raises(ValueError, match="expected 3"):
            normalize_nodata(bad, 3, np.float64)
    with pytest.raises(ValueError, match="column 1 is NaN"):
        normalize_nodata([0, np.nan, np.nan], 3, np.int16)
    with pytest.raises(ValueError, match="column 0 is NaN"):
        normalize_nodata(np.nan, 3, np.uint8)
    with pytest.raises(ValueError, match="nodata must be"):
        normalize_nodata("cloud", 3, np.float64)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
@pytest.mark.parametrize("d_in", [1, 7, 32])
def test_restated_mask_is_plain_indexing(dtype, d_in):
    rng = np.random.default_rng(d_in)
    nq = 1000
    x = rng.integers(0, 5, size=(nq, d_in)).astype(dtype)
    nodata = rng.integers(0, 5, size=d_in).astype(np.float64)
    if np.dtype(dtype).kind == "f":
        x[rng.random(x.shape) < 0.02] = np.nan
        nodata[::2] = np.nan
    valid = ND.row_mask(x, nodata)
    want = np.ones(nq, dtype=bool)
    for c in range(d_in):
        col = x[:, c].astype(np.float64)
        want &= ~(np.isnan(col) if np.isnan(nodata[c]) else col == nodata[c])
    np.testing.assert_array_equal(valid, want.astype(np.uint8))
    assert 0 < valid.sum() < nq or d_in > 7


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257, 1025, 5000])
@pytest.mark.parametrize("kind", ND.MASK_KINDS)
def test_restated_compaction_is_plain_indexing(nq, kind):
    rng = np.random.default_rng(nq)
    x = rng.integers(-100, 100, size=(nq, 7)).astype(np.int16)
    valid = ~ND.make_mask(kind, nq)
    counts = ND.block_counts(valid)
    offsets, total = ND.exclusive_scan(counts)
    assert counts.size == ND.mask_blocks(nq) and total == valid.sum() and (np.diff(offsets) == counts[:-1]).all()
    rk = ND.ranks(valid)
    np.testing.assert_array_equal(rk, np.cumsum(valid) - valid)  # the exclusive prefix over the whole tile
    packed = ND.compact(x, valid)
    np.testing.assert_array_equal(packed, x[valid])  # stable: order preserved
    res = rng.integers(0, 500, size=(int(valid.sum()), 3))
    full = ND.expand(valid, res, -1)
    np.testing.assert_array_equal(full[valid], res)
    assert (full[~valid] == -1).all()
    dist = ND.expand(valid, res.astype(np.float64), np.nan)
    assert np.isnan(dist[~valid]).all() and np.array_equal(dist[valid], res.astype(np.float64))
    assert ND.expected_path(valid) == (1 if valid.all() else 2 if not valid.any() else 0)
    if kind in ("none", "all"):
        assert ND.expected_path(valid) == {"none": ND.PATH_IN_PLACE, "all": ND.PATH_ALL_MASKED}[kind]


# (source address, output address, row bytes) -> bytes per copy, written out by hand: the largest power of two up to 16
# that divides all three
COMPACT_UNIT_TABLE = [
    (0x7F0000000000, 0x7F0000100000, 1, 1), (0x7F0000000000, 0x7F0000100000, 3, 1), (0x7F0000000000, 0x7F0000100000, 7, 1),
    (0x7F0000000000, 0x7F0000100000, 2, 2), (0x7F0000000000, 0x7F0000100000, 14, 2), (0x7F0000000000, 0x7F0000100000, 6, 2),
    (0x7F0000000000, 0x7F0000100000, 4, 4), (0x7F0000000000, 0x7F0000100000, 12, 4), (0x7F0000000000, 0x7F0000100000, 28, 4),
    (0x7F0000000000, 0x7F0000100000, 8, 8), (0x7F0000000000, 0x7F0000100000, 24, 8), (0x7F0000000000, 0x7F0000100000, 56, 8),
    (0x7F0000000000, 0x7F0000100000, 16, 16), (0x7F0000000000, 0x7F0000100000, 48, 16),
    (0x7F0000000000, 0x7F0000100000, 32, 16), (0x7F0000000000, 0x7F0000100000, 2048, 16),
    (0x7F0000000000, 0x7F0000100000, 1 << 19, 16),
    # an address less aligned than the row size lowers the unit: the source alone, the output alone, both
    (0x7F0000000004, 0x7F0000100000, 16, 4), (0x7F0000000000, 0x7F0000100004, 16, 4), (0x7F0000000004, 0x7F0000100004, 16, 4),
    (0x7F0000000008, 0x7F0000100000, 16, 8), (0x7F0000000008, 0x7F0000100004, 16, 4), (0x7F0000000002, 0x7F0000100008, 48, 2),
    (0x7F0000000000, 0x7F0000100001, 4, 1), (0x7F0000000003, 0x7F0000100000, 2048, 1), (0x7F0000000001, 0x7F0000100001, 8, 1),
    (0x7F0000000010, 0x7F0000100030, 64, 16), (0x7F0000000020, 0x7F0000100010, 24, 8), (0x7F0000000006, 0x7F0000100000, 12, 2),
    # ... and never raises it above what the row size allows
    (0x7F0000000010, 0x7F0000100010, 14, 2), (0x7F0000000008, 0x7F0000100008, 7, 1), (0x7F0000000100, 0x7F0000100100, 12, 4),
    (0, 0, 5, 1), (0, 0, 16, 16), (0, 0, 40, 8),
]


def test_compact_unit_against_a_table_written_by_hand():
    for x_addr, out_addr, row_bytes, want in COMPACT_UNIT_TABLE:
        got = ND.compact_unit(x_addr, out_addr, row_bytes)
        assert got == want, (hex(x_addr), hex(out_addr), row_bytes, got, want)
        # what a unit must be for the kernel's typed loads and stores to be aligned and whole
        assert x_addr % got == 0 and out_addr % got == 0 and row_bytes % got == 0 and got in (1, 2, 4, 8, 16)
        assert got == 16 or any(v % (2 * got) for v in (x_addr, out_addr, row_bytes)), "a larger unit divides all three"


def test_blob_mask_fraction():
    m = ND.blob_mask(100_000, 0.3, seed=1)
    assert 0.3 <= m.mean() < 0.36
    assert (np.diff(m.astype(np.int8)) != 0).sum() < 400  # contiguous runs, not scattered pixels
    assert ND.blob_mask(10, 1.0).all() and not ND.blob_mask(10, 0.0).any()


def test_new_entry_points_are_exported_and_bound():
    from sknnr_amd import _native

    lib = ctypes.CDLL(_native.library_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in _native.EXPORTED_SYMBOLS
        assert getattr(_native.load(), name).argtypes is not None, f"{name} has no prototype in _native.load()"
    for method in ("kneighbors_masked_host", "predict_masked_host", "kneighbors_masked_device", "predict_masked_device",
                   "debug_last_mask"):
        assert callable(getattr(_native.Index, method))
    assert callable(_native.QueryStream.set_nodata) and callable(_native.QueryStream.valid_rows)
    assert callable(_native.mask_rows_host) and callable(_native.mask_rows_device)
    assert callable(_native.debug_mask_compact) and callable(_native.debug_expand_rows)


def test_argument_errors_without_touching_a_device():
    from sknnr_amd import _native

    lib = _native.load()
    nv = ctypes.c_int64(-1)
    nd = (ctypes.c_double * 2)(0.0, 0.0)
    assert lib.sknnr_mask_rows(None, 4, 0, 0, nd, 0, 0, None, None, ctypes.byref(nv)) == _native.ERR_INVALID
    assert b"d_in" in lib.sknnr_last_error()
    assert lib.sknnr_mask_rows(None, 4, 2, 99, nd, 0, 0, None, None, ctypes.byref(nv)) == _native.ERR_INVALID
    assert lib.sknnr_mask_rows(None, 4, 2, 0, None, 0, 0, None, None, ctypes.byref(nv)) == _native.ERR_INVALID
    assert lib.sknnr_mask_rows(None, 0, 2, 0, nd, 0, 0, None, None, ctypes.byref(nv)) == 0 and nv.value == 0
    assert lib.sknnr_kneighbors_masked(None, None, 1, None, nd, -1, None, None, 0, None, None) == _native.ERR_INVALID
    assert lib.sknnr_predict_masked(None, None, 1, None, nd, -1, None, None, None, 0, None, None) == _native.ERR_INVALID
    assert lib.sknnr_stream_set_nodata(None, nd, -1) == _native.ERR_INVALID
    assert lib.sknnr_stream_valid_rows(None, ctypes.byref(nv)) == _native.ERR_INVALID
    assert lib.sknnr_debug_last_mask(None, (ctypes.c_int64 * 8)()) == _native.ERR_INVALID
    unit = ctypes.c_int32(-1)
    assert lib.sknnr_debug_mask_compact(None, 4, 0, 0, nd, 0, None, None, None, None, None, ctypes.byref(unit),
                                        ctypes.byref(nv)) == _native.ERR_INVALID
    assert lib.sknnr_debug_mask_compact(None, 4, 2, 99, nd, 0, None, None, None, None, None, ctypes.byref(unit),
                                        ctypes.byref(nv)) == _native.ERR_INVALID
    assert lib.sknnr_debug_mask_compact(None, -1, 2, 0, nd, 0, None, None, None, None, None, ctypes.byref(unit),
                                        ctypes.byref(nv)) == _native.ERR_INVALID
    assert lib.sknnr_debug_mask_compact(None, 4, 2, 0, None, 0, None, None, None, None, None, ctypes.byref(unit),
                                        ctypes.byref(nv)) == _native.ERR_INVALID
    # no rows: nothing is launched, the unit is still the one of (NULL, NULL, 2 x float64)
    assert lib.sknnr_debug_mask_compact(None, 0, 2, 0, nd, 0, None, None, None, None, None, ctypes.byref(unit),
                                        ctypes.byref(nv)) == 0 and nv.value == 0 and unit.value == 16
    assert lib.sknnr_debug_mask_compact(None, 4, 2, 0, nd, 0, None, None, None, None, None, ctypes.byref(unit),
                                        ctypes.byref(nv)) == _native.ERR_INVALID and b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_debug_expand_rows(-1, 3, 2, *[None] * 8, -1, None) == _native.ERR_INVALID
    assert lib.sknnr_debug_expand_rows(4, 0, 2, *[None] * 8, -1, None) == _native.ERR_INVALID
    assert lib.sknnr_debug_expand_rows(4, 3, 0, *[None] * 8, -1, None) == _native.ERR_INVALID
