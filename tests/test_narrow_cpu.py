"""Typed raster outputs, the part that needs no device: the numpy restatement of the conversions (tests/_narrow.py)
against a hand-written table, two float64 roundings against an fma, the host's wide-path choice against a table, and
every refusal that the Python layer and ``sknnr_narrow`` promise to make before any device work."""

from __future__ import annotations

import ctypes
import types
from fractions import Fraction

import numpy as np
import pytest

import _narrow as NR

nan, inf = np.nan, np.inf


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_restatement_int16_table():
    v = [0.5, 1.5, 2.5, -0.5, -1.5, 32767.5, 32767.49, -32768.5, -32769, 1e300, -1e300, inf, -inf, nan, -0.0]
    want = [0, 2, 2, 0, -2, 32767, 32767, -32768, -32768, 32767, -32768, 32767, -32768, 7, 0]
    got = NR.narrow_values(np.array(v), np.int16, fill=7)
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, np.array(want, dtype=np.int16))


@pytest.mark.parametrize("dtype, v, want", [(np.uint8, 255.5, 255), (np.uint8, 254.5, 254), (np.uint16, 65535.5, 65535),
                                            (np.int32, 1e300, 2147483647), (np.int32, -1e300, -2147483648),
                                            (np.uint8, -0.5, 0), (np.uint8, -3.0, 0), (np.uint16, 0.5, 0)])
def test_restatement_other_integer_types(dtype, v, want):
    got = NR.narrow_values(np.array([v]), dtype, fill=1)
    assert got.dtype == np.dtype(dtype) and int(got[0]) == want


def test_restatement_nan_without_fill_and_float32():
    assert int(NR.narrow_values(np.array([nan]), np.int16)[0]) == 0
    f = NR.narrow_values(np.array([nan, 1e39, -1e39, -0.0, 1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24, 1e-40]), np.float32)
    assert f.dtype == np.float32
    assert np.isnan(f[0]) and f[1] == inf and f[2] == -inf and np.signbit(f[3]) and f[3] == 0
    assert f[4] == np.float32(1.0) and f[5] == np.float32(1.0 + 2.0**-22)  # ties to even, both ways
    assert 0 < f[6] < np.finfo(np.float32).tiny  # a subnormal result is kept
    g = NR.narrow_values(np.array([nan, 2.0]), np.float32, fill=-9999.0)
    np.testing.assert_array_equal(g, np.array([-9999.0, 2.0], dtype=np.float32))
    np.testing.assert_array_equal(NR.narrow_indices([0, 2**31 - 1, -1]), np.array([0, 2**31 - 1, -1], dtype=np.int32))


FMA_CASES = NR.FMA_CASES


def exact_fma(v, s, o):
    return float(Fraction(v) * Fraction(s) + Fraction(o))  # (float() of a Fraction rounds once, to nearest even)


@pytest.mark.parametrize("v, s, o, two, one", FMA_CASES)
def test_two_roundings_not_an_fma(v, s, o, two, one):
    assert Fraction(v) * Fraction(s) != Fraction(float(np.float64(v) * np.float64(s))), "the product must be inexact"
    assert float(np.float64(v) * np.float64(s) + np.float64(o)) == two and exact_fma(v, s, o) == one and one != two
    got = NR.narrow_values(np.array([[v]]), np.int32, scale=[s], offset=[o], fill=0)
    assert int(got[0, 0]) == int(np.rint(two))
    gf = NR.narrow_values(np.array([[v]]), np.float32, scale=[s], offset=[o])
    assert gf[0, 0] == np.float32(two) and gf[0, 0] != np.float32(one)


def test_an_fma_would_change_stored_integers():
    assert [int(np.rint(c[3])) for c in FMA_CASES[:2]] == [0, 4] and [int(np.rint(c[4])) for c in FMA_CASES[:2]] == [1, 3]


@pytest.mark.parametrize("src, dst, esz, n, c, stride, want", [
    # packed: dst aligned to 4 elements, src to 16 bytes, one full group
    (0x1000, 0x2000, 2, 100, 3, 0, True),
    (0x1000, 0x2002, 2, 100, 3, 0, False),   # dst one element behind the boundary
    (0x1000, 0x2004, 2, 100, 3, 0, False),   # two
    (0x1000, 0x2006, 2, 100, 3, 0, False),   # three
    (0x1000, 0x2008, 2, 100, 3, 0, True),    # 8 bytes = 4 int16: aligned again
    (0x1008, 0x2000, 2, 100, 3, 0, False),   # src only 8-byte aligned: no 16-byte loads
    (0x1000, 0x2004, 1, 100, 3, 0, True),    # uint8: 4-byte stores
    (0x1000, 0x2002, 1, 100, 3, 0, False),
    (0x1000, 0x2008, 4, 100, 3, 0, False),   # int32 / float32: 16-byte stores
    (0x1000, 0x2010, 4, 100, 3, 0, True),
    (0x1000, 0x2000, 2, 1, 3, 0, False),     # fewer than 4 elements
    (0x1000, 0x2000, 2, 1, 4, 0, True),
    (0x1000, 0x2000, 2, 3, 1, 0, False),
    # planes: dst aligned and the stride a multiple of 4 elements; the source's alignment plays no part
    (0x1008, 0x2000, 2, 100, 3, 100, True),
    (0x1008, 0x2000, 2, 101, 3, 101, False),
    (0x1008, 0x2000, 2, 101, 3, 104, True),
    (0x1008, 0x2000, 2, 100, 3, 113, False),
    (0x1008, 0x2002, 2, 100, 3, 100, False),
    (0x1008, 0x2000, 2, 3, 3, 4, False),     # fewer than 4 pixels
    (0x1008, 0x2000, 2, 4, 1, 4, True),
    (0x1008, 0x2008, 4, 100, 3, 100, False),
    (0x1008, 0x2010, 4, 100, 3, 100, True),
])
def test_wide_path_choice(src, dst, esz, n, c, stride, want):
    assert NR.wide_ok(src, dst, esz, n, c, stride) is want


# ---- Python argument errors, on a fitted estimator, with no device ----------------------------------------------------
class _NoDevice:
    """Stands where the device engine would: any use beyond the target count is a failure of the test."""

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        raise AssertionError(f"the device engine was touched ({name}) before the arguments were refused")


def fitted(cls=None, y_cols=3, metric="euclidean", algorithm="brute", weights="uniform", ids=None):
    """A RawKNNRegressor in the state ``fit`` leaves it in, minus the device handle."""
    import sknnr_amd

    est = (cls or sknnr_amd.RawKNNRegressor)(n_neighbors=3, weights=weights, algorithm=algorithm)
    rng = np.random.default_rng(0)
    est._fit_X = rng.standard_normal((20, 6))
    est._y = rng.standard_normal((20, y_cols)) if y_cols else rng.standard_normal(20)
    est.n_features_in_ = 6
    est.n_samples_fit_ = 20
    est.effective_metric_ = metric
    est.effective_metric_params_ = {}
    est._fit_method = algorithm
    est._affine = est._forest = est._ref_tree = None
    est._engine = _NoDevice(max(y_cols, 1))
    if ids is not None:
        est.dataframe_index_in_ = np.asarray(ids)
    return est


TILES = [np.zeros((4, 6))]


@pytest.mark.parametrize("kwargs, match", [
    (dict(out_dtype=np.int8), "out_dtype=int8 is not supported"),
    (dict(out_dtype=np.int64), "out_dtype=int64 is not supported"),
    (dict(out_dtype=np.float16), "out_dtype=float16 is not supported"),
    (dict(out_dtype="no such type"), "not a numpy dtype"),
    (dict(scale=2.0), "scale needs out_dtype"),
    (dict(offset=1.0), "offset needs out_dtype"),
    (dict(out_nodata=-1), "out_nodata needs out_dtype"),
    (dict(out_dtype=np.float64, scale=2.0), "scale needs out_dtype"),
    (dict(out_dtype=np.int16, scale=[1.0, 2.0]), "one value per target"),
    (dict(out_dtype=np.int16, offset=[1.0, 2.0, 3.0, 4.0]), "one value per target"),
    (dict(out_dtype=np.int16, out_nodata=40000), "not representable in out_dtype=int16"),
    (dict(out_dtype=np.int16, out_nodata=0.5), "not representable in out_dtype=int16"),
    (dict(out_dtype=np.int16, out_nodata=nan), "not representable in out_dtype=int16"),
    (dict(out_dtype=np.uint8, out_nodata=-1), "not representable in out_dtype=uint8"),
    (dict(out_dtype=np.uint16, out_nodata=65536), "not representable in out_dtype=uint16"),
    (dict(out_dtype=np.int32, out_nodata=2**31), "not representable in out_dtype=int32"),
    (dict(out_dtype=np.float32, out_nodata=0.1), "not representable in out_dtype=float32"),
    (dict(out_dtype=np.int16, nodata=0.0), "out_nodata is required"),
])
def test_predict_chunks_refuses_before_any_device_work(kwargs, match):
    with pytest.raises(ValueError, match=match):
        fitted().predict_chunks(TILES, **kwargs)


@pytest.mark.parametrize("kwargs, ids, match", [
    (dict(index_dtype=np.int16), None, "index_dtype=int16 is not supported"),
    (dict(index_dtype=np.uint32), None, "index_dtype=uint32 is not supported"),
    (dict(distance_dtype=np.float16), None, "distance_dtype=float16 is not supported"),
    (dict(distance_dtype=np.int32), None, "distance_dtype=int32 is not supported"),
    (dict(index_dtype=np.int32, nodata=0.0, fill_index=2**31), None, "fill_index=2147483648 is not representable"),
    (dict(index_dtype=np.int32, nodata=0.0, fill_index=-2**31 - 1), None, "fill_index=-2147483649 is not representable"),
    (dict(index_dtype=np.int32, return_dataframe_index=True), np.arange(20) + 2**31, "needs integer dataframe ids"),
    (dict(index_dtype=np.int32, return_dataframe_index=True), np.arange(20) - 2**31 - 1, "needs integer dataframe ids"),
    (dict(index_dtype=np.int32, return_dataframe_index=True), np.arange(20) * 1.5, "needs integer dataframe ids"),
    (dict(index_dtype=np.int32, return_dataframe_index=True), np.array([f"p{i}" for i in range(20)]),
     "needs integer dataframe ids"),
])
def test_kneighbors_chunks_refuses_before_any_device_work(kwargs, ids, match):
    with pytest.raises(ValueError, match=match):
        fitted(ids=ids).kneighbors_chunks(TILES, **kwargs)


def test_host_side_paths_refuse_typed_outputs():
    import sknnr_amd

    with sknnr_amd.tree_tie_policy("tree"):
        est = fitted(algorithm="kd_tree")
        with pytest.raises(NotImplementedError, match="typed outputs are not supported under tree_tie_policy"):
            est.predict_chunks(TILES, out_dtype=np.int16)
        with pytest.raises(NotImplementedError, match="typed outputs are not supported under tree_tie_policy"):
            est.kneighbors_chunks(TILES, index_dtype=np.int32)
        with pytest.raises(NotImplementedError, match="typed outputs are not supported under tree_tie_policy"):
            est.kneighbors_chunks(TILES, distance_dtype=np.float32)
    with sknnr_amd.hamming_tie_policy("numpy"):
        est = fitted(metric="hamming")
        with pytest.raises(NotImplementedError, match="typed outputs are not supported under hamming_tie_policy"):
            est.predict_chunks(TILES, out_dtype=np.float32)
        with pytest.raises(NotImplementedError, match="typed outputs are not supported under hamming_tie_policy"):
            est.kneighbors_chunks(TILES, index_dtype=np.int32)
    est = fitted(weights=lambda d: 1.0 / (1.0 + d))
    with pytest.raises(NotImplementedError, match="typed outputs are not supported with callable weights"):
        est.predict_chunks(TILES, out_dtype=np.uint8)


def test_transformed_estimators_pass_the_arguments_through():
    import sknnr_amd
    from sknnr_amd._base import TransformedKNeighborsRegressor

    est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=3)
    assert isinstance(est, TransformedKNeighborsRegressor)
    est.regressor_ = fitted()
    est.transformer_ = types.SimpleNamespace()
    est._map_on_device = lambda: True
    with pytest.raises(ValueError, match="scale needs out_dtype"):
        est.predict_chunks(TILES, scale=2.0)
    with pytest.raises(ValueError, match="not representable in out_dtype=uint8"):
        est.predict_chunks(TILES, out_dtype=np.uint8, out_nodata=256)
    with pytest.raises(ValueError, match="index_dtype=int16 is not supported"):
        est.kneighbors_chunks(TILES, index_dtype=np.int16)


# ---- C argument errors, without a device ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    import os

    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_narrow_argument_errors_without_touching_a_device(native):
    lib = native.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    wide = ctypes.c_int32(7)

    def call(src=p, kind=NR.VALUE, n=4, c=2, dst=p, dtype=2, stride=0, scale=None, offset=None, has_fill=0, fill=0.0):
        return lib.sknnr_narrow(src, kind, n, c, dst, dtype, stride, scale, offset, has_fill, fill, 0, None,
                                ctypes.byref(wide))

    inv = native.ERR_INVALID
    for dtype in (0, 6, -1, 99):  # float64 is no narrow type; unknown codes
        assert call(dtype=dtype) == inv
    assert b"no conversion" in lib.sknnr_last_error()
    for dtype in (1, 2, 3, 4):  # indices narrow to int32 only
        assert call(kind=NR.INDEX, dtype=dtype) == inv
    assert call(kind=2) == inv and call(kind=-1) == inv
    assert call(n=-1) == inv and b"n must be" in lib.sknnr_last_error()
    assert call(c=0) == inv and call(c=65537) == inv and b"outside [1, 65536]" in lib.sknnr_last_error()
    assert call(stride=3) == inv and b"below n" in lib.sknnr_last_error()
    assert call(src=None) == inv and call(dst=None) == inv and b"NULL" in lib.sknnr_last_error()
    assert call(scale=p) == inv and call(offset=p) == inv and b"come together" in lib.sknnr_last_error()
    assert call(kind=NR.INDEX, dtype=5, scale=p, offset=p) == inv
    assert call(kind=NR.INDEX, dtype=5, has_fill=1) == inv
    assert call(has_fill=1, fill=40000.0) == inv and b"not representable" in lib.sknnr_last_error()
    assert call(has_fill=1, fill=0.5) == inv and call(has_fill=1, fill=nan) == inv
    assert call(dtype=1, has_fill=1, fill=0.1) == inv
    assert wide.value == 0
    # n == 0 is fine, before the pointers are looked at
    assert call(n=0, src=None, dst=None) == 0 and call(n=0, stride=0) == 0
    assert lib.sknnr_stream_set_output(None, 0, 0, 0, None, None, 0, 0.0) == inv
    assert lib.sknnr_stream_push_typed(None, None, 1, None, None, None) == inv
    assert lib.sknnr_stream_push_planes_typed(None, None, 1, None, None, None, 1) == inv
    assert lib.sknnr_debug_last_narrow(None, None) == inv
