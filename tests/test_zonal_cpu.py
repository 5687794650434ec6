"""Zonal statistics without a device: the numpy model of the contract (tests/_zonal.py) on a case worked out by hand, the
limb identity of the sum of squares, the value semantics and the data-unit numbers of ``sknnr_amd.ZonalStats``, the
refusals of ``zones=`` / ``zonal=`` that come before any device work, and the new C symbols on NULL handles."""

from __future__ import annotations

import ctypes
import pickle

import numpy as np
import pytest

import _zonal as Z


def test_model_on_the_hand_written_case():
    acc, hist, n_nan, n_outside, n_other = Z.zonal(Z.HAND_VALUES, Z.HAND_ZONES, np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 3,
                                                   Z.HAND_CLASSES)
    np.testing.assert_array_equal(acc, Z.HAND_ACC)
    np.testing.assert_array_equal(hist.reshape(3, 3), Z.HAND_HIST)
    assert (n_nan, n_outside, n_other) == Z.HAND_COUNTERS
    # every entry is tallied, NaN or in a pixel outside the zones
    assert acc[..., Z.COUNT].sum() + n_nan + n_outside * 2 == Z.HAND_VALUES.size
    # accumulate: counts, sums and limbs double; min and max stay
    again, hist2, *_ = Z.zonal(Z.HAND_VALUES, Z.HAND_ZONES, np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 3, Z.HAND_CLASSES,
                               acc.copy(), hist.copy())
    np.testing.assert_array_equal(again[..., :Z.MIN], 2 * Z.HAND_ACC[..., :Z.MIN])
    np.testing.assert_array_equal(again[..., Z.MIN:], Z.HAND_ACC[..., Z.MIN:])
    np.testing.assert_array_equal(hist2.reshape(3, 3), 2 * Z.HAND_HIST)
    # a zone nothing fell into keeps the sentinels
    acc5, *_ = Z.zonal(Z.HAND_VALUES, Z.HAND_ZONES, np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 5, None)
    np.testing.assert_array_equal(acc5[4], [[0, 0, 0, 0, Z.I64_MAX, Z.I64_MIN]] * 2)
    np.testing.assert_array_equal(acc5[3, 0], [1, 80, 6400, 0, 80, 80])  # (zone code 3 now exists)


def test_limb_identity_on_int32_extremes():
    q = [-2**31, 2**31 - 1, -2**30, 2**30, 65536, -65537, 0, 1, -1, 2**31 - 1, -2**31]
    values = np.array(q, dtype=np.float64).reshape(-1, 1)
    acc, *_ = Z.zonal(values, np.zeros(len(q), dtype=np.int32), np.int32, None, None, 1, None)
    count, s, lo, hi, mn, mx = (int(v) for v in acc[0, 0])
    assert count == len(q) and s == sum(q) and (mn, mx) == (min(q), max(q))
    assert hi * 2**32 + lo == sum(v * v for v in q)  # Python ints: exact
    assert lo == sum((v * v) % 2**32 for v in q) and hi == sum((v * v) >> 32 for v in q) and hi > 0
    # the narrow types never reach the high limb
    acc16, *_ = Z.zonal(np.array([[-32768.0], [32767.0]]), [0, 0], np.int16, None, None, 1, None)
    assert acc16[0, 0, Z.SQ_HI] == 0 and acc16[0, 0, Z.SQ_LO] == 32768**2 + 32767**2


def stats_of(acc, hist=None, *, n_zones=3, classes=None, dtype=np.int16, scale=None, offset=None, labels=None):
    import sknnr_amd

    z = sknnr_amd.ZonalStats(n_zones, classes=classes, labels=labels)
    return z._bind(acc.shape[1], dtype, scale, offset)._add(acc, hist)


def test_zonal_stats_binding_and_nan_where_empty():
    import sknnr_amd

    assert "ZonalStats" not in sknnr_amd.__all__
    z = sknnr_amd.ZonalStats(4, classes={1: 3}, labels=["a", "b", "c", "d"])
    assert z.n_planes is None and "unbound" in repr(z)
    with pytest.raises(ValueError, match="tallied nothing"):
        z.count
    z._check(2, np.int16, [10.0, 1.0], None)  # (unbound: any binding the classes fit)
    with pytest.raises(ValueError, match="classes names plane 1"):
        z._check(1, np.int16)
    with pytest.raises(ValueError, match="stored integers"):
        z._check(2, np.float32)
    acc, hist = Z.empty(4, 2, Z.HAND_CLASSES)
    Z.zonal(Z.HAND_VALUES, Z.HAND_ZONES, np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 4, Z.HAND_CLASSES, acc, hist)
    z._bind(2, np.int16, [10.0, 1.0], 0.0)._add(acc, hist)
    assert z.n_planes == 2 and z.out_dtype == np.int16 and "n_zones=4, n_planes=2" in repr(z)
    np.testing.assert_array_equal(z.count, acc[..., Z.COUNT])
    np.testing.assert_array_equal(z.sum_stored[:3], Z.HAND_ACC[..., Z.SUM])
    np.testing.assert_array_equal(z.min_stored[:3], Z.HAND_ACC[..., Z.MIN])
    np.testing.assert_array_equal(z.max_stored[:3], Z.HAND_ACC[..., Z.MAX])
    np.testing.assert_array_equal(z.hist[1][:3], Z.HAND_HIST)
    assert list(z.hist) == [1] and z.count.dtype == np.int64
    for name in ("mean", "total", "std", "min", "max"):
        got = getattr(z, name)
        assert got.shape == (4, 2) and got.dtype == np.float64
        np.testing.assert_array_equal(np.isnan(got), z.count == 0)
    empty = sknnr_amd.ZonalStats(2)._bind(1, np.uint8)
    for name in ("mean", "total", "std", "min", "max"):
        assert np.isnan(getattr(empty, name)).all()
    np.testing.assert_array_equal(z.mean[0], [2.0, 1.0])  # stored 10, 20, 30 at scale 10; classes 0, 1, 2
    np.testing.assert_array_equal(z.total[0], [6.0, 3.0])
    np.testing.assert_array_equal(z.min[1], [-1.5, 1.0])
    np.testing.assert_array_equal(z.max[2], [3276.7, 0.0])
    # bound now: another binding is refused, and changes nothing
    for other in ((3, np.int16, [10.0, 1.0, 1.0], None), (2, np.int32, [10.0, 1.0], None), (2, np.int16, None, None),
                  (2, np.int16, [10.0, 1.0], 1.0)):
        with pytest.raises(ValueError, match="bound to"):
            z._check(*other)
    with pytest.raises(ValueError, match="acc must be"):
        z._add(np.zeros((3, 2, 6), dtype=np.int64), hist)
    np.testing.assert_array_equal(z.count, acc[..., Z.COUNT])
    for bad in (dict(n_zones=0), dict(n_zones=2, classes={0: 0}), dict(n_zones=2, classes={-1: 3}), dict(n_zones=2, labels=["a"])):
        with pytest.raises(ValueError):
            sknnr_amd.ZonalStats(**bad)


def test_zonal_stats_merge_pickle_and_equality():
    import sknnr_amd

    kw = dict(classes={1: 3}, scale=[10.0, 1.0], offset=[0.0, 0.0])
    a = stats_of(Z.HAND_ACC, Z.HAND_HIST.reshape(-1), **kw)
    rev_acc, rev_hist, *_ = Z.zonal(Z.HAND_VALUES, 2 - Z.HAND_ZONES, np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 3, Z.HAND_CLASSES)
    b = stats_of(rev_acc, rev_hist, **kw)
    both = pickle.loads(pickle.dumps(a))
    assert both == a and both is not a and both != b
    both += b
    one_acc, one_hist, *_ = Z.zonal(np.concatenate([Z.HAND_VALUES] * 2), np.concatenate([Z.HAND_ZONES, 2 - Z.HAND_ZONES]),
                                    np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 3, Z.HAND_CLASSES)
    np.testing.assert_array_equal(both.acc, one_acc)
    np.testing.assert_array_equal(both.hist[1], one_hist.reshape(3, 3))
    assert both != a and a == stats_of(Z.HAND_ACC, Z.HAND_HIST.reshape(-1), **kw)  # (+= left the right-hand side alone)
    assert a != stats_of(Z.HAND_ACC, Z.HAND_HIST.reshape(-1), labels=["x", "y", "z"], **kw)  # labels are part of the value
    empty = sknnr_amd.ZonalStats(3, classes={1: 3})
    empty += a  # binds
    assert empty == a
    a += sknnr_amd.ZonalStats(3, classes={1: 3})  # an unbound one adds nothing
    assert empty == a
    with pytest.raises(ValueError, match="bound to"):
        a += stats_of(Z.HAND_ACC, Z.HAND_HIST.reshape(-1), classes={1: 3}, scale=[1.0, 1.0], offset=[0.0, 0.0])
    with pytest.raises(ValueError, match="cannot merge"):
        a += sknnr_amd.ZonalStats(4, classes={1: 3})
    with pytest.raises(ValueError, match="cannot merge"):
        a += sknnr_amd.ZonalStats(3)
    with pytest.raises(TypeError):
        hash(a)
    assert sknnr_amd.ZonalStats(3) == sknnr_amd.ZonalStats(3) and sknnr_amd.ZonalStats(3) != sknnr_amd.ZonalStats(4)


@pytest.mark.parametrize("dtype, scale, offset", [(np.int16, 10.0, -500.0), (np.int32, 1000.0, 0.0), (np.uint8, -0.5, 200.0)])
def test_mean_and_std_against_numpy_on_a_small_raster(dtype, scale, offset):
    rng = np.random.default_rng(5)
    h, w, n_zones = 37, 53, 8
    values = rng.normal(120.0, 60.0, size=(h * w, 2)) * (1000.0 if dtype == np.int32 else 1.0)
    zones = (np.arange(h * w) // w // 6 + rng.integers(0, 2, h * w)).astype(np.int32)  # rough bands
    zones[rng.random(h * w) < 0.01] = -1
    values[rng.random(h * w) < 0.02] = np.nan
    sc, off = np.array([scale, 1.0]), np.array([offset, 0.0])
    acc, *_ = Z.zonal(values, zones, dtype, sc, off, n_zones + 1, None)  # (the last zone stays empty)
    z = stats_of(acc, n_zones=n_zones + 1, dtype=dtype, scale=sc, offset=off)
    from _narrow import narrow_values

    stored = narrow_values(values, dtype, sc, off).astype(np.float64)
    for zone in range(n_zones):
        for j in range(2):
            pick = (zones == zone) & ~np.isnan(values[:, j])
            data = (stored[pick, j] - off[j]) / sc[j]
            assert z.count[zone, j] == pick.sum() > 0
            np.testing.assert_allclose(z.mean[zone, j], np.mean(data), rtol=1e-12)
            np.testing.assert_allclose(z.total[zone, j], np.sum(data), rtol=1e-12)
            np.testing.assert_allclose(z.std[zone, j], np.std(data), rtol=1e-9)
            assert z.min[zone, j] == data.min() and z.max[zone, j] == data.max()
    assert np.isnan(z.mean[n_zones]).all() and np.isnan(z.std[n_zones]).all()
    # the variance's numerator is exact: a constant zone has std 0.0, not a rounding residue
    const = np.full((1000, 1), 2**31 - 1, dtype=np.float64)
    acc_c, *_ = Z.zonal(const, np.zeros(1000, dtype=np.int32), np.int32, None, None, 1, None)
    assert stats_of(acc_c, n_zones=1, dtype=np.int32).std[0, 0] == 0.0


class _Fitted:
    """The pieces of a fitted estimator the refusals of ``zonal=`` read before any device work."""

    def __new__(cls, weights="uniform", k=5):
        import sknnr_amd

        est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights)
        est._fit_X = np.zeros((12, 3))
        est._y = np.zeros((12, 2))
        est.n_samples_fit_, est.n_features_in_ = 12, 3
        est._fit_method = "brute"
        return est


def test_zonal_refusals_need_no_device():
    import sknnr_amd

    tiles, zones = [np.zeros((4, 3))], [np.zeros(4, dtype=np.int32)]
    typed = dict(out_dtype=np.int16, scale=10.0)
    est = _Fitted()
    # one without the other
    with pytest.raises(ValueError, match="zones and zonal come together"):
        est.predict_chunks(iter(tiles), zonal=sknnr_amd.ZonalStats(3), **typed)
    with pytest.raises(ValueError, match="zones and zonal come together"):
        est.predict_chunks(iter(tiles), zones=iter(zones), **typed)
    # a float or missing out_dtype: no order-independent sum
    with pytest.raises(NotImplementedError, match="float atomic sum is order-dependent.*stored integers"):
        est.predict_chunks(iter(tiles), zones=iter(zones), zonal=sknnr_amd.ZonalStats(3))
    with pytest.raises(NotImplementedError, match="float atomic sum is order-dependent"):
        est.predict_chunks(iter(tiles), zones=iter(zones), zonal=sknnr_amd.ZonalStats(3), out_dtype=np.float32)
    # classes naming a plane that does not exist: two targets, plane 2
    with pytest.raises(ValueError, match="classes names plane 2: the output has 2"):
        est.predict_chunks(iter(tiles), zones=iter(zones), zonal=sknnr_amd.ZonalStats(3, classes={2: 4}), **typed)
    with pytest.raises(ValueError, match="classes names plane 3: the output has 3"):
        est.predict_chunks(iter(tiles), zones=iter(zones), zonal=sknnr_amd.ZonalStats(3, classes={3: 4}),
                           outputs=[(0, "mean"), (1, "mean"), (1, "mode")], **typed)
    # an object bound to another output
    bound = sknnr_amd.ZonalStats(3)._bind(2, np.int16, 1.0, 0.0)
    with pytest.raises(ValueError, match="bound to"):
        est.predict_chunks(iter(tiles), zones=iter(zones), zonal=bound, **typed)
    with pytest.raises(TypeError, match="ZonalStats"):
        est.predict_chunks(iter(tiles), zones=iter(zones), zonal=object(), **typed)
    # a callable runs on the host between the search and the reduction
    with pytest.raises(NotImplementedError, match="zonal is not supported with callable weights"):
        _Fitted(weights=lambda d: 1.0 / (1.0 + d)).predict_chunks(iter(tiles), zones=iter(zones),
                                                                    zonal=sknnr_amd.ZonalStats(3), **typed)
    # the host-side tie policies answer tile by tile on the host
    with sknnr_amd.tree_tie_policy("tree"):
        tree = _Fitted()
        tree._fit_method = "kd_tree"
        with pytest.raises(NotImplementedError, match=r"zonal is not supported under tree_tie_policy\('tree'\)"):
            tree.predict_chunks(iter(tiles), zones=iter(zones), zonal=sknnr_amd.ZonalStats(3), **typed)
    with sknnr_amd.hamming_tie_policy("numpy"):
        ham = _Fitted()
        ham.effective_metric_ = "hamming"
        with pytest.raises(NotImplementedError, match=r"zonal is not supported under hamming_tie_policy\('numpy'\)"):
            ham.predict_chunks(iter(tiles), zones=iter(zones), zonal=sknnr_amd.ZonalStats(3), **typed)
    # the transformed family takes the keywords too (and refuses before it is even fitted-checked for the device)
    import inspect

    for cls in (sknnr_amd.RawKNNRegressor, sknnr_amd.GNNRegressor, sknnr_amd.RFNNRegressor):
        params = inspect.signature(cls.predict_chunks).parameters
        assert "zones" in params and "zonal" in params


def test_zone_tiles_are_normalised_to_int32():
    from sknnr_amd._base import normalize_zone_tile

    for dt in (np.uint8, np.int16, np.uint16, np.int32, np.int64, np.uint64):
        got = normalize_zone_tile(np.arange(6, dtype=dt).reshape(2, 3), 6)
        assert got.dtype == np.int32 and got.shape == (6,) and got.flags.c_contiguous
        np.testing.assert_array_equal(got, np.arange(6))
    np.testing.assert_array_equal(normalize_zone_tile(np.array([-1, 2**31 - 1], dtype=np.int64), 2), [-1, 2**31 - 1])
    with pytest.raises(ValueError, match="fit int32"):
        normalize_zone_tile(np.array([0, 2**31], dtype=np.int64), 2)
    with pytest.raises(ValueError, match="fit int32"):
        normalize_zone_tile(np.array([-2**31 - 1, 0], dtype=np.int64), 2)
    with pytest.raises(ValueError, match="integer zone codes"):
        normalize_zone_tile(np.zeros(4), 4)
    with pytest.raises(ValueError, match="one code per pixel"):
        normalize_zone_tile(np.zeros(5, dtype=np.int32), 4)


@pytest.fixture(scope="module")
def native():
    import os

    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_new_symbols_refuse_null_handles(native):
    lib = native.load()
    acc = (ctypes.c_int64 * 6)()
    out = (ctypes.c_int64 * 8)()
    zones = (ctypes.c_int32 * 1)()
    assert lib.sknnr_zonal_from_values(None, None, None, 0, 1, 2, None, None, 1, None, acc, None, 0, native.MEM_HOST,
                                       None) == native.ERR_INVALID
    assert b"index is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_stream_set_zonal(None, 3, None) == native.ERR_INVALID
    assert b"stream is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_stream_next_zones(None, zones, 1) == native.ERR_INVALID
    assert lib.sknnr_stream_get_zonal(None, acc, None) == native.ERR_INVALID
    assert lib.sknnr_debug_last_zonal(None, out) == native.ERR_INVALID
    assert lib.sknnr_debug_zonal_geometry(0, out) == native.ERR_INVALID
    geo = native.zonal_geometry(3)  # (no device work)
    assert geo["pixels_per_workgroup"] >= 1 and geo["probes"] >= 1
    assert native.zonal_geometry(10**6)["pixels_per_workgroup"] == 1
