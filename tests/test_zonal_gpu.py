"""Zonal statistics at estimator level: ``zones=`` / ``zonal=`` on ``predict_chunks``, and the stream-level entry points,
on the Moscow fixture (n_neighbors = 5) and a small synthetic set (37 reference rows, d = 3, k = 1).

Tiles are the 33 test rows repeated 100 times and jittered (3,300 pixels) in five pushes of 1, 1,500, 0, 700 and 1,099
pixels; the zones are 17 runs of 97 pixels repeated, with a few codes outside.  The expectation is always the numpy
model (tests/_zonal.py) applied to the WRITTEN ``out`` raster of the same call and the zones, the nodata pixels -- taken
from the input mask -- left out; ``out`` must be byte-equal to the same call without ``zonal``.

Without the feature every test here fails: the keywords, the class and the methods do not exist.

Measured on an MI355X: the 11 cases take 4.1 s, of which 3.4 s are the first fixture's device set-up; the 1,200,000-row push
takes 0.1 s.
"""

from __future__ import annotations

import numpy as np
import pytest

import _zonal as Z

pytestmark = pytest.mark.gpu

K = 5
SIZES = (1, 1_500, 0, 700, 1_099)
N = sum(SIZES)
N_ZONES = 17
NODATA = -32768
INT_COLS = slice(5, 20)  # Moscow columns whose rounded values fit int16 (the first two are UTM coordinates)
ZONE_DTYPES = (np.int64, np.uint8, np.int32, np.int16, np.uint16)


def cut(x, axis=0):
    edges = np.cumsum((0,) + SIZES)
    assert edges[-1] == x.shape[axis]
    return [np.take(x, np.arange(a, b), axis=axis) for a, b in zip(edges[:-1], edges[1:])]


def zone_codes():
    z = (np.arange(N) // 97) % N_ZONES
    z[::211] = -1
    z[5::307] = N_ZONES
    z[7::401] = N_ZONES + 40
    return z.astype(np.int64)


def zone_tiles(codes=None):
    """One array per tile, each of another integer dtype (the outside codes that a narrow unsigned type cannot hold are
    moved to another outside code it can)."""
    tiles = []
    for i, z in enumerate(cut(zone_codes() if codes is None else codes)):
        dt = ZONE_DTYPES[i % len(ZONE_DTYPES)]
        if np.dtype(dt).kind == "u":
            z = np.where(z < 0, 200, z)
        tiles.append(z.astype(dt))
    return tiles


def float_tiles(moscow):
    rng = np.random.default_rng(7)
    x = np.tile(moscow["X_test"], (100, 1))
    return cut(x * (1.0 + 0.01 * rng.standard_normal(x.shape)))


def int_tiles(moscow):
    """int16 tiles: the 1-pixel and the 1,099-pixel tile fully valid, the 1,500-pixel tile mixed, the 700-pixel tile fully
    masked."""
    rng = np.random.default_rng(8)
    x = np.tile(np.rint(moscow["X_test"][:, INT_COLS]), (100, 1)) + rng.integers(-20, 21, size=(N, 15))
    tiles = cut(x.astype(np.int16))
    rows = np.flatnonzero(rng.random(1_500) < 0.3)
    tiles[1][rows, rng.integers(0, 15, size=rows.size)] = NODATA
    tiles[3][:, 3] = NODATA
    return tiles


def as_bands(tiles):
    return [np.ascontiguousarray(t.T) for t in tiles]


def expect(z, written, zones, *, valid=None, n_classes=None, times=1):
    """``z`` against the model on the written raster ``(N, planes)`` (integers: the model's conversion leaves them as they
    are) with the masked pixels left out."""
    values = np.asarray(written).astype(np.float64)
    if valid is not None:
        values[~valid] = np.nan
    acc, hist, *_ = Z.zonal(values, zones, written.dtype, None, None, z.n_zones, n_classes)
    assert z.n_planes == written.shape[1] and z.out_dtype == written.dtype
    np.testing.assert_array_equal(z.count, times * acc[..., Z.COUNT])
    np.testing.assert_array_equal(z.acc[..., :Z.MIN], times * acc[..., :Z.MIN])
    np.testing.assert_array_equal(z.acc[..., Z.MIN:], acc[..., Z.MIN:])
    if n_classes is not None:
        blocks = Z.hist_blocks(hist, z.n_zones, n_classes)
        assert sorted(z.hist) == sorted(blocks)
        for plane, block in blocks.items():
            np.testing.assert_array_equal(z.hist[plane], times * block)
    return acc


@pytest.fixture(scope="module")
def raw(moscow):
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    y = moscow["y_train"][:, :3].copy()
    y[:, 2] = np.floor(y[:, 0]) % 6  # a class plane: codes 0 .. 5
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(moscow["X_train"], y)
    return est, float_tiles(moscow)


@pytest.mark.parametrize("layout", ["rows", "bands"])
def test_five_uneven_tiles(raw, layout):
    import sknnr_amd

    est, tiles = raw
    bands = layout == "bands"
    feed = as_bands(tiles) if bands else tiles
    kw = dict(layout=layout, out_dtype=np.int16, scale=10.0, offset=-3.0)
    shape = (3, N) if bands else (N, 3)
    base, out = np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.int16)
    est.predict_chunks(iter(feed), out=base, **kw)
    z = sknnr_amd.ZonalStats(N_ZONES)
    zones = zone_tiles()
    if bands:  # (zone codes of a band tile may keep the window's shape)
        zones[1] = zones[1].reshape(30, 50)
    got = est.predict_chunks(iter(feed), out=out, zones=iter(zones), zonal=z, **kw)
    assert out.tobytes() == base.tobytes() and got.dtype == np.int16
    written = out.T if bands else out
    acc = expect(z, written, zone_codes())
    inside = (zone_codes() >= 0) & (zone_codes() < N_ZONES)
    assert acc[..., Z.COUNT].sum() == 3 * inside.sum() and (acc[..., Z.COUNT] > 0).all()
    rec = est.engine_._index.debug_last_zonal()
    assert rec["ran"] == 1 and rec["pixels"] == N and rec["c"] == 3 and rec["outside"] == (~inside).sum(), rec
    assert rec["nan"] == 0 and rec["tallied"] == 3 * inside.sum(), rec
    # the data-unit numbers are those of the written raster
    zone3 = (written[zone_codes() == 3, 0].astype(np.float64) + 3.0) / 10.0
    np.testing.assert_allclose(z.mean[3, 0], zone3.mean(), rtol=1e-12)
    np.testing.assert_allclose(z.std[3, 0], zone3.std(), rtol=1e-9)
    assert z.min[3, 0] == zone3.min() and z.max[3, 0] == zone3.max()
    # without out: the returned predictions are the same bytes
    z2 = sknnr_amd.ZonalStats(N_ZONES)
    ret = est.predict_chunks(iter(feed), zones=iter(zone_tiles()), zonal=z2, **kw)
    assert ret.tobytes() == base.tobytes() and z2 == z


def test_lockstep_errors_add_nothing(raw):
    import sknnr_amd

    est, tiles = raw
    kw = dict(out_dtype=np.int16, scale=10.0)
    z = sknnr_amd.ZonalStats(N_ZONES)
    with pytest.raises(ValueError, match="zones ended before tiles"):
        est.predict_chunks(iter(tiles), zones=iter(zone_tiles()[:3]), zonal=z, **kw)
    with pytest.raises(ValueError, match="tiles ended before zones"):
        est.predict_chunks(iter(tiles[:4]), zones=iter(zone_tiles()), zonal=z, **kw)
    wide = zone_tiles()
    wide[1] = wide[1].astype(np.int64)
    wide[1][5] = 2**31
    with pytest.raises(ValueError, match="fit int32"):
        est.predict_chunks(iter(tiles), zones=iter(wide), zonal=z, **kw)
    with pytest.raises(ValueError, match="one code per pixel"):
        est.predict_chunks(iter(tiles), zones=iter(zone_tiles()[::-1]), zonal=z, **kw)
    assert z.n_planes is None  # (only a call that came through whole is added)
    est.predict_chunks(iter([]), zones=iter([]), zonal=z, **kw)  # nothing pushed: bound, all empty
    assert z.n_planes == 3 and not z.count.any() and np.isnan(z.mean).all()


def test_nodata_masked_valid_and_mixed_tiles(moscow):
    """int16 tiles under a nodata mask -- one tile fully masked, two fully valid, one mixed -- in both layouts: a masked
    pixel holds out_nodata in the raster and contributes nothing, though valid pixels may store the same value."""
    import sknnr_amd

    x = np.rint(moscow["X_train"][:, INT_COLS])
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K).fit(x, moscow["y_train"][:, :2])
    tiles = int_tiles(moscow)
    valid = ~(np.concatenate(tiles) == NODATA).any(axis=1)
    assert valid[0] and valid[-1_099:].all() and not valid[1_501:2_201].any() and 0 < valid[1:1_501].sum() < 1_500
    fill = 0  # (a value valid pixels store too: the tally must go by NaN, not by the fill)
    kw = dict(nodata=NODATA, out_dtype=np.uint16, scale=2.0, out_nodata=fill)
    results = []
    for layout, feed in (("rows", tiles), ("bands", as_bands(tiles))):
        shape = (N, 2) if layout == "rows" else (2, N)
        base, out = np.full(shape, 9, dtype=np.uint16), np.full(shape, 9, dtype=np.uint16)
        est.predict_chunks(iter(feed), out=base, layout=layout, **kw)
        z = sknnr_amd.ZonalStats(N_ZONES)
        est.predict_chunks(iter(feed), out=out, layout=layout, zones=iter(zone_tiles()), zonal=z, **kw)
        assert out.tobytes() == base.tobytes()
        written = out if layout == "rows" else out.T
        assert (written[~valid] == fill).all()
        expect(z, written, zone_codes(), valid=valid)
        results.append(z)
    assert results[0] == results[1]
    inside = (zone_codes() >= 0) & (zone_codes() < N_ZONES)
    assert results[0].count[:, 0].sum() == (valid & inside).sum()
    rec = est.engine_._index.debug_last_zonal()
    assert rec["nan"] == 2 * (~valid & inside).sum() and rec["pixels"] == N, rec


def test_output_plan_with_a_class_plane_and_scale_list(raw):
    """mean + two quantiles + mode from one search; the mode plane is a class plane of 5 classes (code 5 is "other");
    one scale / offset per plane, int32 so that the high limb of the sum of squares is in use."""
    import sknnr_amd

    est, tiles = raw
    plan = [(0, "mean"), (0, ("quantile", 0.1)), (0, ("quantile", 0.9)), (2, "mode")]
    kw = dict(outputs=plan, out_dtype=np.int32, scale=[1e4, 1e4, 1e4, 1.0], offset=[0.0, 5.0, -5.0, 0.0])
    base, out = np.zeros((N, 4), dtype=np.int32), np.zeros((N, 4), dtype=np.int32)
    est.predict_chunks(iter(tiles), out=base, **kw)
    z = sknnr_amd.ZonalStats(N_ZONES, classes={3: 5})
    est.predict_chunks(iter(tiles), out=out, zones=iter(zone_tiles()), zonal=z, **kw)
    assert out.tobytes() == base.tobytes()
    n_classes = np.array([0, 0, 0, 5], dtype=np.int32)
    acc = expect(z, out, zone_codes(), n_classes=n_classes)
    assert (acc[:, :3, Z.SQ_HI] > 0).any()
    codes = zone_codes()
    for zone in range(N_ZONES):
        cls = out[codes == zone, 3]
        np.testing.assert_array_equal(z.hist[3][zone], np.bincount(cls[cls < 5], minlength=5))
    assert set(np.unique(out[:, 3])) <= set(range(6)) and len(np.unique(out[:, 3])) > 1
    rec = est.engine_._index.debug_last_zonal()
    inside = (codes >= 0) & (codes < N_ZONES)
    assert rec["other"] == (out[inside, 3] == 5).sum() and rec["c"] == 4, rec
    # statistic= (per target) takes the same path
    z3 = sknnr_amd.ZonalStats(N_ZONES, classes={2: 6})
    got = est.predict_chunks(iter(tiles), statistic=["mean", "max", "mode"], out_dtype=np.int16, scale=[10.0, 10.0, 1.0],
                             zones=iter(zone_tiles()), zonal=z3)
    expect(z3, got, codes, n_classes=np.array([0, 0, 6], dtype=np.int32))
    assert est.engine_._index.debug_last_zonal()["other"] == 0


def test_with_usage_and_with_neighbors(raw):
    import sknnr_amd

    est, tiles = raw
    kw = dict(out_dtype=np.int16, scale=10.0)
    z_alone, u_alone = sknnr_amd.ZonalStats(N_ZONES), sknnr_amd.NeighborUsage()
    want = est.predict_chunks(iter(tiles), zones=iter(zone_tiles()), zonal=z_alone, **kw)
    est.predict_chunks(iter(tiles), usage=u_alone, **kw)
    z, u = sknnr_amd.ZonalStats(N_ZONES), sknnr_amd.NeighborUsage()
    got = est.predict_chunks(iter(tiles), zones=iter(zone_tiles()), zonal=z, usage=u, **kw)
    assert got.tobytes() == want.tobytes() and z == z_alone and u == u_alone
    expect(z, got, zone_codes())
    # beside the neighbours
    base = est.predict_chunks(iter(tiles), return_neighbors=True, **kw)
    zn = sknnr_amd.ZonalStats(N_ZONES)
    with_n = est.predict_chunks(iter(tiles), return_neighbors=True, zones=iter(zone_tiles()), zonal=zn, **kw)
    for a, b in zip(with_n, base):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert zn == z_alone


def test_two_calls_into_one_object(raw):
    import sknnr_amd

    est, tiles = raw
    kw = dict(out_dtype=np.int16, scale=10.0)
    whole = sknnr_amd.ZonalStats(N_ZONES)
    out = est.predict_chunks(iter(tiles), zones=iter(zone_tiles()), zonal=whole, **kw)
    parts = sknnr_amd.ZonalStats(N_ZONES)
    zt = zone_tiles()
    est.predict_chunks(iter(tiles[3:]), zones=iter(zt[3:]), zonal=parts, **kw)
    est.predict_chunks(iter(tiles[:3]), zones=iter(zt[:3]), zonal=parts, **kw)
    assert parts == whole
    est.predict_chunks(iter(tiles), zones=iter(zone_tiles()), zonal=parts, **kw)
    expect(parts, out, zone_codes(), times=2)
    before = parts.acc.copy()
    with pytest.raises(ValueError, match="bound to"):
        est.predict_chunks(iter(tiles), zones=iter(zone_tiles()), zonal=parts, out_dtype=np.int16, scale=5.0)
    np.testing.assert_array_equal(parts.acc, before)


def test_rfnn_through_the_forest_map(moscow):
    import sknnr_amd

    X, y = moscow["X_train"], moscow["y_train"][:, :2]
    est = sknnr_amd.RFNNRegressor(n_neighbors=K, n_estimators=20, random_state=0).fit(X, y)
    assert est._map_on_device()
    tiles = float_tiles(moscow)
    kw = dict(out_dtype=np.int16, scale=10.0)
    want = est.predict_chunks(iter(tiles), **kw)
    z = sknnr_amd.ZonalStats(N_ZONES)
    got = est.predict_chunks(iter(tiles), zones=iter(zone_tiles()), zonal=z, **kw)
    assert got.tobytes() == want.tobytes()
    expect(z, got, zone_codes())


@pytest.fixture(scope="module")
def small():
    """37 reference rows, d = 3, two targets."""
    import sknnr_amd

    rng = np.random.default_rng(37)
    x = rng.integers(-500, 500, size=(37, 3)).astype(np.float64)
    y = np.stack([rng.uniform(0.0, 400.0, 37), rng.uniform(-50.0, 50.0, 37)], axis=1)
    return sknnr_amd.RawKNNRegressor(n_neighbors=1).fit(x, y)


def test_one_large_push_is_cut_by_the_pipeline(small):
    """1,200,000 rows in ONE push straight on a QueryStream: the pipeline's ramp and chunk cuts split the zones array."""
    eng = small.engine_
    n, n_zones = 1_200_000, 1_000
    rng = np.random.default_rng(12)
    q = rng.integers(-500, 500, size=(n, 3)).astype(np.float64)
    zones = ((np.arange(n) // 1_200) % (n_zones + 3) - 1).astype(np.int32)  # runs of 1,200; codes -1, n_zones, n_zones + 1 too
    scale, offset = np.array([100.0, 10.0]), np.array([0.0, 1_000.0])
    stream = eng.open_stream(1, weights="uniform", want_dist=False,
                             output=dict(pred_dtype=np.int16, scale=scale, offset=offset), zonal=(n_zones, None))
    try:
        stream.next_zones(zones)
        zones[:] = -7  # (reusable on return)
        _, _, pred = stream.push(q, need_idx=False)
        acc, hist = stream.zonal()
        rec = eng._index.debug_last_zonal()
    finally:
        stream.close()
    assert hist is None and pred.dtype == np.int16 and pred.shape == (n, 2)
    zones = ((np.arange(n) // 1_200) % (n_zones + 3) - 1).astype(np.int32)
    want, _, n_nan, n_outside, _ = Z.zonal(pred.astype(np.float64), zones, np.int16, None, None, n_zones, None)
    np.testing.assert_array_equal(acc, want)
    assert rec["pixels"] == n and rec["outside"] == n_outside > 0 and rec["nan"] == n_nan == 0, rec
    assert (pred[:, 0] == 32767).any()  # (the clamp is part of what is summed)


def test_stream_level_refusals(small):
    from sknnr_amd import _native
    from sknnr_amd._base import resolve_statistic

    eng = small.engine_
    q = np.zeros((10, 3))
    typed = dict(pred_dtype=np.int16, scale=np.ones(2), offset=np.zeros(2))

    def invalid(match):
        return pytest.raises(_native.HipBackendError, match=match)

    # a push without zones; another nq; zones consumed by the push
    with eng.open_stream(1, weights="uniform", want_dist=False, output=typed, zonal=(5, None)) as s:
        with invalid("needs sknnr_stream_next_zones first") as e:
            s.push(q, need_idx=False)
        assert e.value.code == _native.ERR_INVALID
        s.next_zones(np.zeros(9, dtype=np.int32))
        with invalid("gave 9 zone codes, the push has 10 rows") as e:
            s.push(q, need_idx=False)
        assert e.value.code == _native.ERR_INVALID
        s.next_zones(np.arange(10, dtype=np.int32) % 5)
        s.push(q, need_idx=False)
        with invalid("needs sknnr_stream_next_zones first"):
            s.push(q, need_idx=False)
        # set after a push
        with invalid("only before the first push") as e:
            s.set_zonal(5)
        assert e.value.code == _native.ERR_INVALID
        acc, hist = s.zonal()
        assert hist is None and acc[..., Z.COUNT].sum() == 20 and (acc[..., Z.COUNT] == 2).all()
    # a float prediction lane at the first push
    for output in (None, dict(pred_dtype=np.float32)):
        with eng.open_stream(1, weights="uniform", want_dist=False, output=output, zonal=(5, None)) as s:
            s.next_zones(np.zeros(10, dtype=np.int32))
            with invalid("integer pred_dtype") as e:
                s.push(q, need_idx=False)
            assert e.value.code == _native.ERR_INVALID
    # a stream without predictions; a stream without zones; a plan after the zones
    with eng.open_stream(1, weights=None) as s:
        with invalid("opened without predictions"):
            s.set_zonal(5)
        with invalid("sknnr_stream_set_zonal was not called"):
            s.next_zones(np.zeros(10, dtype=np.int32))
        with pytest.raises(ValueError, match="set_zonal was not called"):
            s.zonal()
    with eng.open_stream(1, weights="uniform", want_dist=False, output=typed, zonal=(5, None)) as s:
        with invalid("comes before sknnr_stream_set_zonal"):
            s.set_plan(resolve_statistic(None, [(0, "mean")], 2).arrays)


def test_engine_zonal_from_values_numpy_and_cuda(small):
    import torch

    eng = small.engine_
    args = (np.int16, 3)
    kw = dict(scale=Z.HAND_SCALE, offset=Z.HAND_OFFSET, n_classes=Z.HAND_CLASSES)
    acc, hist = eng.zonal_from_values(Z.HAND_VALUES, Z.HAND_ZONES, *args, **kw)
    np.testing.assert_array_equal(acc, Z.HAND_ACC)
    np.testing.assert_array_equal(hist.reshape(3, 3), Z.HAND_HIST)
    acc_t, hist_t = eng.zonal_from_values(torch.from_numpy(Z.HAND_VALUES).cuda(), torch.from_numpy(Z.HAND_ZONES).cuda(), *args, **kw)
    assert acc_t.tobytes() == acc.tobytes() and hist_t.tobytes() == hist.tobytes()
