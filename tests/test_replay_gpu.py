"""Neighbour replay end to end: ``predict_neighbors_chunks`` on the neighbour rasters a search call stored gives, bit for
bit, what that search call gave -- predictions, statistics, output plans, typed outputs, usage, zonal tables and the
distance domain -- for rows and bands, full and narrow storage, an attribute table the estimator was never fitted with,
the leading columns of a wider store, and unknown values.

n_ref = 300, d = 6, t = 3, k = 5; tiles of 700, 1, 0 and 1300 pixels; every 13th pixel is nodata in one band.

Without the feature every test here fails with ``AttributeError`` (no ``predict_neighbors_chunks`` / ``TargetIndex``)."""

from __future__ import annotations

import numpy as np
import pytest

import _replay as RP

pytestmark = pytest.mark.gpu

K = 5
SIZES = (700, 1, 0, 1300)
N = sum(SIZES)
NODATA = -32768
N_ZONES = 7
WEIGHTS = ("uniform", "distance", "law")


def cut(x, axis=0):
    edges = np.cumsum((0,) + SIZES)
    return [np.take(x, np.arange(a, b), axis=axis) for a, b in zip(edges[:-1], edges[1:])]


def reference_rows():
    rng = np.random.default_rng(31)
    X = rng.integers(100, 900, size=(300, 6)).astype(np.float64)
    X[10] = X[11]  # (two co-located plots: exact zero distances and ties)
    y = np.column_stack([X[:, 0] * 0.5 + X[:, 1], np.sqrt(X[:, 2]) * 10.0, (X[:, 3] - X[:, 4]) // 100])
    return X, y


def raster():
    rng = np.random.default_rng(32)
    X, _ = reference_rows()
    px = X[rng.integers(0, len(X), size=N)] + rng.integers(-40, 41, size=(N, 6))
    px[::9] += rng.integers(300, 3000, size=(len(px[::9]), 6))
    px[5::17] = X[rng.integers(0, len(X), size=len(px[5::17]))]
    px = px.astype(np.int16)
    px[3::13, 2] = NODATA
    return px


def weights_of(name):
    from sknnr_amd import weights as W

    return W.InverseDistance(1.0) if name == "law" else name


def restated(y, idx, dist, name, k=K, fill=-1, ids=None, **kw):
    i64, d64, _, _ = RP.decode(idx, dist, k, 300, fill, ids)
    w = weights_of(name)
    return RP.reduce(y, i64, d64, "uniform" if name == "law" else name, weight_fn=w if name == "law" else None, **kw)


@pytest.fixture(scope="module", params=WEIGHTS)
def stored(request):
    """An estimator per weight kind, the raster, and what ONE search call stored and returned: float64 distances, int64
    row positions, float64 predictions.  Computed once, never changed."""
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    X, y = reference_rows()
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights_of(request.param)).fit(X, y)
    px = raster()
    dist, idx = np.empty((N, K)), np.empty((N, K), dtype=np.int64)
    pred, _, _ = est.predict_chunks(iter(cut(px)), return_neighbors=True, neighbors_out=(dist, idx), nodata=NODATA)
    for a in (dist, idx, pred):
        a.setflags(write=False)
    assert (idx[3::13] == -1).all() and np.isnan(dist[3::13]).all() and np.isnan(pred[3::13]).all()
    return request.param, est, px, dist, idx, pred


def pairs(dist, idx, axis=0):
    return list(zip(cut(dist, axis), cut(idx, axis)))


def test_round_trip_rows(stored):
    name, est, px, dist, idx, pred = stored
    searches = est.engine_._index.stats()["queries"]
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)))
    assert got.tobytes() == pred.tobytes() and got.shape == (N, 3)
    assert est.replay_unknown_ == 0
    assert est.engine_._index.stats()["queries"] == searches, "a replay searched"
    rec = est.engine_._index.debug_last_replay()
    assert rec["search_launches"] == 0 and rec["pixels"] == 1300 and rec["masked"] == int(np.isnan(dist[701:, 0]).sum())
    # the restatement on the stored values
    np.testing.assert_array_equal(got, restated(est._y, idx, dist, name))
    # one tile through the same path, and into a caller's array
    one = est.predict_neighbors(idx[:700], dist[:700])
    assert one.tobytes() == pred[:700].tobytes()
    out = np.full((N + 5, 3), 7.0)
    back = est.predict_neighbors_chunks(iter(pairs(dist, idx)), out=out)
    assert back.tobytes() == pred.tobytes() and np.shares_memory(back, out) and (out[N:] == 7.0).all()
    if name == "uniform":  # no distances needed
        assert est.predict_neighbors_chunks(iter(cut(idx))).tobytes() == pred.tobytes()


def test_round_trip_bands(stored):
    name, est, px, dist, idx, pred = stored
    bands = np.ascontiguousarray(px.T)
    bd, bi, bp = np.empty((K, N)), np.empty((K, N), dtype=np.int64), np.empty((3, N))
    est.predict_chunks(iter(cut(bands, 1)), out=bp, layout="bands", return_neighbors=True, neighbors_out=(bd, bi), nodata=NODATA)
    np.testing.assert_array_equal(bp.T, pred)
    got = est.predict_neighbors_chunks(iter(pairs(bd, bi, 1)), layout="bands")
    assert got.shape == (3, N) and got.tobytes() == bp.tobytes()
    # (ks, h, w) windows, and rows stored / bands replayed: the layout is the tile's, not the raster's
    first = (bd[:, :700].reshape(K, 20, 35), bi[:, :700].reshape(K, 20, 35))
    assert est.predict_neighbors_chunks([first], layout="bands").tobytes() == np.ascontiguousarray(bp[:, :700]).tobytes()


def test_round_trip_statistics_and_plans(stored):
    name, est, px, dist, idx, pred = stored
    stat = ["mean", "mean", "mode"]
    want = est.predict_chunks(iter(cut(px)), nodata=NODATA, statistic=stat)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), statistic=stat)
    assert got.tobytes() == want.tobytes()
    outputs = [(0, "mean"), (0, ("quantile", 0.1)), (0, ("quantile", 0.9)), (2, "mode"), (1, "median")]
    want = est.predict_chunks(iter(cut(px)), nodata=NODATA, outputs=outputs)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), outputs=outputs)
    assert got.shape == (N, 5) and got.tobytes() == want.tobytes()
    np.testing.assert_array_equal(got, restated(est._y, idx, dist, name, outputs=outputs))


def test_round_trip_typed_outputs(stored):
    name, est, px, dist, idx, pred = stored
    kw = dict(out_dtype=np.int16, scale=[0.1, 10.0, 1.0], offset=[0.0, -500.0, 3.0], out_nodata=-9999)
    want = est.predict_chunks(iter(cut(px)), nodata=NODATA, **kw)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), **kw)
    assert got.dtype == np.int16 and got.tobytes() == want.tobytes()
    assert (got[3::13] == -9999).all()
    want32 = est.predict_chunks(iter(cut(px)), nodata=NODATA, out_dtype=np.float32)
    assert est.predict_neighbors_chunks(iter(pairs(dist, idx)), out_dtype=np.float32).tobytes() == want32.tobytes()


def test_round_trip_usage_zonal_domain(stored):
    import sknnr_amd

    name, est, px, dist, idx, pred = stored
    zones = ((np.arange(N) // 61) % N_ZONES).astype(np.int32)
    kw = dict(out_dtype=np.int16, scale=0.1, out_nodata=-9999)
    u0, z0, d0 = sknnr_amd.NeighborUsage(), sknnr_amd.ZonalStats(N_ZONES, classes={2: 16}), est.distance_domain(p=0.05)
    p0 = np.zeros(N, dtype=np.uint8)
    want = est.predict_chunks(iter(cut(px)), nodata=NODATA, usage=u0, zones=iter(cut(zones)), zonal=z0, domain=d0,
                              domain_out=p0, **kw)
    u1, z1, d1 = sknnr_amd.NeighborUsage(), sknnr_amd.ZonalStats(N_ZONES, classes={2: 16}), est.distance_domain(p=0.05)
    p1 = np.zeros(N, dtype=np.uint8)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), usage=u1, zones=iter(cut(zones)), zonal=z1, domain=d1,
                                       domain_out=p1, **kw)
    assert got.tobytes() == want.tobytes()
    assert u1 == u0 and z1 == z0 and d1 == d0
    np.testing.assert_array_equal(p1, p0)
    assert (p1[3::13] == 255).all() and d1.n_nodata == len(p1[3::13])
    # beyond="nodata": the same blanked pixels, the same tables
    z2, d2 = sknnr_amd.ZonalStats(N_ZONES, classes={2: 16}), est.distance_domain(p=0.05)
    want = est.predict_chunks(iter(cut(px)), nodata=NODATA, zones=iter(cut(zones)), zonal=z2, domain=d2, beyond="nodata", **kw)
    z3, d3 = sknnr_amd.ZonalStats(N_ZONES, classes={2: 16}), est.distance_domain(p=0.05)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), zones=iter(cut(zones)), zonal=z3, domain=d3, beyond="nodata", **kw)
    assert got.tobytes() == want.tobytes() and z3 == z2 and d3 == d2 and d3.n_beyond > 0
    assert not (z3 == z1)


def test_narrow_storage_with_dataframe_ids(stored):
    import pandas as pd

    import sknnr_amd

    name, est, px, dist, idx, pred = stored
    X, y = reference_rows()
    ids = np.random.default_rng(5).permutation(np.concatenate([np.arange(250) * 7 + 1000, -5 - 3 * np.arange(50)]))
    frame = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights_of(name)).fit(pd.DataFrame(X, index=ids), y)
    d32, i32 = np.empty((N, K), dtype=np.float32), np.empty((N, K), dtype=np.int32)
    want, _, _ = frame.predict_chunks(iter(cut(px)), return_neighbors=True, return_dataframe_index=True, index_dtype=np.int32,
                                      distance_dtype=np.float32, neighbors_out=(d32, i32), nodata=NODATA)
    assert (i32[3::13] == -1).all() and set(np.unique(i32[i32 != -1])) <= set(ids)
    got = frame.predict_neighbors_chunks(iter(pairs(d32, i32)), ids=True)
    np.testing.assert_array_equal(got, restated(y, i32, d32, name, ids=ids))
    assert frame.engine_._index.debug_last_replay()["skeleton"] == 1
    if name == "uniform":
        assert got.tobytes() == want.tobytes()
        assert frame.predict_neighbors_chunks(iter(cut(i32)), ids=True).tobytes() == want.tobytes()
    else:
        # The weights come from the float32 distances as widened: each d moves by at most 2^-24 of itself, so does each
        # weight (1 / d and 1 / (1 + d) alike), and a normalised weighted mean of values bounded by Y moves by at most
        # 2 * 2^-24 * Y (numerator and denominator each by 2^-24); twice that covers the roundings of the sums.
        for j in range(3):
            np.testing.assert_allclose(got[:, j], want[:, j], rtol=0, atol=4 * 2.0**-24 * np.abs(y[:, j]).max(), equal_nan=True)


def test_an_attribute_table_the_estimator_was_never_fitted_with(stored):
    import pandas as pd

    import sknnr_amd

    name, est, px, dist, idx, pred = stored
    X, y = reference_rows()
    rng = np.random.default_rng(8)
    y2 = np.column_stack([y[:, 1] * 3.0, rng.standard_normal(300), rng.integers(0, 9, size=300), X[:, 5]])
    fresh = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights_of(name)).fit(X, y2)
    want = fresh.predict_chunks(iter(cut(px)), nodata=NODATA)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), y=y2)
    assert got.shape == (N, 4) and got.tobytes() == want.tobytes()
    assert est._replay_targets[0] is y2
    held = est._replay_targets[1]
    outputs = [(3, "max"), (2, "mode"), (0, ("quantile", 0.5))]
    want = fresh.predict_chunks(iter(cut(px)), nodata=NODATA, outputs=outputs, out_dtype=np.int32, out_nodata=-1)
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), y=y2, outputs=outputs, out_dtype=np.int32, out_nodata=-1)
    assert got.tobytes() == want.tobytes() and est._replay_targets[1] is held  # (cached by the table's identity)
    frame = pd.DataFrame(y2, columns=list("abcd"))
    assert est.predict_neighbors_chunks(iter(pairs(dist, idx)), y=frame).tobytes() == fresh.predict_chunks(
        iter(cut(px)), nodata=NODATA).tobytes()
    one = est.predict_neighbors_chunks(iter(pairs(dist, idx)), y=y2[:, 1])
    assert one.shape == (N,) and one.tobytes() == np.ascontiguousarray(
        fresh.predict_chunks(iter(cut(px)), nodata=NODATA)[:, 1]).tobytes()
    # the estimator's own targets are untouched
    assert est.predict_neighbors_chunks(iter(pairs(dist, idx))).tobytes() == pred.tobytes()


def test_the_leading_columns_of_a_wider_store(stored):
    name, est, px, dist, idx, pred = stored
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)), n_neighbors=2)
    np.testing.assert_array_equal(got, restated(est._y, idx, dist, name, k=2))
    assert est.engine_._index.debug_last_replay()["k"] == 2 and est.engine_._index.debug_last_replay()["ks"] == K


def test_unknown_values_raise_or_become_nodata(stored):
    name, est, px, dist, idx, pred = stored
    bad = idx.copy()
    bad[901, 4] = -7
    with pytest.raises(ValueError, match=r"^1 pixels hold stored neighbours that name no reference row.*tile 3\."):
        est.predict_neighbors_chunks(iter(pairs(dist, bad)))
    assert est.replay_unknown_ == 1
    bad[5, 0] = 300
    bad[6, 2] = 10**9
    with pytest.raises(ValueError, match=r"^3 pixels hold.*tile 0\."):
        est.predict_neighbors_chunks(iter(pairs(dist, bad)))
    kw = dict(out_dtype=np.int16, scale=0.1, out_nodata=-9999)
    base = est.predict_neighbors_chunks(iter(pairs(dist, idx)), **kw)
    got = est.predict_neighbors_chunks(iter(pairs(dist, bad)), unknown="nodata", **kw)
    rows = np.zeros(N, dtype=bool)
    rows[[5, 6, 901]] = True
    assert est.replay_unknown_ == 3 and (base[rows] != -9999).all()
    np.testing.assert_array_equal(got[rows], np.full((3, 3), -9999))
    np.testing.assert_array_equal(got[~rows], base[~rows])
    floats = est.predict_neighbors_chunks(iter(pairs(dist, bad)), unknown="nodata")
    np.testing.assert_array_equal(np.isnan(floats).all(axis=1), rows | np.isnan(dist[:, 0]))
    np.testing.assert_array_equal(floats[~rows], pred[~rows])
    with pytest.raises(ValueError, match="out_nodata is required"):
        est.predict_neighbors_chunks(iter(pairs(dist, bad)), unknown="nodata", out_dtype=np.int16)


def test_search_entries_refuse_an_attribute_only_handle():
    from sknnr_amd import _native

    assert _native.device_count() >= 1
    _, y = reference_rows()
    ix = _native.TargetIndex(y)
    try:
        with pytest.raises(_native.HipBackendError, match="holds a target table only") as err:
            ix.kneighbors_host(np.zeros((4, 6)), ix.make_opts(K))
        assert err.value.code == _native.ERR_INVALID
        with pytest.raises(_native.HipBackendError, match="holds a target table only") as err:
            ix.open_stream(ix.make_opts(K))
        assert err.value.code == _native.ERR_INVALID
        with pytest.raises(_native.HipBackendError, match="sknnr_index_set_groups"):
            ix.set_groups(np.zeros(300, dtype=np.int32))
        # the from-neighbours entries accept it
        idx = np.random.default_rng(0).integers(0, 300, size=(50, K))
        got = ix.predict_from_neighbors_host(None, idx, None, _native.WEIGHTS_UNIFORM)
        np.testing.assert_array_equal(got, RP.reduce(y, idx.astype(np.int64), None, "uniform"))
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["gnn", "rfnn"])
def test_transformed_estimators_round_trip(kind):
    import sknnr_amd

    X, y = reference_rows()
    px = raster().astype(np.float64)
    if kind == "gnn":
        est = sknnr_amd.GNNRegressor(n_neighbors=K, weights="distance").fit(X, y)
    else:
        est = sknnr_amd.RFNNRegressor(n_neighbors=K, n_estimators=5, random_state=0).fit(X, y)
    dist, idx = np.empty((N, K)), np.empty((N, K), dtype=np.int64)
    want, _, _ = est.predict_chunks(iter(cut(px)), return_neighbors=True, neighbors_out=(dist, idx))
    got = est.predict_neighbors_chunks(iter(pairs(dist, idx)))
    assert got.tobytes() == want.tobytes() and est.replay_unknown_ == 0
    assert est.predict_neighbors(idx[:9], dist[:9]).tobytes() == want[:9].tobytes()
