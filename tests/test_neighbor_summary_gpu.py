"""Per-target neighbour summaries end to end: ``summarize(X, statistic)`` and ``predict_chunks(tiles, statistic=...)``.

The yardstick of a one-shot call is the numpy restatement (tests/_neighbor_stats.py) applied to the SAME estimator's
``kneighbors(X)`` and its fitted targets; the yardstick of a streamed call is ``summarize(np.concatenate(tiles), s)``, through
the typed-output restatement (tests/_narrow.py) where the call asks for a narrow type.  Every comparison is
``assert_array_equal`` (NaN positions equal).  Raw / Euclidean fits: 1,500 rows of a 4-D integer lattice (exact distance
ties and zero distances), queries in tiles of {1, 255, 256, 257, 1000} rows; GNN and RFNN: moscow.

Without the feature every test here fails with ``AttributeError`` / ``TypeError`` (no ``summarize``, no ``statistic``).
"""

from __future__ import annotations

import numpy as np
import pytest

import _narrow as NR
import _neighbor_stats as NS

pytestmark = pytest.mark.gpu

N_REF, D, K = 1500, 4, 5
SIZES = (1, 255, 256, 257, 1000)
NODATA = -9999.0
TABLES = [("mean", "mode", "std"), ("min", "max", "nearest"), ("mode", "mean", "mean"), ("std", "nearest", "mode")]


def yaimpute(d):
    return 1.0 / (1.0 + d)


def lattice(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 6, size=(N_REF, D)).astype(np.float64)
    y = np.stack([rng.standard_normal(N_REF) * 50.0 + 100.0, rng.integers(0, 5, size=N_REF) * 40.0 + 3.0,
                  rng.random(N_REF) * 200.0], axis=1)
    return x, y


def make_tiles(masked=False, seed=1):
    rng = np.random.default_rng(seed)
    tiles = []
    for n in SIZES:
        q = rng.integers(0, 6, size=(n, D)).astype(np.float64)
        if masked:
            rows = np.flatnonzero(rng.random(n) < 0.25) if n > 1 else np.array([0])
            q[rows, rng.integers(0, D, size=rows.size)] = NODATA
        tiles.append(q)
    return tiles


@pytest.fixture(scope="module")
def E():
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    made = {}

    def get(weights="uniform", y_cols=(0, 1, 2), y_dtype=np.float64):
        key = (weights if not callable(weights) else "callable", y_cols, np.dtype(y_dtype))
        if key not in made:
            x, y = lattice()
            yy = y[:, y_cols[0]] if y_cols == (0,) or y_cols == (1,) else y[:, list(y_cols)]
            made[key] = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights).fit(x, yy.astype(y_dtype))
        return made[key]

    return get


def restate(est, X, table, reg=None):
    """The restatement on the estimator's own neighbours of ``X`` (None: of its fitted rows)."""
    reg = est if reg is None else reg
    dist, idx = est.kneighbors(X)
    y = reg._y.reshape(len(reg._y), -1)
    weights = "uniform" if reg.weights is None else reg.weights
    w, mode = None, weights
    if callable(weights):
        w, mode = weights(dist), "explicit"
    with np.errstate(all="ignore"):
        return NS.summarize(y, dist, idx, w, mode, list(table))


@pytest.mark.parametrize("weights", ["uniform", "distance", yaimpute])
def test_one_shot_every_statistic(E, weights):
    import torch

    est = E(weights)
    X = np.concatenate(make_tiles())
    for table in TABLES + [(s,) * 3 for s in NS.STATISTICS]:
        want = restate(est, X, table)
        got = est.summarize(X, list(table))
        assert got.dtype == np.float64 and got.shape == (len(X), 3)
        np.testing.assert_array_equal(got, want, err_msg=str(table))
    single = est.summarize(X, "std")
    np.testing.assert_array_equal(single, restate(est, X, ("std",) * 3))
    # X=None: every fitted row from its neighbours, itself excluded
    table = TABLES[0]
    np.testing.assert_array_equal(est.summarize(None, list(table)), restate(est, None, table))
    np.testing.assert_array_equal(est.summarize(statistic="mode"), restate(est, None, ("mode",) * 3))
    # CUDA tensors in, CUDA tensors out
    got = est.summarize(torch.as_tensor(X, device="cuda"), list(TABLES[3]))
    assert got.is_cuda and got.dtype == torch.float64
    np.testing.assert_array_equal(got.cpu().numpy(), restate(est, X, TABLES[3]))
    # the usage guide's two-estimator case: one mixed call equals the single-statistic calls column by column
    mixed = est.summarize(X, ["mean", "mode", "mean"])
    np.testing.assert_array_equal(mixed[:, [0, 2]], est.summarize(X, "mean")[:, [0, 2]])
    np.testing.assert_array_equal(mixed[:, 1], est.summarize(X, "mode")[:, 1])


@pytest.mark.parametrize("weights", ["uniform", "distance", yaimpute])
def test_mean_is_predict_and_nearest_is_the_first_neighbour(E, weights):
    X = np.concatenate(make_tiles())
    for y_cols, y_dtype in (((0, 1, 2), np.float64), ((0, 1, 2), np.float32), ((0,), np.float64), ((0,), np.float32)):
        est = E(weights, y_cols, y_dtype)
        pred = est.predict(X)
        got = est.summarize(X, "mean")
        assert got.dtype == np.float64 and got.shape == pred.shape
        np.testing.assert_array_equal(got, pred)
        np.testing.assert_array_equal(est.summarize(None, "mean"), est.predict(None))
        idx = est.kneighbors(X, return_distance=False)
        np.testing.assert_array_equal(est.summarize(X, "nearest"), est._y[idx[:, 0]].astype(np.float64))


def test_one_dimensional_y(E):
    est = E("distance", (1,))
    X = np.concatenate(make_tiles())
    for s in NS.STATISTICS:
        got = est.summarize(X, s)
        assert got.shape == (len(X),)
        np.testing.assert_array_equal(got, restate(est, X, (s,))[:, 0], err_msg=s)
        np.testing.assert_array_equal(est.predict_chunks(iter(make_tiles()), statistic=[s]), got, err_msg=s)


@pytest.mark.parametrize("k", [9, 17])
def test_std_around_the_sequential_mean(k):
    """Uniform weights, t >= 2, k >= 8 on continuous targets: ``std`` is taken around the mean whose k values are added in
    order (``predict``'s), which differs from the pairwise mean in the last bits there."""
    import sknnr_amd

    x, y = lattice()
    est = sknnr_amd.RawKNNRegressor(n_neighbors=k).fit(x, y[:, [0, 2]])
    X = make_tiles()[-1]
    want = restate(est, X, ("std", "std"))
    dist, idx = est.kneighbors(X)
    v = np.ascontiguousarray(est._y[idx, 0])
    assert (np.sum(v, axis=1) / k != est.predict(X)[:, 0]).any(), "the two orders differ on these inputs"
    np.testing.assert_array_equal(est.summarize(X, "std"), want)
    np.testing.assert_array_equal(est.summarize(X, ["mean", "std"])[:, 0], est.predict(X)[:, 0])


def as_bands(tiles):
    return [np.ascontiguousarray(t.T) for t in tiles]


@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("table", TABLES)
def test_streamed_equals_one_shot(E, weights, table):
    est = E(weights)
    table = list(table)
    tiles = make_tiles()
    X = np.concatenate(tiles)
    want = est.summarize(X, table)
    got = est.predict_chunks(iter(tiles), statistic=table)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    rec = est.engine_._index.debug_last_summary()
    assert rec["path"] == 1 and rec["rows"] == SIZES[-1] and rec["cols"] == sum(s != "mean" for s in table), rec
    # layout="bands" alone, out= alone
    np.testing.assert_array_equal(est.predict_chunks(iter(as_bands(tiles)), layout="bands", statistic=table), want.T)
    out = np.full(want.shape, 77.0)
    ret = est.predict_chunks(iter(tiles), out=out, statistic=table)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(ret, want)
    # nodata alone: masked rows NaN, the others what the call on the valid rows gives
    mtiles = make_tiles(masked=True)
    MX = np.concatenate(mtiles)
    valid = ~(MX == NODATA).any(axis=1)
    assert 0 < valid.sum() < len(MX) and not valid[0]
    mwant = np.full((len(MX), 3), np.nan)
    mwant[valid] = est.summarize(MX[valid], table)
    got = est.predict_chunks(iter(mtiles), nodata=NODATA, statistic=table)
    np.testing.assert_array_equal(got, mwant)
    assert np.isnan(got[~valid]).all()
    # all together, as the stored raster: band-first, masked, into a caller's int16 array, scaled
    scale, offset = np.array([10.0, 1.0, 5.0]), np.array([0.5, 0.0, -3.0])
    typed = NR.narrow_values(mwant, np.int16, scale, offset, -32768)
    out = np.zeros((3, len(MX)), dtype=np.int16)
    est.predict_chunks(iter(as_bands(mtiles)), out=out, nodata=NODATA, layout="bands", out_dtype=np.int16, scale=scale,
                       offset=offset, out_nodata=-32768, statistic=table)
    np.testing.assert_array_equal(out, typed.T)
    assert (out[:, ~valid] == -32768).all()


def test_typed_mode_and_std(E):
    """A class-code target stored as uint8, and the spread stored as int16 with a scale."""
    est = E("distance")
    tiles = make_tiles()
    X = np.concatenate(tiles)
    y = est._y.copy()
    want = est.summarize(X, ["nearest", "mode", "min"])
    got = est.predict_chunks(iter(tiles), statistic=["nearest", "mode", "min"], out_dtype=np.uint8)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, NR.narrow_values(want, np.uint8))
    assert set(np.unique(got[:, 1])) <= set((np.arange(5) * 40 + 3).tolist()), "class codes arrive unchanged"
    want = est.summarize(X, "std")
    got = est.predict_chunks(iter(tiles), statistic="std", out_dtype=np.int16, scale=100.0)
    np.testing.assert_array_equal(got, NR.narrow_values(want, np.int16, np.full(3, 100.0), np.zeros(3)))
    np.testing.assert_array_equal(est._y, y)


def test_all_mean_table_launches_nothing_new(E):
    est = E("uniform")
    tiles = make_tiles()
    want = est.predict_chunks(iter(tiles))
    got = est.predict_chunks(iter(tiles), statistic="mean")
    np.testing.assert_array_equal(got, want)
    rec = est.engine_._index.debug_last_summary()
    assert rec["path"] == 0 and rec["cols"] == 0 and rec["predict_ran"] == 1, rec
    est.predict_chunks(iter(tiles), statistic=["mode", "min", "std"])
    rec = est.engine_._index.debug_last_summary()
    assert rec["path"] == 1 and rec["cols"] == 3 and rec["predict_ran"] == 0, rec


def test_callable_weights_stream_tile_by_tile(E):
    est = E(yaimpute)
    tiles = make_tiles()
    table = ["std", "mode", "mean"]
    np.testing.assert_array_equal(est.predict_chunks(iter(tiles), statistic=table),
                                  est.summarize(np.concatenate(tiles), table))
    with pytest.raises(NotImplementedError, match="callable weights"):
        est.predict_chunks(iter(tiles), statistic=table, nodata=NODATA)
    with pytest.raises(NotImplementedError, match="callable weights"):
        est.predict_chunks(iter(as_bands(tiles)), statistic=table, layout="bands")
    with pytest.raises(ValueError, match="negative or non-finite"):
        import sknnr_amd

        x, y = lattice()
        sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=lambda d: 1.0 - d).fit(x[:200], y[:200]).summarize(x[:50], "mode")


def test_refusals_before_device_work(E):
    est = E("uniform")
    X = np.concatenate(make_tiles())[:10]
    for bad, msg in (("median", "unknown statistic"), (["mean", "mode"], "one name per target"),
                     (["mean", 1, "mode"], "must be strings")):
        with pytest.raises(ValueError, match=msg):
            est.summarize(X, bad)
        with pytest.raises(ValueError, match=msg):
            est.predict_chunks(iter([X]), statistic=bad)


def test_stream_refusals_of_set_statistics(E):
    from sknnr_amd import _native

    est = E("uniform")
    eng = est.engine_
    X = np.concatenate(make_tiles())[:10]
    s = eng.open_stream(K, weights=None)
    try:
        with pytest.raises(_native.HipBackendError, match="opened without predictions"):
            s.set_statistics([1, 1, 1])
    finally:
        s.close()
    s = eng.open_stream(K, weights="uniform", want_dist=False)
    try:
        with pytest.raises(_native.HipBackendError, match="t = 2: the handle has 3 targets"):
            s.set_statistics([1, 1])
        with pytest.raises(_native.HipBackendError, match="is no sknnr_statistic"):
            s.set_statistics([1, 6, 0])
        s.set_statistics([1, 0, 5])
        s.set_statistics([4, 0, 5])  # (again, before a push: the last table holds)
        _, _, pred = s.push(X, need_idx=False)
        with pytest.raises(_native.HipBackendError, match="only before the first push"):
            s.set_statistics([1, 1, 1])
        s.flush()
    finally:
        s.close()
    # (the handle serves one stream or call at a time; the engine's call, with the engine stream's own search options)
    np.testing.assert_array_equal(pred, eng.summarize(X, K, "uniform", np.array([4, 0, 5], dtype=np.int32)))
    with pytest.raises(ValueError, match="statistics need a stream that predicts"):
        eng.open_stream(K, weights=None, statistic=np.array([1, 1, 1], dtype=np.int32))


def test_hamming_numpy_tie_policy():
    import sknnr_amd

    rng = np.random.default_rng(12)
    ref = rng.integers(0, 3, (400, 12)).astype(np.float64)
    q = rng.integers(0, 3, (300, 12)).astype(np.float64)
    y = np.stack([rng.standard_normal(400), rng.integers(0, 4, 400).astype(np.float64)], axis=1)
    w = rng.integers(1, 4, 12).astype(np.float64)
    table = ["std", "mode"]
    with sknnr_amd.hamming_tie_policy("numpy"):
        for weights in ("uniform", "distance"):
            est = sknnr_amd.RawKNNRegressor(n_neighbors=4, algorithm="brute", metric="hamming", metric_params={"w": w},
                                            weights=weights).fit(ref, y)
            np.testing.assert_array_equal(est.summarize(q, table), restate(est, q, table))
            np.testing.assert_array_equal(est.summarize(None, table), restate(est, None, table))
            np.testing.assert_array_equal(est.predict_chunks(iter([q[:100], q[100:]]), statistic=table),
                                          est.summarize(q, table))
            with pytest.raises(NotImplementedError, match="hamming_tie_policy"):
                est.predict_chunks(iter([q]), statistic=table, nodata=NODATA)


def test_tree_tie_policy():
    import sknnr_amd

    x, y = lattice()
    tiles = make_tiles()
    X = np.concatenate(tiles)
    table = ["mode", "mode", "std"]
    with sknnr_amd.tree_tie_policy("tree"):
        est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="kd_tree", weights="distance").fit(x, y)
        np.testing.assert_array_equal(est.summarize(X, table), restate(est, X, table))
        np.testing.assert_array_equal(est.summarize(None, table), restate(est, None, table))
        np.testing.assert_array_equal(est.predict_chunks(iter(tiles), statistic=table), est.summarize(X, table))


@pytest.mark.parametrize("kind", ["gnn", "rfnn", "euclidean"])
def test_transformed_estimators(moscow, kind):
    import sknnr_amd

    X, y = moscow["X_train"], moscow["y_train"]
    Xq = np.concatenate([moscow["X_test"], moscow["X_train"][:40]])
    if kind == "gnn":
        est = sknnr_amd.GNNRegressor(n_neighbors=5, weights="distance").fit(X, y)
    elif kind == "rfnn":
        est = sknnr_amd.RFNNRegressor(n_neighbors=4, n_estimators=20, random_state=0).fit(X, y)
    else:
        est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=3).fit(X, y)
    t = y.shape[1]
    table = [NS.STATISTICS[j % 6] for j in range(t)]
    want = restate(est, Xq, table, reg=est.regressor_)
    got = est.summarize(Xq, table)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(est.summarize(None, "mode"), restate(est, None, ("mode",) * t, reg=est.regressor_))
    np.testing.assert_array_equal(est.summarize(Xq, "mean"), np.asarray(est.predict(Xq), dtype=np.float64))
    pieces = [Xq[:1], Xq[1:30], Xq[30:]]
    np.testing.assert_array_equal(est.predict_chunks(iter(pieces), statistic=table), got)
