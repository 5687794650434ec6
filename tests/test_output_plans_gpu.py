"""Output plans end to end: ``summarize(X, outputs=plan)`` and ``predict_chunks(tiles, outputs=plan)``.

The yardstick of a one-shot call is the numpy restatement (tests/_output_plans.py) applied to the SAME estimator's
``kneighbors(X)`` and its fitted targets; the yardstick of a streamed call is ``summarize(np.concatenate(tiles),
outputs=plan)``, through the typed-output restatement (tests/_narrow.py) where the call asks for a narrow type.  Every
comparison is ``assert_array_equal`` (NaN positions equal).  Raw fits: the 1,500 rows of a 4-D integer lattice of
test_neighbor_summary_gpu.py (exact distance ties and zero distances), k = 5, queries in tiles of {1, 255, 256, 257, 1000}
rows, a fifth of them outside the box of the lattice -- beyond the bandwidth of the compact law ``Triangular(1.5)``, whose
weights all vanish there (every reference row has another within sqrt(2), so the fit's own independent score is defined);
GNN and RFNN: moscow.

Without the feature every test here fails with ``TypeError`` (no ``outputs``) or ``AttributeError`` (no
``debug_last_plan``)."""

from __future__ import annotations

import numpy as np
import pytest

import _narrow as NR
import _neighbor_stats as NS
import _output_plans as OP

pytestmark = pytest.mark.gpu

N_REF, D, K = 1500, 4, 5
SIZES = (1, 255, 256, 257, 1000)
NODATA = -9999.0
PLAN = [(0, "mean"), (0, "std"), (0, ("quantile", 0.1)), (0, ("quantile", 0.9)), (1, "mode"), (2, "median"), (1, "nearest"),
        (2, "mean"), (0, "min"), (2, ("quantile", 1.0)), (0, "max")]
PLANS = [PLAN, [(1, ("quantile", 0.5))], [(2, "std"), (2, ("quantile", 0.0)), (1, "mode")], [(j, "mean") for j in range(3)]]


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
        if n > 1:  # a fifth of the rows lie outside the box, at least 3 from every reference row in every coordinate
            q[rng.random(n) < 0.2] += 8.0
        if masked:
            rows = np.flatnonzero(rng.random(n) < 0.25) if n > 1 else np.array([0])
            q[rows, rng.integers(0, D, size=rows.size)] = NODATA
        tiles.append(q)
    return tiles


def as_bands(tiles):
    return [np.ascontiguousarray(t.T) for t in tiles]


def weights_of(name):
    from sknnr_amd import weights as W

    return {"uniform": "uniform", "distance": "distance", "inverse": W.InverseDistance(), "triangular": W.Triangular(1.5),
            "callable": yaimpute}[name]


@pytest.fixture(scope="module")
def E():
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    made = {}

    def get(name="uniform", y_cols=(0, 1, 2), y_dtype=np.float64):
        key = (name, y_cols, np.dtype(y_dtype))
        if key not in made:
            x, y = lattice()
            yy = y[:, y_cols[0]] if len(y_cols) == 1 else y[:, list(y_cols)]
            made[key] = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights_of(name)).fit(x, yy.astype(y_dtype))
        return made[key]

    return get


def restate(est, X, plan, reg=None):
    """The restatement on the estimator's own neighbours of ``X`` (None: of its fitted rows)."""
    reg = est if reg is None else reg
    dist, idx = est.kneighbors(X)
    y = reg._y.reshape(len(reg._y), -1)
    weights = "uniform" if reg.weights is None else reg.weights
    w, mode = None, weights
    if callable(weights):
        w, mode = np.asarray(weights(dist), dtype=np.float64), "explicit"
    return OP.plan_of(y, dist, idx, w, mode, plan)


def plan_record(est):
    return getattr(est, "regressor_", est).engine_._index.debug_last_plan()


@pytest.mark.parametrize("name", ["uniform", "distance", "inverse", "triangular", "callable"])
def test_one_shot(E, name):
    import torch

    est = E(name)
    X = np.concatenate(make_tiles())
    for plan in PLANS:
        want = restate(est, X, plan)
        got = est.summarize(X, outputs=plan)
        assert got.dtype == np.float64 and got.shape == (len(X), len(plan))
        np.testing.assert_array_equal(got, want, err_msg=str(plan))
        rec = plan_record(est)
        n_mean = sum(s == "mean" for _, s in plan)
        assert rec["ran"] == 1 and rec["path"] == 1 and rec["n_out"] == len(plan) and rec["k"] == K, rec
        assert rec["n_mean"] == n_mean and rec["predict_ran"] == int(n_mean > 0), rec
    if name == "triangular":  # some rows have no neighbour inside the bandwidth: NaN in every weighted plane
        gone = np.isnan(got[:, 0])
        assert 0 < gone.sum() < len(X)
    np.testing.assert_array_equal(est.summarize(None, outputs=PLAN), restate(est, None, PLAN))
    # per old-statistic entry: the matching column of summarize(X, statistic=...), bit for bit
    got = est.summarize(X, outputs=PLAN)
    for e, (j, s) in enumerate(PLAN):
        if isinstance(s, str) and s in NS.CODES:
            np.testing.assert_array_equal(got[:, e], est.summarize(X, statistic=s)[:, j], err_msg=f"{e} {s}")
    assert plan_record(est)["ran"] == 0
    # CUDA tensors in, CUDA tensors out
    dev = est.summarize(torch.as_tensor(X, device="cuda"), outputs=PLAN)
    assert dev.is_cuda and dev.dtype == torch.float64
    np.testing.assert_array_equal(dev.cpu().numpy(), got)


@pytest.mark.parametrize("name", ["uniform", "distance"])
def test_float32_targets_and_one_dimensional_y(E, name):
    X = np.concatenate(make_tiles())
    est = E(name, (0, 1, 2), np.float32)
    plan = [(2, "mean"), (0, ("quantile", 0.25)), (0, "mean"), (1, "std")]
    got = est.summarize(X, outputs=plan)
    np.testing.assert_array_equal(got, restate(est, X, plan))
    mean = est.summarize(X, statistic="mean")
    np.testing.assert_array_equal(got[:, [0, 2]], mean[:, [2, 0]])
    np.testing.assert_array_equal(got[:, [0, 2]], est.predict(X)[:, [2, 0]].astype(np.float64))
    # a 1-D y: outputs is always 2-D, statistic keeps its shape
    est = E(name, (0,))
    plan = [(0, "median"), (0, "mean")]
    got = est.summarize(X, outputs=plan)
    assert got.shape == (len(X), 2)
    np.testing.assert_array_equal(got, restate(est, X, plan))
    flat = est.summarize(X, statistic=("quantile", 0.5))
    assert flat.shape == (len(X),)
    np.testing.assert_array_equal(flat, got[:, 0])
    np.testing.assert_array_equal(est.predict_chunks(iter(make_tiles()), statistic=[("quantile", 0.5)]), flat)
    np.testing.assert_array_equal(est.predict_chunks(iter(make_tiles()), outputs=plan), got)


@pytest.mark.parametrize("name", ["uniform", "distance", "triangular"])
def test_streamed_equals_one_shot(E, name):
    est = E(name)
    tiles = make_tiles()
    X = np.concatenate(tiles)
    n_out = len(PLAN)
    want = est.summarize(X, outputs=PLAN)
    got = est.predict_chunks(iter(tiles), outputs=PLAN)
    assert got.dtype == np.float64 and got.shape == (len(X), n_out)
    np.testing.assert_array_equal(got, want)
    rec = plan_record(est)
    assert rec["ran"] == 1 and rec["path"] == 1 and rec["rows"] == SIZES[-1] and rec["n_out"] == n_out, rec
    for plan in PLANS[1:]:
        np.testing.assert_array_equal(est.predict_chunks(iter(tiles), outputs=plan), est.summarize(X, outputs=plan))
    # out= alone, layout="bands" with out
    out = np.full(want.shape, 77.0)
    ret = est.predict_chunks(iter(tiles), out=out, outputs=PLAN)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(ret, want)
    np.testing.assert_array_equal(est.predict_chunks(iter(as_bands(tiles)), layout="bands", outputs=PLAN), want.T)
    out = np.full((n_out, len(X)), 77.0)
    est.predict_chunks(iter(as_bands(tiles)), layout="bands", out=out, outputs=PLAN)
    np.testing.assert_array_equal(out, want.T)
    # nodata alone: masked rows NaN across all n_out planes
    mtiles = make_tiles(masked=True)
    MX = np.concatenate(mtiles)
    valid = ~(MX == NODATA).any(axis=1)
    assert 0 < valid.sum() < len(MX) and not valid[0]
    mwant = np.full((len(MX), n_out), np.nan)
    mwant[valid] = est.summarize(MX[valid], outputs=PLAN)
    got = est.predict_chunks(iter(mtiles), nodata=NODATA, outputs=PLAN)
    np.testing.assert_array_equal(got, mwant)
    assert np.isnan(got[~valid]).all()
    # all together, as the stored raster: band-first, masked, into a caller's int16 array, one scale per output plane
    scale = np.array([10.0, 1.0, 5.0, 2.0, 1.0, 0.5, 3.0, 7.0, 1.0, 4.0, 6.0])
    offset = np.linspace(-3.0, 2.0, n_out)
    typed = NR.narrow_values(mwant, np.int16, scale, offset, -32768)
    out = np.zeros((n_out, len(MX)), dtype=np.int16)
    est.predict_chunks(iter(as_bands(mtiles)), out=out, nodata=NODATA, layout="bands", out_dtype=np.int16, scale=scale,
                       offset=offset, out_nodata=-32768, outputs=PLAN)
    np.testing.assert_array_equal(out, typed.T)
    assert (out[:, ~valid] == -32768).all()
    # a scalar scale, row layout
    got = est.predict_chunks(iter(mtiles), nodata=NODATA, out_dtype=np.int16, scale=2.0, out_nodata=-1, outputs=PLAN)
    np.testing.assert_array_equal(got, NR.narrow_values(mwant, np.int16, np.full(n_out, 2.0), np.zeros(n_out), -1))


def test_streamed_with_neighbours_and_dataframe_ids():
    import pandas as pd
    import sknnr_amd

    x, y = lattice()
    ids = np.arange(N_REF, dtype=np.int64) * 7 + 100_000
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(pd.DataFrame(x, index=ids), y)
    tiles = make_tiles()
    want = est.predict_chunks(iter(tiles), outputs=PLAN)
    dist, idx = est.kneighbors_chunks(iter(tiles), return_dataframe_index=True)
    pred, got_d, got_i = est.predict_chunks(iter(tiles), outputs=PLAN, return_neighbors=True, return_dataframe_index=True)
    np.testing.assert_array_equal(pred, want)
    np.testing.assert_array_equal(got_d, dist)
    np.testing.assert_array_equal(got_i, idx)
    assert np.isin(got_i, ids).all()


def test_statistic_with_a_quantile_is_the_per_target_plan(E):
    est = E("distance")
    tiles = make_tiles()
    X = np.concatenate(tiles)
    stat = ["mean", ("quantile", 0.9), "mode"]
    plan = [(0, "mean"), (1, ("quantile", 0.9)), (2, "mode")]
    want = est.summarize(X, outputs=plan)
    np.testing.assert_array_equal(est.summarize(X, statistic=stat), want)
    np.testing.assert_array_equal(est.predict_chunks(iter(tiles), statistic=stat), want)
    np.testing.assert_array_equal(est.summarize(X, statistic=("quantile", 0.5)),
                                  est.summarize(X, outputs=[(j, "median") for j in range(3)]))


def test_the_old_path_is_unchanged(E):
    """An old-names-only ``statistic`` call enqueues what it did: the summary record of the parent commit, no plan kernel."""
    est = E("uniform")
    tiles = make_tiles()
    ix = est.engine_._index
    est.predict_chunks(iter(tiles), outputs=PLAN)
    assert ix.debug_last_plan()["ran"] == 1
    est.predict_chunks(iter(tiles), statistic=["mode", "mean", "std"])
    assert ix.debug_last_summary() == dict(path=1, rows=SIZES[-1], cols=2, k=K, predict_ran=1, t=3, weight_mode=0, reserved=0)
    assert ix.debug_last_plan() == dict.fromkeys(ix.PLAN_FIELDS, 0)
    est.summarize(np.concatenate(tiles), statistic="min")
    rec = ix.debug_last_summary()
    assert rec["path"] == 1 and rec["cols"] == 3 and rec["predict_ran"] == 0 and ix.debug_last_plan()["ran"] == 0
    est.predict_chunks(iter(tiles))
    rec = ix.debug_last_summary()
    assert rec["path"] == 0 and rec["predict_ran"] == 1 and ix.debug_last_plan()["ran"] == 0


def test_uniform_quantile_ends_are_min_and_max(E):
    est = E("uniform")
    X = np.concatenate(make_tiles())
    plan = [(j, s) for j in range(3) for s in (("quantile", 0.0), "min", ("quantile", 1.0), "max")]
    got = est.summarize(X, outputs=plan)
    np.testing.assert_array_equal(got[:, 0::4], got[:, 1::4])
    np.testing.assert_array_equal(got[:, 2::4], got[:, 3::4])


def test_refusals(E):
    est = E("callable")
    tiles = make_tiles()
    np.testing.assert_array_equal(est.predict_chunks(iter(tiles), outputs=PLAN),
                                  est.summarize(np.concatenate(tiles), outputs=PLAN))
    for kwargs, feed, msg in ((dict(nodata=NODATA), tiles, "nodata is not supported with callable weights"),
                              (dict(layout="bands"), as_bands(tiles), "layout='bands' is not supported with callable weights"),
                              (dict(out_dtype=np.float32), tiles, "typed outputs are not supported with callable weights")):
        with pytest.raises(NotImplementedError, match=msg):
            est.predict_chunks(iter(feed), outputs=PLAN, **kwargs)
    est = E("uniform")
    with pytest.raises(ValueError, match="cannot be given together"):
        est.summarize(tiles[1], outputs=PLAN, statistic="mean")
    with pytest.raises(ValueError, match="outside"):
        est.predict_chunks(iter(tiles), outputs=[(3, "mean")])


def test_tree_tie_policy():
    import sknnr_amd

    x, y = lattice()
    tiles = make_tiles()
    X = np.concatenate(tiles)
    with sknnr_amd.tree_tie_policy("tree"):
        est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="kd_tree", weights="distance").fit(x, y)
        want = restate(est, X, PLAN)
        np.testing.assert_array_equal(est.summarize(X, outputs=PLAN), want)
        np.testing.assert_array_equal(est.predict_chunks(iter(tiles), outputs=PLAN), want)
        for kwargs, feed, msg in ((dict(nodata=NODATA), tiles, "nodata is not supported under tree_tie_policy"),
                                  (dict(layout="bands"), as_bands(tiles), "layout='bands' is not supported under tree_tie_policy"),
                                  (dict(out_dtype=np.float32), tiles, "typed outputs are not supported under tree_tie_policy")):
            with pytest.raises(NotImplementedError, match=msg):
                est.predict_chunks(iter(feed), outputs=PLAN, **kwargs)


@pytest.mark.parametrize("kind", ["gnn", "rfnn"])
def test_transformed_estimators(moscow, kind):
    import sknnr_amd

    X, y = moscow["X_train"], moscow["y_train"]
    Xq = np.concatenate([moscow["X_test"], moscow["X_train"][:40]])
    if kind == "gnn":
        est = sknnr_amd.GNNRegressor(n_neighbors=5, weights="distance").fit(X, y)
    else:
        est = sknnr_amd.RFNNRegressor(n_neighbors=4, n_estimators=20, random_state=0).fit(X, y)
    t = y.shape[1]
    plan = [(t - 1, "mean"), (0, ("quantile", 0.1)), (0, "median"), (0, ("quantile", 0.9)), (1, "std"), (t - 1, "mode")]
    want = restate(est, Xq, plan, reg=est.regressor_)
    got = est.summarize(Xq, outputs=plan)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(est.summarize(None, outputs=plan), restate(est, None, plan, reg=est.regressor_))
    np.testing.assert_array_equal(got[:, 0], np.asarray(est.predict(Xq), dtype=np.float64)[:, t - 1])
    pieces = [Xq[:1], Xq[1:30], Xq[30:]]
    np.testing.assert_array_equal(est.predict_chunks(iter(pieces), outputs=plan), got)
