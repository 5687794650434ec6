"""Buffered leave-out at estimator level, on the Moscow fixture (132 training rows) with synthetic seeded plot positions:
uniform in a 10 km square, radius 1,500 m (about nine plots inside it on average).  Neighbours are compared bit for bit
with the contract's numpy model (tests/_buffer.py) on the rows the fitted regressor searches (``regressor_._fit_X``);
everything above them with the engine's own reductions on those neighbours."""

from __future__ import annotations

import numpy as np
import pytest
from sklearn.metrics import r2_score

import _buffer

pytestmark = pytest.mark.gpu

N_TRAIN = 132
GROUPS = np.arange(N_TRAIN) // 3
COORDS = np.random.default_rng(20).uniform(0.0, 10_000.0, (N_TRAIN, 2))
COORDS.setflags(write=False)
RADIUS = 1500.0
BUFFER = (COORDS, RADIUS)

ESTIMATORS = {
    "raw_default": ("RawKNNRegressor", {}),
    "raw_kd_tree": ("RawKNNRegressor", {"algorithm": "kd_tree"}),
    "euclidean": ("EuclideanKNNRegressor", {}),
    "gnn": ("GNNRegressor", {}),
    "rfnn": ("RFNNRegressor", {"n_estimators": 30, "random_state": 0}),  # 1,050 trees: swept in column chunks
}


@pytest.fixture(scope="module")
def fitted(moscow_frames):
    import sknnr_amd
    from sknnr_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    cache = {}

    def get(name, **extra):
        key = (name, tuple(sorted((k, repr(v)) for k, v in extra.items())))
        if key not in cache:
            cls, kw = ESTIMATORS[name]
            cache[key] = getattr(sknnr_amd, cls)(n_neighbors=5, **kw, **extra).fit(moscow_frames["X_train"],
                                                                                  moscow_frames["y_train"])
        return cache[key]

    return get


def searched(est):
    """``(regressor, fitted rows, formula, Hamming weights)`` of an estimator of either kind."""
    reg = getattr(est, "regressor_", est)
    formula = reg._formula()
    return reg, reg._fit_X, formula, (est.hamming_weights_ if formula == "hamming" else None)


def model(est, k, codes=None, deterministic=True, coords=COORDS, radius=RADIUS):
    reg, fit, formula, w = searched(est)
    return _buffer.buffered_kneighbors(fit, coords, radius, k, codes=codes, formula=formula, w=w, deterministic=deterministic)


def test_the_estimators_cover_the_three_formulas(fitted):
    assert [searched(fitted(n))[2] for n in ("raw_default", "raw_kd_tree", "rfnn")] == ["expanded", "direct", "hamming"]
    assert searched(fitted("rfnn"))[1].shape[1] > 1024
    counts = _buffer.excluded_counts(COORDS, RADIUS)
    assert 4.0 < counts.mean() < 14.0


@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_neighbors_equal_the_model(fitted, name):
    est = fitted(name)
    for k, det in ((None, True), (3, False), (9, True)):
        dist, idx = est.independent_kneighbors(buffer=BUFFER, n_neighbors=k, use_deterministic_ordering=det)
        want_d, want_i = model(est, 5 if k is None else k, deterministic=det)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(dist, want_d)
        assert isinstance(idx, np.ndarray)
        assert not np.take_along_axis(_buffer.excluded_mask(COORDS, RADIUS, np.arange(N_TRAIN)), idx, axis=1).any()
    only = est.independent_kneighbors(buffer=BUFFER, return_distance=False)
    np.testing.assert_array_equal(only, model(est, 5)[1])


@pytest.mark.parametrize("name", ["raw_default", "gnn", "rfnn"])
def test_groups_and_buffer_together(fitted, name):
    est = fitted(name)
    labels = np.array([f"plot{g:03d}" for g in GROUPS])
    want_d, want_i = model(est, 5, codes=GROUPS)
    for groups in (GROUPS, labels):
        dist, idx = est.independent_kneighbors(groups, buffer=BUFFER)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(dist, want_d)
    assert (want_i != model(est, 5)[1]).any()  # (the groups did remove somebody's neighbour)
    np.testing.assert_array_equal(est.buffer_counts(BUFFER, GROUPS), _buffer.excluded_counts(COORDS, RADIUS, GROUPS))
    np.testing.assert_array_equal(est.buffer_counts(BUFFER), _buffer.excluded_counts(COORDS, RADIUS))
    # a call without a buffer clears the one before it; a call without groups clears the groups
    import _groups

    reg, fit, formula, w = searched(est)
    _, idx = est.independent_kneighbors(GROUPS)
    np.testing.assert_array_equal(idx, _groups.grouped_kneighbors(fit, GROUPS, 5, formula=formula, w=w)[1])
    _, idx = est.independent_kneighbors(buffer=BUFFER)
    np.testing.assert_array_equal(idx, model(est, 5)[1])


@pytest.mark.parametrize("name", ["raw_default", "gnn"])
def test_dataframe_ids_and_a_frame_of_positions(fitted, moscow_frames, name):
    import pandas as pd

    est = fitted(name)
    reg = getattr(est, "regressor_", est)
    plots = pd.DataFrame({"X": COORDS[:, 0], "Y": COORDS[:, 1], "other": 0.0}, index=moscow_frames["X_train"].index)
    dist, idx = est.independent_kneighbors(buffer=(plots[["X", "Y"]], 1500))
    want_d, want_i = model(est, 5)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(dist, want_d)
    _, ids = est.independent_kneighbors(buffer=BUFFER, return_dataframe_index=True)
    np.testing.assert_array_equal(ids, reg.dataframe_index_in_[idx])
    assert (ids != idx).any()  # (the frame's index starts at 1: ids are not positions)
    # one column and three
    _, idx = est.independent_kneighbors(buffer=(plots["X"], 100.0))
    np.testing.assert_array_equal(idx, model(est, 5, coords=COORDS[:, :1], radius=100.0)[1])
    xyz = np.concatenate([COORDS, np.linspace(0.0, 3000.0, N_TRAIN)[:, None]], axis=1)
    _, idx = est.independent_kneighbors(buffer=(xyz, 2000.0))
    np.testing.assert_array_equal(idx, model(est, 5, coords=xyz, radius=2000.0)[1])


@pytest.mark.parametrize("name", ["raw_default", "raw_kd_tree", "euclidean", "gnn", "rfnn"])
@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_predictions_scores_and_usage(fitted, name, weights):
    est = fitted(name, weights=weights)
    reg = getattr(est, "regressor_", est)
    want_d, want_i = model(est, 5)
    pred = est.independent_predict(buffer=BUFFER)
    np.testing.assert_array_equal(pred, reg.engine_.predict_from_neighbors(want_d, want_i, weights))
    assert pred.shape == reg._y.shape
    assert est.independent_score(buffer=BUFFER) == float(r2_score(reg._y, pred))
    usage = est.independent_neighbor_usage(buffer=BUFFER)
    np.testing.assert_array_equal(usage.counts.sum(axis=1), np.bincount(want_i.reshape(-1), minlength=N_TRAIN))
    counts, _ = reg.engine_.tally_from_neighbors(want_d, want_i)
    np.testing.assert_array_equal(usage.counts, counts)
    usage3 = est.independent_neighbor_usage(GROUPS, n_neighbors=3, buffer=BUFFER)
    np.testing.assert_array_equal(usage3.counts.sum(axis=1),
                                  np.bincount(model(est, 3, codes=GROUPS)[1].reshape(-1), minlength=N_TRAIN))


@pytest.mark.parametrize("name", ["raw_default", "gnn", "rfnn"])
def test_summaries(fitted, name):
    from sknnr_amd._base import normalize_outputs, normalize_statistic

    est = fitted(name, weights="distance")
    reg = getattr(est, "regressor_", est)
    dist, idx = model(est, 5)
    outputs = [(0, "mean"), (0, ("quantile", 0.9)), (1, "mode")]
    got = est.independent_summarize(outputs=outputs, buffer=BUFFER)
    plan = normalize_outputs(outputs, reg._n_targets())
    np.testing.assert_array_equal(got, reg.engine_.summarize_plan_from_neighbors(dist, idx, "distance", plan))
    assert got.shape == (N_TRAIN, 3)
    np.testing.assert_array_equal(got[:, 0], est.independent_predict(buffer=BUFFER)[:, 0])
    got = est.independent_summarize(statistic="max", buffer=BUFFER)
    stat = normalize_statistic("max", reg._n_targets())
    np.testing.assert_array_equal(got, reg.engine_.summarize_from_neighbors(dist, idx, "distance", stat))
    np.testing.assert_array_equal(got, reg._y[idx].max(axis=1))
    np.testing.assert_array_equal(est.independent_summarize(buffer=BUFFER), est.independent_predict(buffer=BUFFER))


def test_one_target_gives_a_vector(moscow_frames):
    import sknnr_amd

    y1 = moscow_frames["y_train"].iloc[:, 0]
    est = sknnr_amd.RawKNNRegressor(n_neighbors=5).fit(moscow_frames["X_train"], y1)
    pred = est.independent_predict(buffer=BUFFER)
    assert pred.shape == (N_TRAIN,)
    dist, idx = model(est, 5)
    np.testing.assert_array_equal(pred, est.engine_.predict_from_neighbors(dist, idx, "uniform").reshape(-1))
    assert est.independent_summarize(statistic="max", buffer=BUFFER).shape == (N_TRAIN,)
    w = np.linspace(1.0, 2.0, N_TRAIN)
    assert est.independent_score(buffer=BUFFER, sample_weight=w) == float(r2_score(y1.to_numpy(), pred, sample_weight=w))
    counts = est.buffer_counts(BUFFER)
    assert counts.dtype == np.int64 and counts.shape == (N_TRAIN,)


def test_the_engine_uploads_positions_only_when_they_change(fitted, monkeypatch):
    est = fitted("raw_default")
    ix = est.engine_._index
    calls = []
    real = ix.set_buffer
    monkeypatch.setattr(ix, "set_buffer", lambda coords, radius=0.0: (calls.append(1), real(coords, radius))[1])
    est.independent_kneighbors(buffer=(COORDS + 1.0, RADIUS))  # whatever the handle held: at most one upload
    n = len(calls)
    assert n == 1
    est.independent_kneighbors(buffer=(COORDS + 1.0, RADIUS))
    est.independent_predict(buffer=((COORDS + 1.0).tolist(), int(RADIUS)))  # the same positions, another container
    est.buffer_counts((COORDS + 1.0, RADIUS))
    assert len(calls) == n
    est.independent_kneighbors(buffer=(COORDS + 1.0, RADIUS + 1.0))  # another radius
    assert len(calls) == n + 1
    est.independent_kneighbors(buffer=(COORDS, RADIUS + 1.0))  # other positions
    assert len(calls) == n + 2
    est.independent_kneighbors(GROUPS)  # no buffer: cleared, once
    est.independent_kneighbors(GROUPS)
    assert len(calls) == n + 3
    import pickle

    assert not any("buffer" in k for k in est.__getstate__())
    clone = pickle.loads(pickle.dumps(est))
    np.testing.assert_array_equal(clone.independent_kneighbors(buffer=BUFFER)[1], est.independent_kneighbors(buffer=BUFFER)[1])


def test_refusals(fitted):
    from sknnr_amd import hamming_tie_policy, tree_tie_policy

    est = fitted("raw_default")
    counts = _buffer.excluded_counts(COORDS, RADIUS)
    worst, row = int(counts.max()), int(np.argmax(counts))
    with pytest.raises(ValueError, match=rf"Expected n_neighbors <= n_samples_fit - max\(excluded\), but n_neighbors = {133 - worst}, "
                                         rf"n_samples_fit = 132, max\(excluded\) = {worst} \(row {row}\)"):
        est.independent_kneighbors(buffer=BUFFER, n_neighbors=133 - worst)
    est.independent_kneighbors(buffer=BUFFER, n_neighbors=132 - worst)
    with pytest.raises(ValueError, match=r"max\(excluded\) = 132 \(row 0\)"):  # a radius that swallows everything
        est.independent_predict(buffer=(COORDS, 1e6))
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit - largest group, but n_neighbors = 130, "
                                         "n_samples_fit = 132, largest group = 3"):  # groups alone: the message as it was
        est.independent_kneighbors(GROUPS, n_neighbors=130)
    with pytest.raises(ValueError, match="one row per fitted row"):
        est.independent_predict(buffer=(COORDS[:-1], RADIUS))
    with pytest.raises(ValueError, match="radius must be finite and >= 0"):
        est.independent_score(buffer=(COORDS, -1.0))
    with pytest.raises(ValueError, match="1 to 3 columns, got 4"):
        est.buffer_counts((np.zeros((N_TRAIN, 4)), 1.0))
    with pytest.raises(ValueError, match="single group"):
        est.independent_kneighbors(np.zeros(N_TRAIN), buffer=BUFFER)
    with pytest.raises(ValueError, match=r"groups must be 1-D with one label per fitted row, got an array of shape \(\)"):
        est.independent_kneighbors()
    with tree_tie_policy("tree"):
        if searched(fitted("raw_kd_tree"))[0]._tree_ties():
            with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
                fitted("raw_kd_tree").independent_score(buffer=BUFFER)
    with hamming_tie_policy("numpy"):
        for name in ("independent_kneighbors", "independent_predict", "independent_summarize", "independent_score",
                     "independent_neighbor_usage"):
            with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
                getattr(fitted("rfnn"), name)(buffer=BUFFER)
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            fitted("rfnn").buffer_counts(BUFFER)
