"""Leave-group-out neighbours at estimator level, on the Moscow fixture (132 training rows, groups of three consecutive
rows, as integers and as strings).  Neighbours are compared bit for bit with the contract's numpy model (tests/_groups.py)
on the rows the fitted regressor searches (``regressor_._fit_X``); everything above them with the engine's own reductions
on those neighbours, and with the oracle's ``predict``.

``RawKNNRegressor()`` resolves to the brute engine on this fixture (28 features), so ``algorithm="kd_tree"`` stands for
the direct formula beside the default and ``algorithm="brute"``."""

from __future__ import annotations

import numpy as np
import pytest
from sklearn.metrics import r2_score

import _groups
from conftest import yaimpute_weights

pytestmark = pytest.mark.gpu

N_TRAIN = 132
GROUPS = np.arange(N_TRAIN) // 3

ESTIMATORS = {
    "raw_default": ("RawKNNRegressor", {}),
    "raw_brute": ("RawKNNRegressor", {"algorithm": "brute"}),
    "raw_kd_tree": ("RawKNNRegressor", {"algorithm": "kd_tree"}),
    "euclidean": ("EuclideanKNNRegressor", {}),
    "gnn": ("GNNRegressor", {}),
    "rfnn": ("RFNNRegressor", {"n_estimators": 30, "random_state": 0}),  # 35 forests: 1,050 trees, swept in column chunks
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


def model(est, codes, k, deterministic=True):
    reg, fit, formula, w = searched(est)
    return _groups.grouped_kneighbors(fit, codes, k, formula=formula, w=w, deterministic=deterministic)


def test_the_three_raw_estimators_cover_both_formulas(fitted):
    assert [searched(fitted(n))[2] for n in ("raw_default", "raw_brute", "raw_kd_tree")] == ["expanded", "expanded", "direct"]
    assert searched(fitted("rfnn"))[2] == "hamming" and searched(fitted("rfnn"))[1].shape[1] > 1024


@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_neighbors_equal_the_model(fitted, name):
    est = fitted(name)
    for groups in (GROUPS, np.array([f"plot{g:03d}" for g in GROUPS])):
        for k, det in ((None, True), (3, False), (9, True)):
            dist, idx = est.independent_kneighbors(groups, n_neighbors=k, use_deterministic_ordering=det)
            want_d, want_i = model(est, GROUPS, 5 if k is None else k, det)
            np.testing.assert_array_equal(idx, want_i)
            np.testing.assert_array_equal(dist, want_d)
            assert isinstance(idx, np.ndarray) and not (GROUPS[idx] == GROUPS[:, None]).any()
    only = est.independent_kneighbors(GROUPS, return_distance=False)
    np.testing.assert_array_equal(only, model(est, GROUPS, 5)[1])


@pytest.mark.parametrize("name", ["raw_default", "gnn"])
def test_dataframe_ids(fitted, moscow_frames, name):
    import pandas as pd

    est = fitted(name)
    reg = getattr(est, "regressor_", est)
    _, idx = est.independent_kneighbors(pd.Series(GROUPS, index=moscow_frames["X_train"].index))
    _, ids = est.independent_kneighbors(GROUPS, return_dataframe_index=True)
    np.testing.assert_array_equal(ids, reg.dataframe_index_in_[idx])
    assert (ids != idx).any()  # (the frame's index starts at 1: ids are not positions)


@pytest.mark.parametrize("name", ["raw_default", "raw_kd_tree", "euclidean", "gnn", "rfnn"])
@pytest.mark.parametrize("weights", ["uniform", "distance", "yaimpute", "law"])
def test_predictions(fitted, name, weights):
    from oracle import oracle
    from sknnr_amd.weights import InverseDistance

    w = {"uniform": "uniform", "distance": "distance", "yaimpute": yaimpute_weights, "law": InverseDistance(1.0)}[weights]
    est = fitted(name, weights=w)
    reg = getattr(est, "regressor_", est)
    dist, idx = est.independent_kneighbors(GROUPS)
    pred = est.independent_predict(GROUPS)
    np.testing.assert_array_equal(pred, reg.engine_.predict_from_neighbors(dist, idx, w))
    np.testing.assert_array_equal(pred, oracle.predict(reg._y, dist, idx, w))  # (tests/test_hip_parity.py: bit for bit)
    assert pred.shape == reg._y.shape
    assert est.independent_score(GROUPS) == float(r2_score(reg._y, pred))


def test_one_target_gives_a_vector(moscow_frames):
    import sknnr_amd

    y1 = moscow_frames["y_train"].iloc[:, 0]
    est = sknnr_amd.RawKNNRegressor(n_neighbors=5).fit(moscow_frames["X_train"], y1)
    pred = est.independent_predict(GROUPS)
    assert pred.shape == (N_TRAIN,)
    dist, idx = est.independent_kneighbors(GROUPS)
    np.testing.assert_array_equal(pred, est.engine_.predict_from_neighbors(dist, idx, "uniform").reshape(-1))
    assert est.independent_summarize(GROUPS, statistic="max").shape == (N_TRAIN,)
    w = np.linspace(1.0, 2.0, N_TRAIN)
    assert est.independent_score(GROUPS, sample_weight=w) == float(r2_score(y1.to_numpy(), pred, sample_weight=w))


@pytest.mark.parametrize("name", ["raw_default", "gnn", "rfnn"])
def test_summaries(fitted, name):
    from sknnr_amd._base import normalize_outputs, normalize_statistic

    est = fitted(name, weights="distance")
    reg = getattr(est, "regressor_", est)
    dist, idx = est.independent_kneighbors(GROUPS)
    outputs = [(0, "mean"), (0, ("quantile", 0.9)), (1, "mode")]
    got = est.independent_summarize(GROUPS, outputs=outputs)
    plan = normalize_outputs(outputs, reg._n_targets())
    np.testing.assert_array_equal(got, reg.engine_.summarize_plan_from_neighbors(dist, idx, "distance", plan))
    assert got.shape == (N_TRAIN, 3)
    np.testing.assert_array_equal(got[:, 0], est.independent_predict(GROUPS)[:, 0])
    got = est.independent_summarize(GROUPS, statistic="max")
    stat = normalize_statistic("max", reg._n_targets())
    np.testing.assert_array_equal(got, reg.engine_.summarize_from_neighbors(dist, idx, "distance", stat))
    np.testing.assert_array_equal(got, reg._y[idx].max(axis=1))
    np.testing.assert_array_equal(est.independent_summarize(GROUPS), est.independent_predict(GROUPS))


@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_singleton_groups_are_the_independent_prediction(fitted, name):
    est = fitted(name)
    reg, fit, formula, w = searched(est)
    full = _groups.value_rows(fit, np.arange(N_TRAIN), formula, w)
    keep = np.ones(N_TRAIN, dtype=bool)
    keep[_groups.boundary_tie_rows(full, np.arange(N_TRAIN), 5)] = False  # (found with the oracle alone)
    assert keep.sum() >= 0.9 * N_TRAIN
    pred = est.independent_predict(np.arange(N_TRAIN))
    np.testing.assert_array_equal(pred[keep], reg.independent_prediction_[keep])
    if keep.all():
        assert est.independent_score(np.arange(N_TRAIN)) == reg.independent_score_


def test_the_engine_uploads_codes_only_when_they_change(fitted, monkeypatch):
    est = fitted("raw_default")
    ix = est.engine_._index
    calls = []
    real = ix.set_groups
    monkeypatch.setattr(ix, "set_groups", lambda codes: (calls.append(1), real(codes))[1])
    est.independent_kneighbors(GROUPS + 7)  # other labels, the same codes as before or not: at most one upload
    est.independent_kneighbors(GROUPS)
    est.independent_predict([f"p{g}" for g in GROUPS % 44 + 100])
    n = len(calls)
    assert n <= 1
    est.independent_kneighbors(np.arange(N_TRAIN) // 4)
    assert len(calls) == n + 1
    import pickle

    assert not any("group" in k for k in est.__getstate__())
    clone = pickle.loads(pickle.dumps(est))
    np.testing.assert_array_equal(clone.independent_kneighbors(GROUPS)[1], est.independent_kneighbors(GROUPS)[1])


def test_refusals(fitted):
    from sknnr_amd import hamming_tie_policy, tree_tie_policy

    est = fitted("raw_default")
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit - largest group, but n_neighbors = 130, "
                                         "n_samples_fit = 132, largest group = 3"):
        est.independent_kneighbors(GROUPS, n_neighbors=130)
    est.independent_kneighbors(GROUPS, n_neighbors=129)
    with pytest.raises(ValueError, match="one label per fitted row"):
        est.independent_predict(GROUPS[:-1])
    with tree_tie_policy("tree"):
        for name in ("raw_kd_tree", "gnn"):
            if searched(fitted(name))[0]._tree_ties():
                with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
                    fitted(name).independent_kneighbors(GROUPS)
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            fitted("raw_kd_tree").independent_score(GROUPS)
    with hamming_tie_policy("numpy"):
        for call in ("independent_kneighbors", "independent_predict", "independent_summarize", "independent_score"):
            with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
                getattr(fitted("rfnn"), call)(GROUPS)
