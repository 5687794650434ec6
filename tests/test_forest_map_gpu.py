"""The query-time forest map of RFNN / GBNN on the GPU (sknnr_index_set_forest, sknnr_forest_apply, Hamming calls with
apply_affine): node ids equal to scikit-learn's apply, adversarial values at the thresholds, and the estimators answering
raw rows bit for bit as the host-ids call does -- with scikit-learn's traversal disabled."""

from __future__ import annotations

import os
import pickle

import numpy as np
import pytest
from sklearn.ensemble import (GradientBoostingClassifier, GradientBoostingRegressor, RandomForestClassifier,
                              RandomForestRegressor)

from conftest import GOLDEN, yaimpute_weights

pytestmark = pytest.mark.gpu

REF_DIR = os.path.join(GOLDEN, "ref_regressions")
NARROW = [np.float32, np.int16, np.uint16, np.uint8, np.int32]


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture
def no_host_traversal(monkeypatch):
    """Make every host route to node ids raise: TreeNodeTransformer.transform and each ensemble's apply."""
    from sknnr_amd.transformers import TreeNodeTransformer

    def refuse(*a, **k):
        raise AssertionError("host tree traversal was called")

    def disable():
        monkeypatch.setattr(TreeNodeTransformer, "transform", refuse)
        for cls in (RandomForestRegressor, RandomForestClassifier, GradientBoostingRegressor, GradientBoostingClassifier):
            monkeypatch.setattr(cls, "apply", refuse)

    return disable


def _index_for(N, transformer, X_fit):
    ids = transformer.transform(X_fit).astype(np.float64)
    ix = N.Index(ids)
    image = transformer.forest_image()
    ix.set_forest(image["d_in"], image["tree_offset"], image["threshold"], image["feature"], image["left"],
                  image["right"])
    return ix


def _transformers():
    from sknnr_amd.transformers import GBNodeTransformer, RFNodeTransformer

    rng = np.random.default_rng(0)
    X = rng.normal(size=(400, 7))
    y = X[:, 0] + 0.3 * rng.normal(size=400)
    y_str = np.where(X[:, 1] > 0.2, "high", "low")
    y3 = np.array(["a", "b", "c"])[rng.integers(0, 3, 400)]
    return X, {
        "rf_regressor": RFNodeTransformer(n_estimators=12, random_state=0).fit(X, y),
        "rf_classifier_strings": RFNodeTransformer(n_estimators=9, random_state=0).fit(X, np.c_[y, y_str].astype(object)),
        "gb_regressor": GBNodeTransformer(n_estimators=20, random_state=0).fit(X, y),
        "gb_binary": GBNodeTransformer(n_estimators=15, random_state=0).fit(X, y_str),
        "gb_3class": GBNodeTransformer(n_estimators=10, random_state=0).fit(X, y3),
        "gb_early_stop": GBNodeTransformer(n_estimators=300, n_iter_no_change=2, random_state=0).fit(X, y),
    }


def _threshold_rows(image, base, n_rows=4000, seed=1):
    """Rows whose values sit at, and on both sides of, the forests' thresholds: the threshold itself, its float64
    neighbours (they round across it when cast to float32 whenever the threshold is no float32), its float32
    neighbours, and +-0."""
    rng = np.random.default_rng(seed)
    inner = np.flatnonzero(image["left"] != -1)
    pick = inner[rng.integers(0, inner.size, n_rows)]
    thr = image["threshold"][pick]
    f32 = thr.astype(np.float32)
    cand = np.stack([thr, np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf),
                     np.nextafter(f32, np.float32(np.inf)).astype(np.float64),
                     np.nextafter(f32, np.float32(-np.inf)).astype(np.float64), f32.astype(np.float64)], axis=1)
    rows = base[rng.integers(0, len(base), n_rows)].astype(np.float64)
    rows[np.arange(n_rows), image["feature"][pick]] = cand[np.arange(n_rows), rng.integers(0, 6, n_rows)]
    zeros = base[:8].astype(np.float64).copy()
    zeros[:4] = 0.0
    zeros[4:] = -0.0
    return np.vstack([rows, zeros])


@pytest.mark.parametrize("name", ["rf_regressor", "rf_classifier_strings", "gb_regressor", "gb_binary", "gb_3class",
                                  "gb_early_stop"])
def test_forest_apply_equals_apply(N, name):
    X, transformers = _transformers()
    t = transformers[name]
    ix = _index_for(N, t, X)
    Xq = np.vstack([np.random.default_rng(3).normal(size=(3000, X.shape[1])), _threshold_rows(t.forest_image(), X)])
    np.testing.assert_array_equal(ix.forest_apply_host(Xq), t.transform(Xq))
    np.testing.assert_array_equal(ix.forest_apply_host(Xq.astype(np.float32), 1), t.transform(Xq.astype(np.float32)))
    ix.close()


def test_float64_values_that_round_across_a_threshold(N):
    """A float64 value above a threshold whose float32 is not (or the reverse) goes where apply sends it; a plain
    float64 compare would send it the other way."""
    X, transformers = _transformers()
    t = transformers["rf_regressor"]
    image = t.forest_image()
    ix = _index_for(N, t, X)
    Xq = _threshold_rows(image, X, n_rows=20000, seed=9)
    want = t.transform(Xq)
    np.testing.assert_array_equal(ix.forest_apply_host(Xq), want)
    # the adversarial case is present: some row's float64 value and its float32 fall on different sides
    inner = np.flatnonzero(image["left"] != -1)
    thr = image["threshold"][inner]
    v = np.nextafter(thr, np.inf)
    assert np.any((v.astype(np.float32).astype(np.float64) <= thr) != (v <= thr))
    ix.close()


def test_narrow_dtypes_large_int32_and_subnormals(N):
    from sknnr_amd.transformers import RFNodeTransformer

    rng = np.random.default_rng(4)
    n = 600
    X = np.c_[rng.integers(0, 256, n), rng.integers(-300, 300, n), rng.integers(0, 60000, n),
              rng.integers(1 << 24, 1 << 26, n), rng.uniform(0, 1e-38, n), rng.normal(size=n)].astype(np.float64)
    y = X[:, 0] + X[:, 3] / (1 << 24) + X[:, 4] * 1e38 + X[:, 5]
    t = RFNodeTransformer(n_estimators=10, min_samples_leaf=2, random_state=0).fit(X, y)
    ix = _index_for(N, t, X)
    Xq = _threshold_rows(t.forest_image(), X, n_rows=5000, seed=2)
    np.testing.assert_array_equal(ix.forest_apply_host(Xq), t.transform(Xq))
    # int32 above 2^24 (rounded to float32 as numpy does), and every narrow dtype on values it holds
    big = np.c_[np.zeros((4000, 3)), rng.integers((1 << 24) - 5, (1 << 26) + 5, 4000), np.zeros((4000, 2))]
    big = np.vstack([Xq[:4000], big]).round()
    for dt, lo, hi in ((np.int32, -(1 << 31), (1 << 31) - 1), (np.int16, -32768, 32767), (np.uint16, 0, 65535),
                       (np.uint8, 0, 255)):
        q = np.clip(big, lo, hi).astype(dt)
        np.testing.assert_array_equal(ix.forest_apply_host(q, N.dtype_code(dt)), t.transform(q))
    q = Xq.astype(np.float32)
    np.testing.assert_array_equal(ix.forest_apply_host(q, 1), t.transform(q))
    ix.close()


def test_structure_check_on_install(N):
    X, transformers = _transformers()
    t = transformers["rf_regressor"]
    ids = t.transform(X).astype(np.float64)
    ix = N.Index(ids)
    base = t.forest_image()
    inner = np.flatnonzero(base["left"] != -1)
    for field, value in (("right", 0), ("left", int(base["tree_offset"][1] - base["tree_offset"][0])),
                         ("feature", base["d_in"])):
        img = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        img[field][inner[0] if field != "right" else inner[1]] = value
        with pytest.raises(N.HipBackendError) as e:
            ix.set_forest(img["d_in"], img["tree_offset"], img["threshold"], img["feature"], img["left"], img["right"])
        assert e.value.code == N.ERR_INVALID
    with pytest.raises(N.HipBackendError):  # no forest installed: nothing to apply
        ix.forest_apply_host(X[:3])
    ix.close()


def test_ids_beyond_16_bits_reach_the_exact_scan(no_host_traversal):
    """A forest of large trees (node ids beyond 65,535): the integer Hamming pre-filter cannot hold them and the float64
    scan answers; the ids and the neighbours equal the host path's."""
    import sknnr_amd

    rng = np.random.default_rng(8)
    X = rng.normal(size=(90000, 4))
    y = X @ np.array([1.0, -2.0, 0.5, 0.0]) + rng.normal(size=len(X))
    est = sknnr_amd.RFNNRegressor(n_estimators=2, min_samples_leaf=1, n_neighbors=5, random_state=0).fit(X, y)
    Xq = rng.normal(size=(700, 4))
    ids = est.transformer_.transform(Xq)
    assert est.transformer_.transform(X).max() > 65535
    want_d, want_i = est.regressor_.kneighbors(ids.astype(np.float64))
    want_p = est.regressor_.predict(ids.astype(np.float64))
    no_host_traversal()
    np.testing.assert_array_equal(est.regressor_.engine_.forest_apply(Xq), ids)
    d, i = est.kneighbors(Xq)
    np.testing.assert_array_equal(i, want_i)
    np.testing.assert_array_equal(d, want_d)
    np.testing.assert_array_equal(est.predict(Xq), want_p)


def _moscow_estimator(which, f, **kw):
    import sknnr_amd

    cls = {"rfnn": sknnr_amd.RFNNRegressor, "gbnn": sknnr_amd.GBNNRegressor}[which]
    return cls(n_neighbors=5, random_state=42, **kw).fit(f["X_train"], f["y_train"])


def _host_answers(est, X):
    ids = np.ascontiguousarray(est.transformer_.transform(X), dtype=np.float64)
    out = {}
    for det in (True, False):
        out["kn", det] = est.regressor_.kneighbors(ids, use_deterministic_ordering=det)
    out["kn_ids"] = est.regressor_.kneighbors(ids, return_dataframe_index=True)
    out["kn3"] = est.regressor_.kneighbors(ids, n_neighbors=3)
    out["pred"] = est.regressor_.predict(ids)
    return ids, out


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
def test_moscow_estimators_map_raw_rows_on_the_device(which, moscow_frames, no_host_traversal):
    """RFNN / GBNN with their reference configuration on the Moscow frames: kneighbors / predict / score of raw rows
    equal the host-ids call bit for bit, with scikit-learn's traversal disabled."""
    from sklearn.metrics import r2_score

    f = moscow_frames
    est = _moscow_estimator(which, f)
    est_w = _moscow_estimator(which, f, weights=yaimpute_weights)
    X = f["X_test"]
    ids, want = _host_answers(est, X)
    want_w = est_w.regressor_.predict(est_w.transformer_.transform(X).astype(np.float64))
    no_host_traversal()
    np.testing.assert_array_equal(est.regressor_.engine_.forest_apply(X.to_numpy()), ids)
    for det in (True, False):
        d, i = est.kneighbors(X, use_deterministic_ordering=det)
        np.testing.assert_array_equal(i, want["kn", det][1])
        np.testing.assert_array_equal(d, want["kn", det][0])
    d, i = est.kneighbors(X, return_dataframe_index=True)
    np.testing.assert_array_equal(i, want["kn_ids"][1])
    d, i = est.kneighbors(X, n_neighbors=3)
    np.testing.assert_array_equal(i, want["kn3"][1])
    np.testing.assert_array_equal(d, want["kn3"][0])
    np.testing.assert_array_equal(est.predict(X), want["pred"])
    np.testing.assert_array_equal(est_w.predict(X), want_w)
    assert est.score(X, f["y_test"]) == float(r2_score(f["y_test"], want["pred"]))
    # plain arrays and float32 rows (validated, kept at their width)
    np.testing.assert_array_equal(est.kneighbors(X.to_numpy())[1], want["kn", True][1])
    X32 = X.to_numpy().astype(np.float32)
    np.testing.assert_array_equal(est.regressor_.engine_.forest_apply(X32),
                                  est.regressor_.engine_.forest_apply(X32.astype(np.float64)))


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
def test_chunks_of_narrow_tiles_equal_the_one_shot_call(which, moscow_frames, no_host_traversal):
    f = moscow_frames
    est = _moscow_estimator(which, f)
    no_host_traversal()
    base = f["X_all"].to_numpy()
    rows = np.vstack([base] * 30)  # 4,950 rows
    for dt in (np.uint8, np.int16, np.float32):
        info = np.iinfo(dt) if np.issubdtype(dt, np.integer) else None
        q = (np.clip(rows.round(), info.min, info.max) if info else rows).astype(dt)
        tiles = [q[:1000], q[1000:1001], q[1001:3333], q[3333:]]
        want_d, want_i = est.kneighbors(q.astype(np.float64))
        want_p = est.predict(q.astype(np.float64))
        d, i = est.kneighbors_chunks(iter(tiles))
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(d, want_d)
        np.testing.assert_array_equal(est.predict_chunks(iter(tiles)), want_p)
        d, i = est.kneighbors(q)
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(est.predict(q), want_p)


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
def test_cuda_tensor_queries_equal_host_queries(which, moscow_frames, no_host_traversal):
    import torch

    f = moscow_frames
    est = _moscow_estimator(which, f)
    no_host_traversal()
    X = f["X_test"].to_numpy()
    want_d, want_i = est.kneighbors(X)
    want_p = est.predict(X)
    for dt in (torch.float64, torch.float32, torch.int64):
        Xt = torch.as_tensor(X if dt != torch.int64 else X.round()).to(dt).cuda()
        host = X if dt != torch.int64 else X.round().astype(np.int64)
        hd, hi = est.kneighbors(host)
        d, i = est.kneighbors(Xt)
        assert isinstance(i, np.ndarray) and isinstance(d, np.ndarray)  # (these estimators return host arrays)
        np.testing.assert_array_equal(i, hi)
        np.testing.assert_array_equal(d, hd)
        np.testing.assert_array_equal(est.predict(Xt), est.predict(host))
    Xt = torch.as_tensor(X).cuda()
    np.testing.assert_array_equal(est.kneighbors(Xt)[1], want_i)
    np.testing.assert_array_equal(est.predict(Xt), want_p)
    np.testing.assert_array_equal(est.regressor_.engine_.forest_apply(Xt).cpu().numpy(),
                                  est.regressor_.engine_.forest_apply(X))


@pytest.mark.parametrize("which, cls_name", [("randomForest", "RFNNRegressor"), ("gbnn", "GBNNRegressor")])
def test_numpy_tie_policy_files_with_apply_disabled(which, cls_name, moscow_frames, no_host_traversal):
    """The reference's committed RFNN / GBNN regression files under hamming_tie_policy("numpy"), the query rows mapped
    by the device (the tied rows' ids from forest_apply)."""
    import sknnr_amd

    f = moscow_frames
    with sknnr_amd.hamming_tie_policy("numpy"):
        est = getattr(sknnr_amd, cls_name)(n_neighbors=5, random_state=42).fit(f["X_train"], f["y_train"])
        est_w = getattr(sknnr_amd, cls_name)(n_neighbors=5, random_state=42, weights=yaimpute_weights).fit(
            f["X_train"], f["y_train"])
        no_host_traversal()
        for ret_ids, tag in ((False, "index"), (True, "ids")):
            rf = np.load(os.path.join(REF_DIR, f"test_kneighbors_target_full_{which}_k5_{tag}_.npz"))
            dist, nn = est.kneighbors(f["X_test"], return_dataframe_index=ret_ids)
            np.testing.assert_array_equal(nn, rf["nn"])
            np.testing.assert_allclose(dist, rf["dist"], rtol=1e-5, atol=1e-8)
        for e, stem in ((est, "unweighted"), (est_w, "weighted")):
            rf = np.load(os.path.join(REF_DIR, f"test_predict_target_{stem}_full_{which}_k5_.npz"))
            np.testing.assert_allclose(e.predict(f["X_test"]), rf["pred"], rtol=1e-5, atol=1e-8)
        assert est.regressor_._last_numpy_tie_rows >= 0


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
def test_errors_are_the_host_paths(which, moscow_frames, no_host_traversal):
    """NaN, infinity, a finite value beyond float32, wrong feature counts and names: the host path's exceptions."""
    import torch

    f = moscow_frames
    est = _moscow_estimator(which, f)
    X = f["X_test"].to_numpy()
    cases = []
    for v, dt in ((np.nan, np.float64), (np.inf, np.float64), (-np.inf, np.float64), (1e39, np.float64),
                  (-3.5e38, np.float64), (np.inf, np.float32), (np.nan, np.float32)):
        bad = X.astype(dt)
        bad[3, 2] = v
        cases.append(bad)
    cases += [X[:, :-1], f["X_test"].rename(columns={f["X_test"].columns[0]: "renamed"})]
    expected = []
    for bad in cases:
        with pytest.raises(ValueError) as e:
            est.transformer_.transform(bad)
        expected.append(str(e.value))
    no_host_traversal()
    for bad, msg in zip(cases, expected):
        for call in (est.kneighbors, est.predict, lambda q: est.kneighbors_chunks(iter([q[:5], q[5:]]))):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == msg
    for bad, msg in zip(cases[:4], expected[:4]):
        with pytest.raises(ValueError) as e:
            est.kneighbors(torch.as_tensor(bad).cuda())
        assert str(e.value) == msg
    # a failed call leaves no flag behind
    np.testing.assert_array_equal(est.kneighbors(X)[1], est.kneighbors(X.astype(np.float32))[1])


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
def test_pickle_round_trip_reinstalls_the_forests(which, moscow_frames, no_host_traversal):
    f = moscow_frames
    est = _moscow_estimator(which, f)
    X = f["X_test"]
    want_d, want_i = est.kneighbors(X)
    want_p = est.predict(X)
    clone = pickle.loads(pickle.dumps(est))
    no_host_traversal()
    d, i = clone.kneighbors(X)
    np.testing.assert_array_equal(i, want_i)
    np.testing.assert_array_equal(d, want_d)
    np.testing.assert_array_equal(clone.predict(X), want_p)
    assert clone.regressor_.engine_.has_forest
