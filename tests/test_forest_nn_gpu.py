"""RFNN / GBNN on the GPU: the weighted-Hamming search (SKNNR_FORMULA_HAMMING) through the C ABI against
the oracle (bit for bit: same arithmetic, same tie rule) and against the reference's vectors (tie
classes at the k-th distance compared as classes), and the estimator classes end to end."""

from __future__ import annotations

import os

import numpy as np
import pytest
from sklearn.metrics import r2_score

from conftest import (GOLDEN, assert_hamming_neighbors_match, load_golden, mixed_forest_y_fit, rows_without,
                      yaimpute_weights)

pytestmark = pytest.mark.gpu

CASES = ["rfnn", "gbnn", "rfnn_weighted", "gbnn_uniform"]
REF_DIR = os.path.join(GOLDEN, "ref_regressions")
REFERENCE_FILES = {"rfnn": "randomForest", "gbnn": "gbnn"}  # fixtures that are the reference's regression configuration
# rows (kneighbors(X_test), kneighbors()) whose neighbour SET differs from the reference's: boundary ties only,
# where numpy's argpartition -- SIMD quick-select on the maintainers' machine -- and the device's
# lowest-index-first rule keep different rows (scripts/hamming_tie_dispatch.py)
EXPECTED_TIE_ROWS = {"rfnn": (1, 0), "gbnn": (0, 0), "rfnn_weighted": (0, 0), "gbnn_uniform": (4, 1)}
# (the mixed-forest RFNN has 100 uniformly weighted trees: distances are multiples of 1/100 and boundary ties common)
EXPECTED_MIXED_TIE_ROWS = {("randomForest", True): 12, ("randomForest", False): 5, ("gbnn", True): 0, ("gbnn", False): 0}


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("deterministic", [True, False])
def test_hamming_search_equals_the_oracle(N, O, name, deterministic):
    """Node ids and weights the reference produced (1,750 / 3,500 / 700 / 1,050 trees: the wide ones
    exercise the column-chunked scan): indices and float64 distances bit-equal to the oracle, for
    queries and for the X=None self query."""
    g = load_golden(f"moscow_{name}.npz")
    ids_tr, ids_te, w = g["ids_train"].astype(np.float64), g["ids_test"].astype(np.float64), g["hamming_weights"]
    ix = N.Index(ids_tr)
    ix.set_hamming_weights(w)
    for k in (1, 5, 9):
        o = ix.make_opts(k, formula=N.FORMULA_HAMMING, deterministic=deterministic)
        dist, idx = ix.kneighbors_host(ids_te, o)
        od, oi = O.kneighbors_hamming(ids_tr, ids_te, w, k, deterministic=deterministic)
        np.testing.assert_array_equal(idx, oi)
        np.testing.assert_array_equal(dist, od)
        o = ix.make_opts(k, formula=N.FORMULA_HAMMING, deterministic=deterministic, exclude_self=True)
        dist, idx = ix.kneighbors_host(None, o, nq=len(ids_tr))
        od, oi = O.kneighbors_hamming(ids_tr, None, w, k, deterministic=deterministic)
        np.testing.assert_array_equal(idx, oi)
        np.testing.assert_array_equal(dist, od)
    st = ix.stats()
    assert st["exact_only_queries"] == st["queries"] and st["coarse_queries"] == 0
    ix.close()


def test_hamming_search_larger_random_problem(N, O):
    """More rows than a scan pass, few distinct node ids (ties everywhere), real-valued weights, device
    tensors in and out, and a narrow matrix (T = 12 <= 128: the index also holds an unused MFMA image)."""
    import torch

    rng = np.random.default_rng(8)
    for t, levels in ((12, 3), (300, 5), (1100, 20)):
        ref = rng.integers(0, levels, (3000, t)).astype(np.float64)
        q = rng.integers(0, levels, (5000, t)).astype(np.float64)
        w = rng.random(t) + 0.01
        ix = N.Index(ref, rng.standard_normal((3000, 2)))
        ix.set_hamming_weights(w)
        o = ix.make_opts(4, formula=N.FORMULA_HAMMING, row_offset=7)
        qd = torch.as_tensor(q, device="cuda")
        dd = torch.empty((5000, 4), dtype=torch.float64, device="cuda")
        di = torch.empty((5000, 4), dtype=torch.int64, device="cuda")
        ix.kneighbors_device(qd.data_ptr(), 5000, o, dd.data_ptr(), di.data_ptr())
        torch.cuda.synchronize()
        od, oi = O.kneighbors_hamming(ref, q, w, 4, row_offset=7)
        np.testing.assert_array_equal(di.cpu().numpy(), oi)
        np.testing.assert_array_equal(dd.cpu().numpy(), od)
        ix.close()


def test_hamming_errors(N):
    ix = N.Index(np.zeros((10, 4)))
    with pytest.raises(N.HipBackendError, match="set_hamming_weights"):
        ix.kneighbors_host(np.zeros((2, 4)), ix.make_opts(1, formula=N.FORMULA_HAMMING))
    with pytest.raises(N.HipBackendError, match="one weight per column"):
        ix.set_hamming_weights(np.ones(3))
    with pytest.raises(N.HipBackendError, match="finite and non-negative"):
        ix.set_hamming_weights(np.array([1.0, -1.0, 1.0, 1.0]))
    with pytest.raises(N.HipBackendError, match="sum to zero"):
        ix.set_hamming_weights(np.zeros(4))
    ix.close()


@pytest.mark.parametrize("name, cls_name, kw", [
    ("rfnn", "RFNNRegressor", dict(random_state=42)),
    ("gbnn", "GBNNRegressor", dict(random_state=42)),
    ("rfnn_weighted", "RFNNRegressor", dict(random_state=42, n_estimators=20, forest_weights=np.arange(1, 36))),
    ("gbnn_uniform", "GBNNRegressor", dict(random_state=42, n_estimators=30, tree_weighting_method="uniform")),
])
def test_estimators_against_the_reference(name, cls_name, kw, moscow_frames):
    """End to end (forests grown here by scikit-learn with the reference's seeds): Hamming weights equal,
    neighbours and predictions as the reference's up to the tie classes at the k-th distance."""
    import sknnr_amd

    g = load_golden(f"moscow_{name}.npz")
    f = moscow_frames
    est = getattr(sknnr_amd, cls_name)(n_neighbors=5, **kw).fit(f["X_train"], f["y_train"])
    np.testing.assert_array_equal(est.hamming_weights_, g["hamming_weights"])
    assert est.hamming_weights_.sum() == pytest.approx(1.0)
    assert est.n_features_in_ == g["ids_train"].shape[1]
    ids_tr, ids_te, w = g["ids_train"], g["ids_test"], g["hamming_weights"]
    d, i = est.kneighbors(f["X_test"])
    tie_tgt = assert_hamming_neighbors_match(i, d, g["kn_tgt_k5_nn"], g["kn_tgt_k5_dist"], ids_tr, ids_te, w)
    d_ids, ids = est.kneighbors(f["X_test"], return_dataframe_index=True)
    np.testing.assert_array_equal(ids, est.dataframe_index_in_[i])
    d, i = est.kneighbors()
    tie_ref = assert_hamming_neighbors_match(i, d, g["kn_ref_k5_nn"], g["kn_ref_k5_dist"], ids_tr, ids_tr, w,
                                             row_offset_self=0)
    d1, i1 = est.kneighbors(f["X_test"], n_neighbors=1)
    assert_hamming_neighbors_match(i1, d1, g["kn_tgt_k1_nn"], g["kn_tgt_k1_dist"], ids_tr, ids_te, w)
    # The rows whose index set differs from the reference's are exactly boundary-tie rows (asserted above), a
    # machine-dependent pick of numpy's argpartition (profiles/r03_hamming_tie_dispatch.txt); their number is pinned
    # so that a new deviation cannot hide behind the rule.  EVERY other row must carry the reference's predictions.
    assert (len(tie_tgt), len(tie_ref)) == EXPECTED_TIE_ROWS[name], (tie_tgt, tie_ref)
    keep_tgt, keep_ref = rows_without(33, tie_tgt), rows_without(132, tie_ref)
    y_train = f["y_train"].to_numpy()
    ref_files = REFERENCE_FILES.get(name)

    def check_predictions(est_, pred_tgt, indep_pred, indep_score):
        np.testing.assert_allclose(est_.predict(f["X_test"])[keep_tgt], pred_tgt[keep_tgt], rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(est_.independent_prediction_[keep_ref], indep_pred[keep_ref], rtol=1e-5, atol=1e-8)
        if indep_score is not None:
            # the score with the tie rows' predictions taken from the reference: everything else is ours
            patched = est_.independent_prediction_.copy()
            patched[~keep_ref] = indep_pred[~keep_ref]
            assert r2_score(y_train, patched) == pytest.approx(float(indep_score), rel=1e-6)
            if not len(tie_ref):
                assert est_.independent_score_ == pytest.approx(float(indep_score), rel=1e-6)

    check_predictions(est, g["pred_tgt_uniform"], g["indep_pred_uniform"], g["indep_score_uniform"])
    est_w = getattr(sknnr_amd, cls_name)(n_neighbors=5, weights=yaimpute_weights, **kw).fit(f["X_train"], f["y_train"])
    check_predictions(est_w, g["pred_tgt_yaimpute"], g["indep_pred_yaimpute"], None)
    est_d = getattr(sknnr_amd, cls_name)(n_neighbors=5, weights="distance", **kw).fit(f["X_train"], f["y_train"])
    np.testing.assert_allclose(est_d.predict(f["X_test"])[keep_tgt], g["pred_tgt_distance"][keep_tgt], rtol=1e-5, atol=1e-8)
    if ref_files:  # ... and the reference maintainers' own files (REF tests/test_regressions.py:89-122)
        def ref(kind):
            return np.load(os.path.join(REF_DIR, f"test_predict_{kind}_full_{ref_files}_k5_.npz"))

        check_predictions(est, ref("target_unweighted")["pred"], ref("reference_unweighted")["pred"],
                          ref("reference_unweighted")["score"])
        check_predictions(est_w, ref("target_weighted")["pred"], ref("reference_weighted")["pred"],
                          ref("reference_weighted")["score"])
        for kind, own in (("target", (est.kneighbors(f["X_test"]), ids_te, None)), ("reference", (est.kneighbors(), ids_tr, 0))):
            (dd, ii), q_ids, self0 = own
            rf = np.load(os.path.join(REF_DIR, f"test_kneighbors_{kind}_full_{ref_files}_k5_index_.npz"))
            t_rows = assert_hamming_neighbors_match(ii, dd, rf["nn"], rf["dist"], ids_tr, q_ids, w, row_offset_self=self0)
            keep = rows_without(len(ii), t_rows)
            np.testing.assert_array_equal(ii[keep], rf["nn"][keep])  # same order too, on every non-tie row
            rid = np.load(os.path.join(REF_DIR, f"test_kneighbors_{kind}_full_{ref_files}_k5_ids_.npz"))
            got_ids = est.kneighbors(f["X_test"] if kind == "target" else None, return_dataframe_index=True)[1]
            np.testing.assert_array_equal(got_ids[keep], rid["nn"][keep])


@pytest.mark.parametrize("which, reference, atol", [("randomForest", True, 1e-8), ("randomForest", False, 1e-8),
                                                     ("gbnn", True, 1e-8), ("gbnn", False, 1e-2)])
def test_estimators_with_mixed_type_forests(which, reference, atol, moscow_frames):
    """REF tests/test_regressions.py:125-195, same construction (one regression forest on Total_BA and one
    three-class classification forest on the dominant species), same columns and tolerances, against the
    reference's own four files."""
    import sknnr_amd

    f = moscow_frames
    cls = {"randomForest": sknnr_amd.RFNNRegressor, "gbnn": sknnr_amd.GBNNRegressor}[which]
    est = cls(n_neighbors=5, random_state=42).fit(f["X_train"], f["y_train"], y_fit=mixed_forest_y_fit(f["y_train"]))
    assert sorted(est.transformer_.estimator_type_dict_.values()) == ["classification", "regression"]
    ids_tr = est.transformer_.transform(f["X_train"])
    rf = np.load(os.path.join(REF_DIR, f"test_estimators_with_mixed_type_forests_{'reference' if reference else 'target'}_{which}_.npz"))
    if reference:
        dist, nn = est.kneighbors()
        pred, q_ids = est.independent_prediction_, ids_tr
    else:
        dist, nn = est.kneighbors(f["X_test"])
        pred, q_ids = est.predict(f["X_test"]), est.transformer_.transform(f["X_test"])
    ties = assert_hamming_neighbors_match(nn, dist, rf["nn"], rf["dist"], ids_tr, q_ids, est.hamming_weights_,
                                          row_offset_self=0 if reference else None, atol=atol)
    keep = rows_without(len(nn), ties)
    np.testing.assert_array_equal(nn[keep], rf["nn"][keep])
    np.testing.assert_allclose(dist[keep], rf["dist"][keep], rtol=1e-5, atol=atol)
    np.testing.assert_allclose(pred[keep], rf["pred"][keep], rtol=1e-5, atol=1e-8)
    assert len(ties) == EXPECTED_MIXED_TIE_ROWS[(which, reference)], ties
    if reference:
        patched = pred.copy()
        patched[~keep] = rf["pred"][~keep]
        assert r2_score(f["y_train"].to_numpy(), patched) == pytest.approx(float(rf["score"]), rel=1e-5, abs=1e-8)


@pytest.mark.parametrize("which, cls_name", [("randomForest", "RFNNRegressor"), ("gbnn", "GBNNRegressor")])
def test_reference_regression_files_exact_under_the_numpy_tie_policy(which, cls_name, moscow_frames):
    """hamming_tie_policy("numpy") -- the reference's own choice among exactly tied rows (np.argpartition on the full
    distance row, which the device supplies): the reference maintainers' committed regression files for RFNN / GBNN
    (REF tests/test_regressions.py:57-122, the files under REF tests/test_regressions/) are matched with
    assert_array_equal on EVERY row, tie rows included -- neighbour indices, dataframe ids, predictions and score."""
    import sknnr_amd

    f = moscow_frames

    def ref(stem):
        return np.load(os.path.join(REF_DIR, f"{stem}_full_{which}_k5_.npz"))

    with sknnr_amd.hamming_tie_policy("numpy"):
        est = getattr(sknnr_amd, cls_name)(n_neighbors=5, random_state=42).fit(f["X_train"], f["y_train"])
        est_w = getattr(sknnr_amd, cls_name)(n_neighbors=5, random_state=42, weights=yaimpute_weights).fit(f["X_train"], f["y_train"])
        for kind, X in (("target", f["X_test"]), ("reference", None)):
            for ret_ids, tag in ((False, "index"), (True, "ids")):
                rf = np.load(os.path.join(REF_DIR, f"test_kneighbors_{kind}_full_{which}_k5_{tag}_.npz"))
                dist, nn = est.kneighbors(X, return_dataframe_index=ret_ids)
                np.testing.assert_array_equal(nn, rf["nn"])
                np.testing.assert_allclose(dist, rf["dist"], rtol=1e-5, atol=1e-8)
            np.testing.assert_allclose(est.predict(X) if X is not None else est.independent_prediction_,
                                       ref(f"test_predict_{kind}_unweighted")["pred"], rtol=1e-5, atol=1e-8)
            np.testing.assert_allclose(est_w.predict(X) if X is not None else est_w.independent_prediction_,
                                       ref(f"test_predict_{kind}_weighted")["pred"], rtol=1e-5, atol=1e-8)
        assert est.independent_score_ == pytest.approx(float(ref("test_predict_reference_unweighted")["score"]), rel=1e-6)
        assert est_w.independent_score_ == pytest.approx(float(ref("test_predict_reference_weighted")["score"]), rel=1e-6)
        # without the deterministic reorder the ORDER among tied rows is argpartition's as well: the oracle of that is
        # scikit-learn's own brute Hamming search (the call the reference makes) on the node ids
        from sklearn.neighbors import KNeighborsRegressor

        ids_tr, ids_te = est.transformer_.transform(f["X_train"]), est.transformer_.transform(f["X_test"])
        skl = KNeighborsRegressor(n_neighbors=5, algorithm="brute", metric="hamming",
                                  metric_params={"w": est.hamming_weights_}).fit(ids_tr, f["y_train"])
        for X, ids in ((f["X_test"], ids_te), (None, None)):
            d_, i_ = est.kneighbors(X, use_deterministic_ordering=False)
            sd, si = skl.kneighbors(ids)
            np.testing.assert_array_equal(i_, si)
            np.testing.assert_array_equal(d_, sd)
        assert est.regressor_._last_numpy_tie_rows >= 0
    # the default policy is back: lowest index first
    assert sknnr_amd.get_hamming_tie_policy() == "lowest_index"


@pytest.mark.parametrize("which, reference, atol", [("randomForest", True, 1e-8), ("randomForest", False, 1e-8),
                                                     ("gbnn", True, 1e-8), ("gbnn", False, 1e-2)])
def test_mixed_type_forest_files_exact_under_the_numpy_tie_policy(which, reference, atol, moscow_frames):
    """REF tests/test_regressions.py:125-195 under hamming_tie_policy("numpy"): every row of the reference's four files,
    no tie-class allowance (the mixed RFNN has 100 uniformly weighted trees: 12 / 5 boundary-tie rows); the distance
    tolerances are the reference's own (its target-GBNN case allows 1e-2: "the tree weights are less accurate when using a
    multi-class classification forest")."""
    import sknnr_amd

    f = moscow_frames
    cls = {"randomForest": sknnr_amd.RFNNRegressor, "gbnn": sknnr_amd.GBNNRegressor}[which]
    rf = np.load(os.path.join(REF_DIR, f"test_estimators_with_mixed_type_forests_{'reference' if reference else 'target'}_{which}_.npz"))
    with sknnr_amd.hamming_tie_policy("numpy"):
        est = cls(n_neighbors=5, random_state=42).fit(f["X_train"], f["y_train"], y_fit=mixed_forest_y_fit(f["y_train"]))
        if reference:
            dist, nn = est.kneighbors()
            pred = est.independent_prediction_
        else:
            dist, nn = est.kneighbors(f["X_test"])
            pred = est.predict(f["X_test"])
    np.testing.assert_array_equal(nn, rf["nn"])
    np.testing.assert_allclose(dist, rf["dist"], rtol=1e-5, atol=atol)
    np.testing.assert_allclose(pred, rf["pred"], rtol=1e-5, atol=1e-8)
    if reference:
        assert est.independent_score_ == pytest.approx(float(rf["score"]), rel=1e-5, abs=1e-8)


@pytest.mark.parametrize("name", CASES)
def test_reference_generated_goldens_exact_under_the_numpy_tie_policy(name, N):
    """The fixtures generated by importing the reference (tests/golden/make_golden.py: 1,750 / 3,500 / 700 / 1,050 trees):
    indices equal on every row under the numpy policy, through the raw regressor on the reference's node ids."""
    import sknnr_amd

    g = load_golden(f"moscow_{name}.npz")
    ids_tr, ids_te, w = g["ids_train"].astype(np.float64), g["ids_test"].astype(np.float64), g["hamming_weights"]
    with sknnr_amd.hamming_tie_policy("numpy"):
        reg = sknnr_amd.RawKNNRegressor(n_neighbors=5, algorithm="brute", metric="hamming", metric_params={"w": w})
        reg.fit(ids_tr, np.zeros((len(ids_tr), 1)))
        d, i = reg.kneighbors(ids_te)
        np.testing.assert_array_equal(i, g["kn_tgt_k5_nn"])
        np.testing.assert_allclose(d, g["kn_tgt_k5_dist"], rtol=1e-12)
        d, i = reg.kneighbors()
        np.testing.assert_array_equal(i, g["kn_ref_k5_nn"])
        np.testing.assert_allclose(d, g["kn_ref_k5_dist"], rtol=1e-12)
        d, i = reg.kneighbors(ids_te, n_neighbors=1)
        np.testing.assert_array_equal(i, g["kn_tgt_k1_nn"])
        # tiles of a streamed call go through the same replay, positions carried from tile to tile
        d_s, i_s = reg.kneighbors_chunks(iter([ids_te[:10], ids_te[10:11], ids_te[11:]]))
        np.testing.assert_array_equal(i_s, g["kn_tgt_k5_nn"])


def test_hamming_distance_rows_equal_scipy(N):
    """sknnr_hamming_distances: full float64 distance rows of selected queries, bit-equal to scipy's cdist (the matrix
    the reference's brute search materialises), for given rows and for the index's own rows."""
    from scipy.spatial.distance import cdist

    rng = np.random.default_rng(3)
    ref = rng.integers(0, 9, (777, 37)).astype(np.float64)
    q = rng.integers(0, 9, (100, 37)).astype(np.float64)
    w = rng.random(37) + 0.01
    ix = N.Index(ref)
    ix.set_hamming_weights(w)
    rows = np.array([5, 0, 99, 5, 42], dtype=np.int64)
    np.testing.assert_array_equal(ix.hamming_distances_host(q, rows), cdist(q[rows], ref, "hamming", w=w))
    np.testing.assert_array_equal(ix.hamming_distances_host(None, rows), cdist(ref[rows], ref, "hamming", w=w))
    np.testing.assert_array_equal(ix.hamming_distances_host(q), cdist(q, ref, "hamming", w=w))
    with pytest.raises(N.HipBackendError, match="outside"):
        ix.hamming_distances_host(q, np.array([100], dtype=np.int64))
    ix.close()


def test_gbnn_on_synthetic_rows_matches_the_reference(N, O):
    """The reference's GBNN on 1,200 x 8 synthetic rows (real-valued train-improvement weights): its
    node ids / weights through the HIP search, its predictions from the HIP neighbours."""
    g = load_golden("synth_gbnn.npz")
    ref, q, w, y = g["ids_ref"].astype(np.float64), g["ids_q"].astype(np.float64), g["hamming_weights"], g["y"]
    ix = N.Index(ref, y)
    ix.set_hamming_weights(w)
    dist, idx = ix.kneighbors_host(q, ix.make_opts(5, formula=N.FORMULA_HAMMING))
    ties = assert_hamming_neighbors_match(idx, dist, g["nn"], g["dist"], ref, q, w)
    pred = ix.predict_host(q, ix.make_opts(5, formula=N.FORMULA_HAMMING))
    keep = rows_without(len(q), ties)
    assert keep.sum() >= len(q) - 8, ties  # real-valued tree weights: boundary ties are rare
    np.testing.assert_allclose(pred[keep], g["pred"][keep], rtol=1e-5, atol=1e-8)
    np.testing.assert_array_equal(pred, O.predict(y, dist, idx, "uniform"))
    dist, idx = ix.kneighbors_host(None, ix.make_opts(5, formula=N.FORMULA_HAMMING, exclude_self=True), nq=len(ref))
    assert_hamming_neighbors_match(idx, dist, g["ref_nn"], g["ref_dist"], ref, ref, w, row_offset_self=0)
    ix.close()


def test_forest_weight_validation(moscow_frames):
    """REF _weighted_trees.py:100-136."""
    import sknnr_amd

    f = moscow_frames
    y2 = f["y_train"].iloc[:, :2]
    for bad, msg in (([1.0], "to have length 2"), (["a", "b"], "sequence of numeric"), ([1.0, np.inf], "to be finite"),
                     ([1.0, -1.0], "non-negative"), ([0.0, 0.0], "must be positive")):
        with pytest.raises(ValueError, match=msg):
            sknnr_amd.RFNNRegressor(n_estimators=3, forest_weights=bad).fit(f["X_train"], y2)
    est = sknnr_amd.RFNNRegressor(n_estimators=4, forest_weights=[3.0, 1.0], random_state=0).fit(f["X_train"], y2)
    np.testing.assert_allclose(est.hamming_weights_, np.r_[np.full(4, 0.75 / 4), np.full(4, 0.25 / 4)])
    # y_fit: forests grown on other targets than the ones predicted (REF _base.py:361-374)
    est = sknnr_amd.GBNNRegressor(n_estimators=5, random_state=0).fit(f["X_train"], f["y_train"], y_fit=y2)
    assert est.transformer_.n_forests_ == 2 and est.predict(f["X_test"]).shape == (33, f["y_train"].shape[1])
    with pytest.raises(ValueError, match="Input X contains NaN"):
        bad_x = f["X_test"].to_numpy().copy()
        bad_x[0, 0] = np.nan
        est.kneighbors(bad_x)


@pytest.mark.parametrize("name", ["gnn_d32", "mahalanobis_d64"])
def test_wide_synthetic_estimator_goldens(name):
    """GNN in 32 dimensions (BASELINE C3's space) and Mahalanobis in 64 (C4's), fitted by the reference at
    fixture size (the estimator fixtures were all d = 16)."""
    import sknnr_amd
    from conftest import assert_neighbors_match
    from sknnr_amd import synth

    g = load_golden(f"synth_est_{name}.npz")
    cls, kw, kind, d = {"gnn_d32": (sknnr_amd.GNNRegressor, dict(n_neighbors=7, weights="distance"), "positive", 32),
                        "mahalanobis_d64": (sknnr_amd.MahalanobisKNNRegressor, dict(n_neighbors=5), "linear", 64)}[name]
    x_ref, y, x_q = synth.make_problem(2000, 512, d, t=40, kind=kind)
    est = cls(**kw).fit(x_ref, y)
    assert est.n_features_in_ == int(g["n_features_in_"]) == d
    assert est.regressor_._fit_method == str(g["fit_method"])
    dist, idx = est.kneighbors(x_q)
    assert_neighbors_match(idx, dist, g["nn"], g["dist"])
    np.testing.assert_allclose(est.predict(x_q), g["pred"], rtol=1e-5, atol=1e-8)
    assert est.independent_score_ == pytest.approx(float(g["indep_score"]), rel=1e-6)
    np.testing.assert_allclose(est.independent_prediction_[::8], g["indep_pred_rows"], rtol=1e-5, atol=1e-8)
    st = est.regressor_.engine_.stats()
    assert st["coarse_queries"] > 0 and st["exact_fallbacks"] < 0.02 * st["queries"], st


# ---------------------------------------------------------------------------------------------
# the reference's own tree-estimator tests (REF tests/test_estimators.py:380-499), same inputs and assertions
# ---------------------------------------------------------------------------------------------
def _expected_forest_weights(forest_weights, n_forests):
    if isinstance(forest_weights, str):
        return np.full(n_forests, 1.0 / n_forests)
    arr = np.asarray(forest_weights, dtype=np.float64)
    return arr / arr.sum()


def _tree_estimators():
    import sknnr_amd

    return {"rfnn": sknnr_amd.RFNNRegressor, "gbnn": sknnr_amd.GBNNRegressor}


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
@pytest.mark.parametrize("forest_weights", ["uniform", [0.5, 1.5], (1.0, 2.0)])
def test_tree_estimator_handles_forest_weights(moscow_frames, which, forest_weights):
    """REF tests/test_estimators.py:380-405: the weights of a forest's trees add up to the forest's share."""
    y = moscow_frames["y_all"].iloc[:, :2]
    est = _tree_estimators()[which](forest_weights=forest_weights).fit(moscow_frames["X_all"], y)
    assert hasattr(est.transformer_, "tree_weights_")
    per_forest = est.hamming_weights_.reshape(est.transformer_.n_forests_, -1).sum(axis=1)
    assert np.allclose(per_forest, _expected_forest_weights(forest_weights, est.transformer_.n_forests_), atol=1e-3)


@pytest.mark.parametrize("forest_weights", ["uniform", [0.5, 1.5], (1.0, 2.0)])
def test_gbnn_multiclass_weights(moscow_frames, forest_weights):
    """REF tests/test_estimators.py:408-441: a three-class classification forest holds 3 x n_estimators trees
    whose weights share the forest's weight."""
    import sknnr_amd

    X, y = moscow_frames["X_all"], moscow_frames["y_all"]
    y_fit = y[["Total_BA"]].assign(
        ABGR_CLASS=np.digitize(y.iloc[:, 0], np.percentile(y.iloc[:, 0], [33, 66])).astype(str))
    est = sknnr_amd.GBNNRegressor(forest_weights=forest_weights).fit(X, y, y_fit=y_fit)
    assert hasattr(est.transformer_, "tree_weights_")
    per_block = est.hamming_weights_.reshape(-1, est.transformer_.n_estimators).sum(axis=1)
    n_classes = np.asarray(est.transformer_.n_trees_per_iteration_)
    expected = np.repeat(_expected_forest_weights(forest_weights, est.transformer_.n_forests_) / n_classes, n_classes)
    assert np.allclose(per_block, expected, atol=1e-3)
    # ... and the search over all 400 node-id columns answers (the classification forest's columns included)
    dist, idx = est.kneighbors(X.iloc[:20])
    assert idx.shape == (20, 5) and np.isfinite(dist).all()


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
@pytest.mark.parametrize("forest_weights", ["uniform", [0.5, 1.5], (1.0, 2.0)])
@pytest.mark.parametrize("tree_weighting_method", ["uniform", "train_improvement"])
def test_hamming_weights_sum_to_one(moscow_frames, which, forest_weights, tree_weighting_method):
    """REF tests/test_estimators.py:444-462."""
    n_targets = 1 if forest_weights == "uniform" else len(forest_weights)
    y = moscow_frames["y_all"].iloc[:, :n_targets]
    kwargs = {"tree_weighting_method": tree_weighting_method} if which == "gbnn" else {}
    est = _tree_estimators()[which](forest_weights=forest_weights, **kwargs).fit(moscow_frames["X_all"], y)
    assert np.isclose(est.hamming_weights_.sum(), 1.0)


@pytest.mark.parametrize("which", ["rfnn", "gbnn"])
@pytest.mark.parametrize(
    ("forest_weights", "expected_msg"),
    [
        ([0.5], "Expected `forest_weights` to have length 2"),
        (1, "Expected `forest_weights` to have length 2"),
        ("ab", "`forest_weights` must be a sequence of numeric values"),
        (["a", "b"], "`forest_weights` must be a sequence of numeric values"),
        ([np.inf, 0.5], "Expected elements in `forest_weights` to be finite"),
        ([0.5, np.nan], "Expected elements in `forest_weights` to be finite"),
        ([0.5, -0.5], "Expected elements in `forest_weights` to be non-negative"),
        ([0, 0], "At least one element in `forest_weights` must be positive"),
    ],
    ids=["invalid_length", "numeric_scalar", "non_numeric_scalar", "non_numeric_sequence", "infinite_weight",
         "nan_weight", "negative_weights", "zero_weights"],
)
def test_tree_estimator_raises_on_invalid_forest_weights(moscow_frames, which, forest_weights, expected_msg):
    """REF tests/test_estimators.py:465-499: same inputs, same messages."""
    y = moscow_frames["y_all"].iloc[:, :2]
    with pytest.raises(ValueError, match=expected_msg):
        _tree_estimators()[which](forest_weights=forest_weights).fit(moscow_frames["X_all"], y)
