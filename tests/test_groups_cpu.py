"""Leave-group-out neighbours without a device: the numpy model (tests/_groups.py) against a hand case and against
``oracle.kneighbors(None)``, the label coding and its refusals, and the new C symbols on a NULL handle."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import _groups
from sknnr_amd import synth

TIE_FREE_SHAPES = [(700, 13, 5), (700, 32, 5), (37, 3, 1), (1100, 8, 9)]  # (n, d, k): make_features(n, d, seed=3)


def test_hand_case():
    """Six rows on a line at 0, 1, 3, 6, 10, 15, groups [0,0,1,1,2,2], k = 2.
    row 0 (group 0): others 3 (d 3), 6 (6), 10, 15        -> rows 2, 3
    row 1 (group 0): 3 (2), 6 (5)                         -> rows 2, 3
    row 2 (group 1): 1 (2), 0 (3), 10 (7), 15             -> rows 1, 0
    row 3 (group 1): 10 (4), 1 (5), 0 (6), 15 (9)         -> rows 4, 1
    row 4 (group 2): 6 (4), 3 (7), 1 (9), 0 (10)          -> rows 3, 2
    row 5 (group 2): 6 (9), 3 (12)                        -> rows 3, 2
    No two kept distances of a row are equal, so the reorder changes nothing."""
    fit = np.array([[0.0], [1.0], [3.0], [6.0], [10.0], [15.0]])
    codes = np.array([0, 0, 1, 1, 2, 2])
    want_idx = np.array([[2, 3], [2, 3], [1, 0], [4, 1], [3, 2], [3, 2]])
    want_dist = np.array([[3.0, 6.0], [2.0, 5.0], [2.0, 3.0], [4.0, 5.0], [4.0, 7.0], [9.0, 12.0]])
    for formula in ("direct", "expanded"):
        for det in (True, False):
            dist, idx = _groups.grouped_kneighbors(fit, codes, 2, formula=formula, deterministic=det)
            np.testing.assert_array_equal(idx, want_idx)
            np.testing.assert_array_equal(dist, want_dist)  # (small integers: both formulas are exact)


@pytest.mark.parametrize("formula", ["expanded", "direct"])
@pytest.mark.parametrize("n,d,k", TIE_FREE_SHAPES)
def test_singleton_groups_are_kneighbors_none(n, d, k, formula):
    from oracle import oracle

    fit = synth.make_features(n, d, seed=3)
    rows = np.arange(n)
    full = _groups.value_rows(fit, rows, formula)
    assert _groups.boundary_tie_rows(full, rows, k).size == 0  # no row has equal k-th and (k+1)-th values
    dist, idx = _groups.grouped_from_values(full, rows, _groups.singletons(n), k)
    od, oi = oracle.kneighbors(fit, None, k, formula)
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(dist, od)


def test_model_skips_groups_on_a_lattice():
    rng = np.random.default_rng(5)
    fit = rng.integers(0, 3, (700, 4)).astype(np.float64)
    codes = rng.integers(0, 200, 700)
    for formula in ("expanded", "direct"):
        dist, idx = _groups.grouped_kneighbors(fit, codes, 5, formula=formula)
        assert not (codes[idx] == codes[:, None]).any()


def test_label_coding():
    from sknnr_amd._base import normalize_groups

    codes = normalize_groups([7, 3, 7, 9], 4)
    assert codes.dtype == np.int32 and codes.tolist() == [1, 0, 1, 2]
    assert normalize_groups(np.array(["b", "a", "b", "c"]), 4).tolist() == [1, 0, 1, 2]
    assert normalize_groups(np.array([2.5, 1.0, 2.5]), 3).tolist() == [1, 0, 1]
    pd = pytest.importorskip("pandas")
    assert normalize_groups(pd.Series(["p2", "p1", "p2"], index=[10, 11, 12]), 3).tolist() == [1, 0, 1]


def test_label_refusals():
    from sknnr_amd._base import normalize_groups

    with pytest.raises(ValueError, match=r"one label per fitted row \(4\), got 3"):
        normalize_groups([0, 1, 2], 4)
    with pytest.raises(ValueError, match=r"1-D .* got an array of shape \(2, 2\)"):
        normalize_groups(np.zeros((2, 2)), 4)
    with pytest.raises(ValueError, match=r"must not hold NaN, got 1 NaN"):
        normalize_groups([0.0, np.nan, 1.0], 3)
    with pytest.raises(ValueError, match=r"at least two groups, got the single group"):
        normalize_groups([4, 4, 4], 3)


def test_estimator_refuses_before_the_device():
    """An estimator whose engine is never built: the refusals come first."""
    from sknnr_amd import RawKNNRegressor, hamming_tie_policy, tree_tie_policy

    est = RawKNNRegressor(n_neighbors=2)
    est._fit_X = np.zeros((4, 3))
    est._y = np.zeros(4)
    est.n_samples_fit_ = 4
    est._fit_method = "kd_tree"
    est.effective_metric_ = "euclidean"
    est._engine = None
    for call in (est.independent_kneighbors, est.independent_predict, est.independent_summarize, est.independent_score):
        with pytest.raises(ValueError, match="one label per fitted row"):
            call([0, 1])
        with pytest.raises(ValueError, match="single group"):
            call(["a"] * 4)
    with pytest.raises(TypeError, match="n_neighbors does not take"):
        est.independent_kneighbors([0, 1, 2, 3], n_neighbors=1.5)
    with tree_tie_policy("tree"):
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            est.independent_kneighbors([0, 1, 2, 3])
    est.effective_metric_ = "hamming"
    with hamming_tie_policy("numpy"):
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            est.independent_predict([0, 1, 2, 3])
    assert est._engine is None


def test_new_symbols_on_a_null_handle():
    from sknnr_amd import _build, _native

    import os

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    lib = _native.load()
    codes = (ctypes.c_int32 * 2)(0, 1)
    assert lib.sknnr_index_set_groups(None, codes, 2) == _native.ERR_INVALID
    assert b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_kneighbors_grouped(None, 1, None, None, None, 0, None) == _native.ERR_INVALID
    assert lib.sknnr_debug_last_grouped(None, (ctypes.c_int64 * 8)()) == _native.ERR_INVALID
    for name in ("sknnr_index_set_groups", "sknnr_kneighbors_grouped", "sknnr_debug_last_grouped"):
        assert name in _native.EXPORTED_SYMBOLS
