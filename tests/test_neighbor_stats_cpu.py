"""The per-target neighbour summaries without a device: the numpy restatement (tests/_neighbor_stats.py) against
scikit-learn's ``KNeighborsClassifier`` and against a table computed by hand, and every refusal that needs no device."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import _neighbor_stats as NS


# ---- restated `mode` against scikit-learn ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    rng = np.random.default_rng(20260112)
    X = rng.integers(0, 4, size=(300, 3)).astype(np.float64)
    Q = rng.integers(0, 4, size=(3000, 3)).astype(np.float64)
    y = np.stack([3 * rng.integers(0, 5, size=300) - 2, rng.integers(0, 2, size=300)], axis=1).astype(np.float64)
    return X, Q, y


@pytest.mark.parametrize("algorithm", ["brute", "kd_tree"])
@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("k", [1, 2, 5, 8, 16, 130])
def test_restated_mode_is_scikit_learns_classifier(lattice, algorithm, weights, k):
    from sklearn.neighbors import KNeighborsClassifier

    X, Q, y = lattice
    clf = KNeighborsClassifier(n_neighbors=k, algorithm=algorithm, weights=weights).fit(X, y)
    dist, idx = clf.kneighbors(Q)
    assert (dist == 0).any() and (k == 1 or (np.diff(dist, axis=1) == 0).any()), "the lattice gives zero and tied distances"
    want = clf.predict(Q)
    got = NS.summarize(y, dist, idx, None, weights, ["mode", "mode"])
    np.testing.assert_array_equal(got, want)


# ---- a table computed by hand -----------------------------------------------------------------------------------------------
Y = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 20.0], [7.0, 30.0], [7.0, 10.0]])
IDX = np.array([[0, 1, 2], [3, 4, 0], [2, 1, 3], [4, 2, 0]])
DIST = np.array([[1.0, 2.0, 4.0], [0.5, 0.5, 1.0], [0.0, 1.0, 2.0], [1.0, 1.0, 2.0]])


def test_hand_computed_uniform():
    got = NS.summarize(Y, DIST, IDX, None, "uniform", ["std", "mode"])
    # column 0 values: [1,2,4] [7,7,1] [4,2,7] [7,4,1]; population std
    means = np.array([7 / 3, 5.0, 13 / 3, 4.0])
    var = np.array([((1 - 7 / 3)**2 + (2 - 7 / 3)**2 + (4 - 7 / 3)**2) / 3, (4 + 4 + 16) / 3,
                    ((4 - 13 / 3)**2 + (2 - 13 / 3)**2 + (7 - 13 / 3)**2) / 3, (9 + 0 + 9) / 3])
    np.testing.assert_allclose(got[:, 0], np.sqrt(var), rtol=1e-14)
    assert got[1, 0] == np.sqrt(8.0) and got[3, 0] == np.sqrt(6.0) and means[1] == 5.0
    # column 1 labels: [10,20,20] -> 20; [30,10,10] -> 10; [20,20,30] -> 20; [10,20,10] -> 10
    np.testing.assert_array_equal(got[:, 1], [20.0, 10.0, 20.0, 10.0])
    got = NS.summarize(Y, DIST, IDX, None, "uniform", ["min", "max"])
    np.testing.assert_array_equal(got, [[1.0, 20.0], [1.0, 30.0], [2.0, 30.0], [1.0, 20.0]])
    got = NS.summarize(Y, DIST, IDX, None, "uniform", ["nearest", "nearest"])
    np.testing.assert_array_equal(got, [[1.0, 10.0], [7.0, 30.0], [4.0, 20.0], [7.0, 10.0]])


def test_hand_computed_distance_tie_and_zero_row():
    got = NS.summarize(Y, DIST, IDX, None, "distance", ["mode", "mode"])
    # row 0, column 1: 10 has 1/1, 20 has 1/2 + 1/4 -> 10.  column 0: 1 has the largest weight
    # row 1, column 1: 30 has 2, 10 has 2 + 1 -> 10.  column 0: 7 has 4, 1 has 1 -> 7
    # row 2 holds d == 0: only its first neighbour (row 2: 4.0, 20.0) votes
    # row 3, column 1: 10 has 1 + 1/2, 20 has 1 -> 10.  column 0: 7 and 4 tie at 1.0 -> the smaller label, 4
    np.testing.assert_array_equal(got, [[1.0, 10.0], [7.0, 10.0], [4.0, 20.0], [4.0, 10.0]])
    assert NS.top_vote_tied(Y[IDX, 0], NS.weights_of(DIST, IDX, None, "distance")).tolist() == [False, False, False, True]
    # the zero row: mean and nearest are that neighbour's value, std is 0
    got = NS.summarize(Y, DIST, IDX, None, "distance", ["std", "mean"])
    assert got[2, 0] == 0.0 and got[2, 1] == 20.0
    # row 1, column 0: weights (2, 2, 1), values (7, 7, 1): m = 29 / 5, var = (2 * 1.44 + 2 * 1.44 + 23.04) / 5
    np.testing.assert_allclose(got[1, 0], np.sqrt((4 * 1.2**2 + 4.8**2) / 5), rtol=1e-14)
    # a uniform tie between two labels: [1, 2, 4] has three labels with one vote each -> the smallest
    assert NS.summarize(Y, DIST, IDX, None, "uniform", ["mode", "mean"])[0, 0] == 1.0


def test_all_zero_votes_give_nan():
    w = np.zeros((4, 3))
    w[1] = [0.0, 0.0, 2.0]
    got = NS.summarize(Y, DIST, IDX, w, "explicit", ["mode", "nearest"])
    assert np.isnan(got[[0, 2, 3], 0]).all() and got[1, 0] == 1.0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_statistic_names_are_validated_before_any_device_work():
    from sknnr_amd._base import normalize_statistic

    np.testing.assert_array_equal(normalize_statistic("mode", 3), [1, 1, 1])
    np.testing.assert_array_equal(normalize_statistic(["mean", "std", "nearest"], 3), [0, 5, 4])
    np.testing.assert_array_equal(normalize_statistic(("min", "max"), 2), [2, 3])
    assert normalize_statistic("mean", 1).dtype == np.int32
    with pytest.raises(ValueError, match="unknown statistic 'median'"):
        normalize_statistic("median", 2)
    with pytest.raises(ValueError, match="unknown statistic 'Mode'"):
        normalize_statistic(["mean", "Mode"], 2)
    with pytest.raises(ValueError, match="one name per target \\(3\\), got 2"):
        normalize_statistic(["mean", "mode"], 3)
    with pytest.raises(ValueError, match="one name per target \\(1\\), got 0"):
        normalize_statistic([], 1)
    with pytest.raises(ValueError, match="must be strings"):
        normalize_statistic(["mean", 1], 2)
    with pytest.raises(ValueError, match="must be strings"):
        normalize_statistic([None, "mean"], 2)
    with pytest.raises(ValueError, match="a name or a sequence of names"):
        normalize_statistic(5, 2)


def test_statistic_codes_match_the_header():
    import os
    import re

    from sknnr_amd import _native

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sknnr_hip.h")).read()
    body = re.search(r"enum sknnr_statistic \{(.*?)\};", header, re.S).group(1)
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"SKNNR_STAT_(\w+) = (\d+)", body)}
    assert codes == _native.STATISTICS == NS.CODES


def test_argument_errors_without_touching_a_device():
    from sknnr_amd import _native

    lib = _native.load(build_if_missing=True)
    INV = _native.ERR_INVALID
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    stat = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    assert lib.sknnr_summarize_from_neighbors(None, p, p, None, 4, 3, 0, stat, p, 0, None) == INV
    assert b"index is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_summarize(None, p, 4, None, stat, p, None, None, 0, None) == INV
    assert b"index is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_stream_set_statistics(None, stat, 4) == INV and b"stream is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_debug_last_summary(None, (ctypes.c_int64 * 8)()) == INV
