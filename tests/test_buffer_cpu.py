"""Buffered leave-out without a device: the numpy model (tests/_buffer.py) against a hand case and a brute-force double
loop, ``normalize_buffer`` and its refusals, an estimator that refuses before device work, and the new C symbols on a
NULL handle."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import _buffer
import _groups
from sknnr_amd import synth


def test_hand_case():
    """Six rows on a line: the features ARE the positions 0, 1, 3, 6, 10, 15; radius 3, k = 2.
    row 0 (at 0):  excluded 0, 1, 3 (d 0, 1, 3 <= 3)    candidates 6 (6), 10 (10), 15      -> rows 3, 4
    row 1 (at 1):  excluded 0, 1, 3                     candidates 6 (5), 10 (9)           -> rows 3, 4
    row 2 (at 3):  excluded 0, 1, 3, 6 (d 3 <= 3)       candidates 10 (7), 15 (12)         -> rows 4, 5
    row 3 (at 6):  excluded 3, 6                        candidates 10 (4), 1 (5), 0 (6)    -> rows 4, 1
    row 4 (at 10): excluded 10                          candidates 6 (4), 15 (5)           -> rows 3, 5
    row 5 (at 15): excluded 15                          candidates 10 (5), 6 (9)           -> rows 4, 3
    With groups [0, 0, 2, 2, 1, 0] as well, no row shares a group with either of its two: nothing changes."""
    fit = np.array([[0.0], [1.0], [3.0], [6.0], [10.0], [15.0]])
    want_idx = np.array([[3, 4], [3, 4], [4, 5], [4, 1], [3, 5], [4, 3]])
    want_dist = np.array([[6.0, 10.0], [5.0, 9.0], [7.0, 12.0], [4.0, 5.0], [4.0, 5.0], [5.0, 9.0]])
    np.testing.assert_array_equal(_buffer.excluded_counts(fit, 3.0), [3, 3, 4, 2, 1, 1])
    for formula in ("direct", "expanded"):
        for det in (True, False):
            for codes in (None, np.array([0, 0, 2, 2, 1, 0])):
                dist, idx = _buffer.buffered_kneighbors(fit, fit, 3.0, 2, codes=codes, formula=formula, deterministic=det)
                np.testing.assert_array_equal(idx, want_idx)
                np.testing.assert_array_equal(dist, want_dist)  # (small integers: both formulas are exact)
    np.testing.assert_array_equal(_buffer.excluded_counts(fit, 3.0, np.array([0, 0, 0, 0, 1, 0])), [5, 5, 5, 5, 1, 5])
    # just below 3: the rows at distance exactly 3 come back
    np.testing.assert_array_equal(_buffer.excluded_counts(fit, math.nextafter(3.0, 0.0)), [2, 3, 2, 1, 1, 1])
    np.testing.assert_array_equal(_buffer.excluded_counts(fit, 0.0), [1] * 6)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_model_against_a_double_loop(c):
    """Python floats are float64 and every ``*``, ``+``, ``-`` rounds once: the loop is the contract, letter by letter."""
    n, d, k = 60, 3, 4
    fit = synth.make_features(n, d, seed=3)
    coords = _buffer.uniform_square(n, c, seed=c)
    radius = _buffer.radius_for(n, c, 6.0)
    codes = _groups.random_sizes(n, 1, 4, seed=n)
    r2 = radius * radius
    p = [[float(v) for v in row] + [0.0] * (3 - c) for row in coords]
    for use_codes in (None, codes):
        want_mask = np.zeros((n, n), dtype=bool)
        want_idx = np.zeros((n, k), dtype=np.int64)
        for i in range(n):
            cand = []
            for r in range(n):
                dx, dy, dz = p[i][0] - p[r][0], p[i][1] - p[r][1], p[i][2] - p[r][2]
                g = (dx * dx + dy * dy) + dz * dz
                out = g <= r2 or (use_codes is not None and use_codes[r] == use_codes[i])
                want_mask[i, r] = out
                if not out:
                    t = fit[i] - fit[r]
                    v = 0.0
                    for e in t:  # the direct formula: sum of squares in column order
                        v = v + float(e) * float(e)
                    cand.append((v, r))
            cand.sort()
            want_idx[i] = [r for _, r in cand[:k]]
        np.testing.assert_array_equal(_buffer.excluded_mask(coords, radius, np.arange(n), use_codes), want_mask)
        np.testing.assert_array_equal(_buffer.excluded_counts(coords, radius, use_codes), want_mask.sum(axis=1))
        assert want_mask.diagonal().all() and 2.0 < want_mask.sum(axis=1).mean() < 12.0
        _, idx = _buffer.buffered_kneighbors(fit, coords, radius, k, codes=use_codes, formula="direct", deterministic=False)
        np.testing.assert_array_equal(idx, want_idx)
        sub = np.array([7, 31, 59])
        _, part = _buffer.buffered_kneighbors(fit, coords, radius, k, codes=use_codes, formula="direct", rows=sub,
                                              deterministic=False)
        np.testing.assert_array_equal(part, want_idx[sub])


def test_missing_columns_add_positive_zero():
    coords = _buffer.uniform_square(50, 1, seed=4)
    padded = np.concatenate([coords, np.zeros((50, 2))], axis=1)
    rows = np.arange(50)
    np.testing.assert_array_equal(_buffer.excluded_mask(coords, 0.07, rows), _buffer.excluded_mask(padded, 0.07, rows))


def test_lattice_counts_in_integers():
    n, width = 37, 6
    coords = _buffer.lattice(n, width)
    plus = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]
    diag = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    np.testing.assert_array_equal(_buffer.excluded_counts(coords, 1.0), _buffer.lattice_counts(n, width, plus))
    np.testing.assert_array_equal(_buffer.excluded_counts(coords, math.sqrt(2.0)), _buffer.lattice_counts(n, width, plus + diag))
    np.testing.assert_array_equal(_buffer.excluded_counts(coords, math.nextafter(math.sqrt(2.0), 0.0)),
                                  _buffer.lattice_counts(n, width, plus))
    assert math.sqrt(2.0) * math.sqrt(2.0) > 2.0 > math.nextafter(math.sqrt(2.0), 0.0) ** 2


def test_position_laws():
    n = 700
    counts = _buffer.excluded_counts(_buffer.uniform_square(n, 2, seed=1), _buffer.radius_for(n, 2))
    assert 3.0 < counts.mean() < 7.0
    pairs = _buffer.colocated_pairs(n, seed=1)
    np.testing.assert_array_equal(_buffer.excluded_counts(pairs, 0.0), np.full(n, 2))
    coords, who = _buffer.cluster(n, 600, 0.05, seed=1)
    counts = _buffer.excluded_counts(coords, 0.05)
    assert (counts[who] == 600).all() and counts.max() == 600


def test_normalize_buffer():
    from sknnr_amd._base import normalize_buffer

    c, r = normalize_buffer(([[0, 1], [2, 3], [4, 5]], 2), 3)
    assert c.dtype == np.float64 and c.shape == (3, 2) and c.flags.c_contiguous and r == 2.0 and isinstance(r, float)
    c, r = normalize_buffer([np.arange(4), np.float32(0.5)], 4)
    assert c.shape == (4, 1) and r == 0.5
    c, _ = normalize_buffer((np.zeros((5, 3), dtype=np.float32, order="F"), 0), 5)
    assert c.shape == (5, 3) and c.dtype == np.float64 and c.flags.c_contiguous
    pd = pytest.importorskip("pandas")
    frame = pd.DataFrame({"X": [1.0, 2.0, 3.0], "Y": [4, 5, 6]}, index=[10, 11, 12])
    c, r = normalize_buffer((frame[["X", "Y"]], 5000.0), 3)
    np.testing.assert_array_equal(c, [[1.0, 4.0], [2.0, 5.0], [3.0, 6.0]])
    assert r == 5000.0


def test_normalize_buffer_refusals():
    from sknnr_amd._base import normalize_buffer

    ok = np.zeros((4, 2))
    with pytest.raises(ValueError, match=r"a pair \(coords, radius\)"):
        normalize_buffer(ok, 4)
    with pytest.raises(ValueError, match=r"a pair \(coords, radius\), got tuple of length 3"):
        normalize_buffer((ok, 1.0, 2.0), 4)
    with pytest.raises(ValueError, match=r"one row per fitted row \(4\), got 3"):
        normalize_buffer((ok[:3], 1.0), 4)
    with pytest.raises(ValueError, match="1 to 3 columns, got 4"):
        normalize_buffer((np.zeros((4, 4)), 1.0), 4)
    with pytest.raises(ValueError, match="1 to 3 columns, got 0"):
        normalize_buffer((np.zeros((4, 0)), 1.0), 4)
    with pytest.raises(ValueError, match=r"2-D .* got an array of shape \(4, 2, 1\)"):
        normalize_buffer((np.zeros((4, 2, 1)), 1.0), 4)
    for bad in (np.nan, np.inf, -np.inf):
        pos = ok.copy()
        pos[2, 1] = bad
        with pytest.raises(ValueError, match="positions must be finite, got 1 values"):
            normalize_buffer((pos, 1.0), 4)
    with pytest.raises(ValueError, match="positions must be numbers"):
        normalize_buffer((np.array([["a", "b"]] * 4), 1.0), 4)
    for bad in (-1.0, -1e-300, np.nan, np.inf):
        with pytest.raises(ValueError, match="radius must be finite and >= 0"):
            normalize_buffer((ok, bad), 4)
    for bad in ([1.0], np.ones(2), "3", None, (1.0, 2.0)):
        with pytest.raises(ValueError, match="radius must be a scalar"):
            normalize_buffer((ok, bad), 4)


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
    good = (np.zeros((4, 2)), 1.0)
    calls = (est.independent_kneighbors, est.independent_predict, est.independent_summarize, est.independent_score,
             est.independent_neighbor_usage)
    for call in calls:
        with pytest.raises(ValueError, match="one row per fitted row"):
            call(buffer=(np.zeros((3, 2)), 1.0))
        with pytest.raises(ValueError, match="radius must be finite"):
            call(buffer=(np.zeros((4, 2)), -1.0))
        with pytest.raises(ValueError, match="one label per fitted row"):
            call([0, 1], buffer=good)
        with pytest.raises(ValueError, match="single group"):
            call(["a"] * 4, buffer=good)
        # neither mask: what normalize_groups(None, ...) raises
        with pytest.raises(ValueError, match=r"groups must be 1-D with one label per fitted row, got an array of shape \(\)"):
            call()
    with pytest.raises(ValueError, match="1 to 3 columns"):
        est.buffer_counts((np.zeros((4, 5)), 1.0))
    with pytest.raises(ValueError, match="needs buffer="):
        est.buffer_counts(None)
    with pytest.raises(TypeError, match="n_neighbors does not take"):
        est.independent_kneighbors(buffer=good, n_neighbors=1.5)
    with tree_tie_policy("tree"):
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            est.independent_kneighbors(buffer=good)
    est.effective_metric_ = "hamming"
    with hamming_tie_policy("numpy"):
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            est.independent_predict(buffer=good)
        with pytest.raises(NotImplementedError, match="independent_kneighbors with groups"):
            est.buffer_counts(good)
    assert est._engine is None


def test_new_symbols_on_a_null_handle():
    import os

    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    lib = _native.load()
    coords = (ctypes.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    assert lib.sknnr_index_set_buffer(None, coords, 2, 2, 1.0) == _native.ERR_INVALID
    assert b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_buffer_counts(None, (ctypes.c_int64 * 2)(), 0, None) == _native.ERR_INVALID
    assert lib.sknnr_debug_last_buffer(None, (ctypes.c_int64 * 8)()) == _native.ERR_INVALID
    for name in ("sknnr_index_set_buffer", "sknnr_buffer_counts", "sknnr_debug_last_buffer"):
        assert name in _native.EXPORTED_SYMBOLS
