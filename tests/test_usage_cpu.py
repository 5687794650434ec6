"""Neighbour usage without a device: the numpy model of the contract (tests/_usage.py) on a case worked out by hand, the
value semantics of ``sknnr_amd.NeighborUsage``, and the refusals of ``usage=`` that come before any device work."""

from __future__ import annotations

import pickle

import numpy as np
import pytest

import _usage as U


def test_model_on_the_hand_written_case():
    counts, mx, skipped = U.tally(U.HAND_IDX, U.HAND_DIST, U.HAND_N_REF)
    np.testing.assert_array_equal(counts, U.HAND_COUNTS)
    np.testing.assert_array_equal(mx, U.HAND_MAX)
    assert not np.signbit(mx).any() and skipped == U.HAND_SKIPPED
    assert counts.sum() == U.HAND_IDX.size - skipped
    counts_only, none, _ = U.tally(U.HAND_IDX, None, U.HAND_N_REF)
    np.testing.assert_array_equal(counts_only, U.HAND_COUNTS)
    assert none is None
    # accumulate: counts double, maxima stay; a stored value that is not > 0 (NaN, -1) reads as +0.0
    again, mx2, _ = U.tally(U.HAND_IDX, U.HAND_DIST, U.HAND_N_REF, counts, np.where(mx > 3, mx, [np.nan, -1, 0, 0, 0, 0, -0.0]))
    np.testing.assert_array_equal(again, 2 * U.HAND_COUNTS)
    np.testing.assert_array_equal(mx2, U.HAND_MAX)


def usage_of(counts, mx, ids=None):
    import sknnr_amd

    return sknnr_amd.NeighborUsage()._add(counts, mx, ids)


def test_neighbor_usage_binding_and_numbers():
    import sknnr_amd

    u = sknnr_amd.NeighborUsage()
    assert u.shape is None and repr(u) == "NeighborUsage(unbound)" and u.ids is None
    with pytest.raises(ValueError, match="tallied nothing"):
        u.counts
    u._check(7, 3)  # (unbound: anything goes)
    counts = U.HAND_COUNTS.copy()
    counts[5] = 0  # row 5 never used: the C ABI's maximum for it is 0.0
    mx = U.HAND_MAX.copy()
    mx[5] = 0.0
    u._add(counts, mx)
    assert u.shape == (7, 3) and "n_ref=7, k=3" in repr(u)
    assert u.counts.dtype == np.int64 and u.max_distance.dtype == np.float64
    np.testing.assert_array_equal(u.counts, counts)
    np.testing.assert_array_equal(u.total, counts.sum(1))
    np.testing.assert_array_equal(u.unused, [False] * 5 + [True, False])
    # NaN exactly where total == 0: row 6 was used, at distance +0.0
    np.testing.assert_array_equal(np.isnan(u.max_distance), u.total == 0)
    np.testing.assert_array_equal(u.max_distance[[0, 6]], [6.0, 0.0])
    assert u.n_rows == counts[:, 0].sum() == 8
    with pytest.raises(ValueError, match=r"bound to \(n_ref, k\) = \(7, 3\)"):
        u._check(7, 5)
    with pytest.raises(ValueError, match="bound to"):
        u._add(np.zeros((8, 3), dtype=np.int64), np.zeros(8))
    np.testing.assert_array_equal(u.counts, counts)  # (the refused tally changed nothing)


def test_neighbor_usage_merge_pickle_and_equality():
    import sknnr_amd

    ids = np.arange(7) * 11 + 5
    a = usage_of(U.HAND_COUNTS, U.HAND_MAX, ids)
    b = usage_of(U.HAND_COUNTS[::-1].copy(), U.HAND_MAX[::-1].copy(), ids)
    both = pickle.loads(pickle.dumps(a))
    assert both == a and both is not a and both != b
    np.testing.assert_array_equal(both.ids, ids)
    both += b
    np.testing.assert_array_equal(both.counts, U.HAND_COUNTS + U.HAND_COUNTS[::-1])
    np.testing.assert_array_equal(both.max_distance, np.maximum(U.HAND_MAX, U.HAND_MAX[::-1]))
    assert both.n_rows == a.n_rows + b.n_rows and both != a
    assert a == usage_of(U.HAND_COUNTS, U.HAND_MAX, ids)  # (+= left the right-hand side alone)
    assert a != usage_of(U.HAND_COUNTS, U.HAND_MAX)  # ids are part of the value
    empty = sknnr_amd.NeighborUsage()
    empty += a  # binds
    assert empty == a
    a += sknnr_amd.NeighborUsage()  # an unbound one adds nothing
    assert empty == a
    with pytest.raises(ValueError, match="bound to"):
        a += usage_of(np.zeros((7, 5), dtype=np.int64), np.zeros(7))
    with pytest.raises(TypeError):
        hash(a)
    assert sknnr_amd.NeighborUsage() == sknnr_amd.NeighborUsage() and sknnr_amd.NeighborUsage() != a


class _Fitted:
    """The pieces of a fitted estimator the refusals of ``usage=`` read before any device work."""

    def __new__(cls, weights="uniform", k=5):
        import sknnr_amd

        est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights)
        est._fit_X = np.zeros((12, 3))
        est._y = np.zeros((12, 2))
        est.n_samples_fit_, est.n_features_in_ = 12, 3
        est._fit_method = "brute"
        return est


def test_usage_refusals_need_no_device():
    import sknnr_amd

    tiles = [np.zeros((4, 3))]
    bound_elsewhere = usage_of(np.zeros((12, 3), dtype=np.int64), np.zeros(12))
    est = _Fitted()
    # another k, another n_ref: ValueError before the stream is opened (the engine does not even exist)
    with pytest.raises(ValueError, match=r"bound to \(n_ref, k\) = \(12, 3\)"):
        est.kneighbors_chunks(iter(tiles), usage=bound_elsewhere)
    with pytest.raises(ValueError, match="bound to"):
        est.predict_chunks(iter(tiles), usage=bound_elsewhere)
    with pytest.raises(ValueError, match="bound to"):
        est.kneighbors_chunks(iter(tiles), usage=usage_of(np.zeros((11, 5), dtype=np.int64), np.zeros(11)))
    # a callable runs on the host between the search and the reduction
    with pytest.raises(NotImplementedError, match="usage is not supported with callable weights"):
        _Fitted(weights=lambda d: 1.0 / (1.0 + d)).predict_chunks(iter(tiles), usage=sknnr_amd.NeighborUsage())
    # the host-side tie policies answer tile by tile on the host
    with sknnr_amd.tree_tie_policy("tree"):
        tree = _Fitted()
        tree._fit_method = "kd_tree"
        with pytest.raises(NotImplementedError, match=r"usage is not supported under tree_tie_policy\('tree'\)"):
            tree.kneighbors_chunks(iter(tiles), usage=sknnr_amd.NeighborUsage())
        with pytest.raises(NotImplementedError, match="usage is not supported under"):
            tree.predict_chunks(iter(tiles), usage=sknnr_amd.NeighborUsage())
    with sknnr_amd.hamming_tie_policy("numpy"):
        ham = _Fitted()
        ham.effective_metric_ = "hamming"
        with pytest.raises(NotImplementedError, match=r"usage is not supported under hamming_tie_policy\('numpy'\)"):
            ham.predict_chunks(iter(tiles), usage=sknnr_amd.NeighborUsage())
