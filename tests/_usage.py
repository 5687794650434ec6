"""The neighbour-usage contract of include/sknnr_hip.h ("Neighbour usage") restated in numpy: the model every usage test
compares the device with."""

from __future__ import annotations

import numpy as np


def tally(idx, dist, n_ref, counts=None, max_dist=None):
    """``(counts, max_dist, skipped)`` of ``idx`` ``(n, k)`` / ``dist`` ``(n, k)`` or None, in the C ABI's form (an unused
    row's maximum is 0.0); ``counts`` / ``max_dist``: what to accumulate on (``accumulate = 1``)."""
    idx = np.asarray(idx, dtype=np.int64)
    k = idx.shape[1]
    ok = (idx >= 0) & (idx < n_ref)  # anything else is skipped, never dereferenced
    out = np.zeros((n_ref, k), dtype=np.int64) if counts is None else counts.copy()
    for j in range(k):
        out[:, j] += np.bincount(idx[ok[:, j], j], minlength=n_ref)
    mx = None
    if dist is not None:
        mx = np.zeros(n_ref) if max_dist is None else np.where(max_dist > 0, max_dist, 0.0)
        d = np.asarray(dist, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            d = np.where(d > 0, d, 0.0)  # 0.0, -0.0, negatives and NaN count as +0.0
        np.maximum.at(mx, idx[ok], d[ok])
    return out, mx, int((~ok).sum())


def rows_form(a, bands):
    """A streamed call's ``(k, N)`` band-first result as the ``(N, k)`` rows the model reads."""
    return np.ascontiguousarray(np.asarray(a).T) if bands else np.asarray(a)


# The hand-written case: n_ref = 7, k = 3, 10 rows -- an all-negative (fill) row, an entry == n_ref, one far outside, a
# negative one in a live row, the same index twice and three times in one row, and distances 0.0, -0.0 and NaN.
HAND_N_REF = 7
HAND_IDX = np.array([[0, 1, 2], [0, 2, 1], [-1, -1, -1], [3, 3, 4], [7, 0, 1],
                     [6, 5, 4], [0, 1, 2], [4, 0, -5], [2, 2, 2], [1, 4, 100]], dtype=np.int64)
HAND_DIST = np.array([[0.5, 1.0, 1.5], [0.0, 2.0, 0.25], [np.nan, np.nan, np.nan], [1.0, 3.0, 0.5], [9.0, 0.75, -0.0],
                      [np.nan, 0.125, 4.0], [0.5, 1.0, 2.5], [0.25, 6.0, 1.0], [0.0, -0.0, 0.0], [7.0, 0.5, 8.0]])
# worked out by hand: column j of HAND_IDX counted per reference row; row 6 is used once, at a NaN distance
HAND_COUNTS = np.array([[3, 2, 0], [1, 2, 2], [1, 2, 3], [1, 1, 0], [1, 1, 2], [0, 1, 0], [1, 0, 0]], dtype=np.int64)
HAND_MAX = np.array([6.0, 7.0, 2.5, 3.0, 4.0, 0.125, 0.0])
HAND_SKIPPED = 6  # the fill row's three, 7, -5 and 100 (whose distances 9.0, 1.0 and 8.0 must not show anywhere)
