"""The leave-group-out contract (include/sknnr_hip.h, sknnr_kneighbors_grouped) in numpy over the oracle.

For fitted row i the candidates are the fitted rows r with ``codes[r] != codes[i]``.  Each pair has the float64 value
``kneighbors`` ranks it by -- what ``oracle.argkmin(..., squared=True)`` or ``oracle.argkmin_hamming`` returns.  The
answer: the k candidates smallest by (value, r), their distances (``sqrt`` for the Euclidean formulas), and, with the
deterministic ordering, ``oracle.deterministic_reorder`` at the row's global number.  No heap history: exact ties at the
k-th value go to the lower index.
"""

from __future__ import annotations

import numpy as np

from oracle import oracle


def value_rows(fit, rows, formula="expanded", w=None):
    """``(len(rows), n_ref)`` float64: the value of every (rows[i], r) pair under ``formula``."""
    fit = np.ascontiguousarray(fit, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    n_ref = fit.shape[0]
    if formula == "hamming":
        val, idx = oracle.argkmin_hamming(fit[rows], fit, w, n_ref)
    else:
        val, idx = oracle.argkmin(fit[rows], fit, n_ref, formula, squared=True)
    full = np.empty_like(val)
    np.put_along_axis(full, idx, val, axis=1)  # (every index appears once in a row of n_ref neighbours)
    return full


def ranked_candidates(full, rows, codes, kmax):
    """Steps 2 and 3 of the model: same-code entries masked, then per row the ``kmax`` candidates smallest by
    (value, index).  Returns ``(values, indices)``; a row with fewer candidates shows ``inf`` values at its end."""
    rows = np.asarray(rows, dtype=np.int64)
    codes = np.asarray(codes)
    val = np.where(codes[None, :] == codes[rows][:, None], np.inf, full)
    ids = np.broadcast_to(np.arange(full.shape[1]), full.shape)
    order = np.lexsort((ids, val), axis=1)[:, :kmax]
    return np.take_along_axis(val, order, axis=1), order.astype(np.int64)


def finish(val, idx, rows, *, hamming=False, deterministic=True, decimals=10):
    """Step 4 on the ``k`` ranked candidates of every row: distances, then the reorder at each row's global number
    (one call when ``rows`` are consecutive, else row by row)."""
    rows = np.asarray(rows, dtype=np.int64)
    n = len(rows)
    assert np.isfinite(val).all(), "a row has fewer candidates than neighbours"
    dist = val.copy() if hamming else np.sqrt(np.maximum(val, 0.0))
    idx = idx.copy()
    if deterministic and n:
        if np.array_equal(rows, np.arange(rows[0], rows[0] + n)):
            dist, idx = oracle.deterministic_reorder(dist, idx, decimals, row_offset=int(rows[0]))
        else:
            for i, r in enumerate(rows):
                dist[i : i + 1], idx[i : i + 1] = oracle.deterministic_reorder(dist[i : i + 1], idx[i : i + 1], decimals,
                                                                               row_offset=int(r))
    return dist, idx


def grouped_from_values(full, rows, codes, k, *, hamming=False, deterministic=True, decimals=10):
    """Steps 2 - 4 of the model on value rows already computed."""
    val, idx = ranked_candidates(full, rows, codes, k)
    return finish(val, idx, rows, hamming=hamming, deterministic=deterministic, decimals=decimals)


def grouped_kneighbors(fit, codes, k, *, formula="expanded", w=None, rows=None, deterministic=True, decimals=10):
    """The model: ``(dist, idx)`` of fitted rows ``rows`` (default: all) under the group codes ``codes``."""
    fit = np.asarray(fit)
    rows = np.arange(fit.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    full = value_rows(fit, rows, formula, w)
    return grouped_from_values(full, rows, codes, k, hamming=formula == "hamming", deterministic=deterministic,
                               decimals=decimals)


def boundary_tie_rows(full, rows, k):
    """Rows whose k-th and (k+1)-th smallest values among the OTHER rows are equal (singleton groups)."""
    rows = np.asarray(rows, dtype=np.int64)
    val = full.copy()
    val[np.arange(len(rows)), rows] = np.inf
    srt = np.sort(val, axis=1)
    return np.nonzero(srt[:, k - 1] == srt[:, k])[0]


# ---- group laws of the tests ----
def singletons(n):
    return np.arange(n, dtype=np.int32)


def pairs(n):
    return (np.arange(n) // 2).astype(np.int32)


def random_sizes(n, lo, hi, seed):
    """Groups of ``lo .. hi`` rows each, their members scattered over the rows."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(lo, hi + 1)))
    codes = np.repeat(np.arange(len(sizes)), sizes)[:n]
    return rng.permutation(codes).astype(np.int32)


def two_piece(n, piece=5):
    """One group holding the first and the last ``piece`` rows; every other row a group of its own."""
    codes = np.arange(n, dtype=np.int32)
    codes[:piece] = codes[n - piece :] = n
    return codes


def one_big_group(n, first):
    """Rows ``first .. n - 1`` are one group; the rows before them groups of their own."""
    codes = np.arange(n, dtype=np.int32)
    codes[first:] = first
    return codes
