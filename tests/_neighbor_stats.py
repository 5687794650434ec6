"""The numpy restatement of the per-target neighbour summaries (include/sknnr_hip.h, ``enum sknnr_statistic``), from
``(y, dist, idx, w, mode)``.  Every sum is a plain ``np.sum(..., axis=1)`` over a C-contiguous ``(nq, k)`` array, so that
numpy itself supplies the summation order (its pairwise sum); ``mean`` is scikit-learn's own ``KNeighborsRegressor.predict``
on those neighbours (tests/_predict_ref.py).  Shared by test_neighbor_stats_cpu.py, test_neighbor_stats_kernels_gpu.py and
test_neighbor_summary_gpu.py."""

from __future__ import annotations

import numpy as np

import _predict_ref as PR

STATISTICS = ("mean", "mode", "min", "max", "nearest", "std")
CODES = {name: code for code, name in enumerate(STATISTICS)}


def weights_of(dist, idx, w, mode):
    """The ``(nq, k)`` float64 weights of ``predict``: ``mode`` "uniform" (ones), "distance" (scikit-learn's
    ``_get_weights``: ``1 / d``, a row holding ``d == 0`` becomes its 0 / 1 mask) or "explicit" (``w``)."""
    if mode == "uniform":
        return np.ones(np.shape(idx), dtype=np.float64)
    if mode == "distance":
        with np.errstate(divide="ignore"):
            ww = 1.0 / np.asarray(dist, dtype=np.float64)
        inf_mask = np.isinf(ww)
        inf_row = np.any(inf_mask, axis=1)
        ww[inf_row] = inf_mask[inf_row]
        return np.ascontiguousarray(ww)
    assert mode == "explicit"
    return np.ascontiguousarray(w, dtype=np.float64)


def _sklearn_weights(w, mode):
    return (lambda d: w) if mode == "explicit" else mode


def mean_of(y, dist, idx, w, mode):
    """``predict`` of every column: scikit-learn's, on these neighbours, in the dtypes it reduces in; ``(nq, t)``."""
    y = np.asarray(y)
    d = np.zeros(np.shape(idx)) if dist is None else dist
    return np.asarray(PR.sklearn_predict(y, d, idx, _sklearn_weights(w, mode))).reshape(len(idx), -1)


def mode_of(v, ww):
    """``weighted_mode`` row by row: per distinct label (ascending) the vote ``np.sum(where(v == c, w, 0), axis=1)``; a
    strictly larger vote takes over, so the smaller label keeps an equal vote; all votes zero: NaN."""
    best_vote = np.zeros(v.shape[0])
    best = np.full(v.shape[0], np.nan)
    for c in np.unique(v):
        vote = np.sum(np.ascontiguousarray(np.where(v == c, ww, 0.0)), axis=1)
        best = np.where(vote > best_vote, c, best)
        best_vote = np.maximum(vote, best_vote)
    return best


def top_vote_tied(v, ww):
    """Rows in which two labels share the largest vote (the restatement's own votes)."""
    labels = np.unique(v)
    votes = np.stack([np.sum(np.ascontiguousarray(np.where(v == c, ww, 0.0)), axis=1) for c in labels], axis=1)
    top = votes.max(axis=1)
    return (np.sum(votes == top[:, None], axis=1) > 1) & (top > 0)


def summarize(y, dist, idx, w, mode, statistics):
    """``(nq, t)`` float64: column ``j`` is ``statistics[j]`` of the neighbours' values ``y[idx, j]``.  ``y``: ``(n, t)``
    (float32 targets reduce their ``mean`` as scikit-learn does; every other statistic is float64 arithmetic)."""
    y = np.asarray(y)
    assert y.ndim == 2 and len(statistics) == y.shape[1]
    idx = np.asarray(idx, dtype=np.int64)
    y64 = y.astype(np.float64)
    ww = weights_of(dist, idx, w, mode)
    out = np.empty((idx.shape[0], y.shape[1]), dtype=np.float64)
    mean = mean64 = None
    for j, name in enumerate(statistics):
        v = np.ascontiguousarray(y64[idx, j])
        if name == "mean":
            if mean is None:
                mean = mean_of(y, dist, idx, w, mode)
            out[:, j] = mean[:, j]
        elif name == "mode":
            out[:, j] = mode_of(v, ww)
        elif name == "min":
            out[:, j] = v.min(axis=1)
        elif name == "max":
            out[:, j] = v.max(axis=1)
        elif name == "nearest":
            out[:, j] = v[:, 0]
        elif name == "std":
            if mean64 is None:  # (the float64 weighted mean, whatever the targets' dtype and the weights' are)
                w64 = None if w is None else np.asarray(w, dtype=np.float64)
                mean64 = mean_of(y64, dist, idx, w64, mode)
            dv = v - mean64[:, j][:, None]
            ss = np.sum(np.ascontiguousarray((ww * dv) * dv), axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[:, j] = np.sqrt(ss / np.sum(ww, axis=1))
        else:
            raise ValueError(name)
    return out
