"""The numpy restatement of neighbour replay (include/sknnr_hip.h, "Neighbour replay"): the decode of a tile of stored
neighbours into the pipeline's full-layout tile, and what the later stages make of it.  Predictions and statistics come
from the existing restatements (tests/_predict_ref.py, tests/_neighbor_stats.py, tests/_output_plans.py), applied to the
decoded neighbours of the pixels that are neither masked nor unknown.  Shared by test_replay_cpu.py,
test_replay_kernels_gpu.py and test_replay_gpu.py."""

from __future__ import annotations

import numpy as np

import _neighbor_stats as NS
import _output_plans as OP


def sorted_table(ids):
    """The id table as the handle holds it: the int64 ids sorted, and the row position of every sorted entry."""
    ids = np.asarray(ids, dtype=np.int64)
    perm = np.argsort(ids, kind="stable")
    return ids[perm], perm.astype(np.int64)


def rows_form(a, bands):
    """A stored array as rows ``(n, ks)``: itself, or band-first ``(ks, ...)`` planes transposed."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(a.shape[0], -1).T) if bands else a


def decode(idx, dist, k, n_ref, fill_index=-1, ids=None, bands=False):
    """``(idx64 (n, k), dist64 (n, k) or None, masked (n,), unknown (n,))`` of one tile: the leading ``k`` stored columns,
    widened exactly; a pixel whose FIRST stored value equals ``fill_index`` is masked (tested on the stored value, before
    any lookup); with ``ids`` every used value is looked up by ``np.searchsorted`` in the sorted table; a value that is not
    in it, or a row position outside ``[0, n_ref)``, in a used column of a pixel that is not masked makes the pixel
    unknown.  Masked and unknown pixels get index -1 and NaN distances."""
    idx = rows_form(idx, bands)
    n, ks = idx.shape
    assert 1 <= k <= ks
    masked = idx[:, 0].astype(np.int64) == fill_index
    used = idx[:, :k].astype(np.int64)
    if ids is not None:
        table, perm = sorted_table(ids)
        pos = np.searchsorted(table, used, side="left")
        found = (pos < table.size) & (table[np.minimum(pos, table.size - 1)] == used)
        rows = np.where(found, perm[np.minimum(pos, table.size - 1)], -1)
    else:
        rows = used
    bad_value = (rows < 0) | (rows >= n_ref)
    unknown = ~masked & bad_value.any(axis=1)
    blank = masked | unknown
    out_idx = np.where(blank[:, None], np.int64(-1), rows).astype(np.int64)
    out_dist = None
    if dist is not None:
        out_dist = rows_form(dist, bands)[:, :k].astype(np.float64)
        out_dist[blank] = np.nan
    return out_idx, out_dist, masked, unknown


def decode_loop(idx, dist, k, n_ref, fill_index=-1, ids=None):
    """:func:`decode` of a row tile as a plain Python loop over pixels and columns (a dict for the id lookup)."""
    lookup = None if ids is None else {int(v): r for r, v in enumerate(ids)}
    n = len(idx)
    out_idx = np.full((n, k), -1, dtype=np.int64)
    out_dist = None if dist is None else np.full((n, k), np.nan)
    masked, unknown = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for i in range(n):
        if int(idx[i][0]) == fill_index:
            masked[i] = True
            continue
        rows = []
        for j in range(k):
            v = int(idx[i][j])
            r = v if lookup is None else lookup.get(v, -1)
            rows.append(r)
        if any(r < 0 or r >= n_ref for r in rows):
            unknown[i] = True
            continue
        out_idx[i] = rows
        if dist is not None:
            out_dist[i] = [float(dist[i][j]) for j in range(k)]
    return out_idx, out_dist, masked, unknown


def reduce(y, idx64, dist64, weights="uniform", statistic=None, outputs=None, weight_fn=None):
    """The prediction tile of decoded neighbours: ``(n, t)`` (``statistic``: one name per target; None: the mean), or
    ``(n, n_out)`` for ``outputs``; NaN rows where the pixel is masked or unknown (index -1).  ``weight_fn``: a
    distance-weight law as a numpy callable (the weights are then explicit)."""
    y = np.asarray(y)
    y2 = y.reshape(len(y), -1)
    good = idx64[:, 0] >= 0
    t_out = len(outputs) if outputs is not None else y2.shape[1]
    out = np.full((len(idx64), t_out), np.nan)
    if not good.any():
        return out
    gi = np.ascontiguousarray(idx64[good])
    gd = None if dist64 is None else np.ascontiguousarray(dist64[good])
    w, mode = None, weights
    if weight_fn is not None:
        w, mode = np.ascontiguousarray(weight_fn(gd), dtype=np.float64), "explicit"
    if outputs is not None:
        out[good] = OP.plan_of(y2, gd, gi, w, mode, list(outputs))
    else:
        out[good] = NS.summarize(y2, gd, gi, w, mode, list(statistic) if statistic is not None else ["mean"] * y2.shape[1])
    return out
