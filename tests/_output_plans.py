"""The numpy restatement of output plans (include/sknnr_hip.h, "output plans"): ``n_out`` planes per query, each one
statistic of one target column over the query's k neighbours.  The six statistics of ``enum sknnr_statistic`` are those of
tests/_neighbor_stats.py (imported, never edited); the weighted quantile is restated here word for word from the header:

1. order the k pairs ``(v_i, w_i)`` by ``(v_i, i)`` ascending -- a stable sort by value, ``-0.0 == 0.0``;
2. ``c_0 = w_(0)``, ``c_a = c_(a-1) + w_(a)``: a plain sequential float64 running sum in sorted order; ``total = c_(k-1)``;
3. ``cdf_a = c_a / total``, one division each;
4. the result is ``v_(a*)``, ``a*`` the first ``a`` with ``cdf_a != 0.0`` and ``cdf_a >= q``, or ``k - 1`` when there is none;
5. ``total`` not ``> 0``: NaN.

That is ``np.quantile(v, q, method="inverted_cdf", weights=w)`` of numpy >= 2.0 (test_output_plans_cpu.py compares the two).
Shared by test_output_plans_cpu.py, test_output_plans_kernels_gpu.py and test_output_plans_gpu.py."""

from __future__ import annotations

import numpy as np

import _neighbor_stats as NS

QUANTILE = 6  # SKNNR_STAT_QUANTILE
CODES = {**NS.CODES, "quantile": QUANTILE}


def weighted_quantile(v, w, q):
    """Rows of ``(nq, k)`` values and weights -> ``(nq,)``: the restatement above, vectorised over the rows (the running sum
    stays a sequential loop over the k sorted positions, so no pairwise order can slip in)."""
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    nq, k = v.shape
    order = np.argsort(v, axis=1, kind="stable")  # (stable: equal values -- -0.0 and 0.0 included -- keep neighbour order)
    vs = np.take_along_axis(v, order, axis=1)
    ws = np.take_along_axis(w, order, axis=1)
    c = np.empty_like(ws)
    c[:, 0] = ws[:, 0]
    for a in range(1, k):
        c[:, a] = c[:, a - 1] + ws[:, a]
    total = c[:, k - 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        cdf = c / total[:, None]
        ok = (cdf != 0.0) & (cdf >= q)
    first = np.where(ok.any(axis=1), ok.argmax(axis=1), k - 1)
    out = vs[np.arange(nq), first]
    return np.where(total > 0.0, out, np.nan)


def split(stat):
    """A plan entry's statistic -- a name, ``"median"`` or ``("quantile", q)`` -- as (name, parameter)."""
    if stat == "median":
        return "quantile", 0.5
    if isinstance(stat, tuple):
        assert stat[0] == "quantile"
        return "quantile", float(stat[1])
    return stat, 0.0


def arrays(plan):
    """``[(target, statistic), ...]`` as the ``(cols, codes, params)`` the C entry points take."""
    names = [split(s) for _, s in plan]
    return (np.array([j for j, _ in plan], dtype=np.int32), np.array([CODES[n] for n, _ in names], dtype=np.int32),
            np.array([p for _, p in names], dtype=np.float64))


def plan_of(y, dist, idx, w, mode, plan):
    """``(nq, n_out)`` float64: plane ``e`` is statistic ``plan[e][1]`` of target ``plan[e][0]``.  ``y``: ``(n, t)``; the six
    old statistics come from ``_neighbor_stats.summarize`` with that name in every column (one call per distinct name)."""
    y = np.asarray(y)
    assert y.ndim == 2
    idx = np.asarray(idx, dtype=np.int64)
    t = y.shape[1]
    y64 = y.astype(np.float64)
    ww = NS.weights_of(dist, idx, w, mode)
    out = np.empty((idx.shape[0], len(plan)), dtype=np.float64)
    old = {}
    for e, (j, stat) in enumerate(plan):
        name, q = split(stat)
        if name == "quantile":
            out[:, e] = weighted_quantile(y64[idx, j], ww, q)
            continue
        if name not in old:
            with np.errstate(all="ignore"):
                old[name] = NS.summarize(y, dist, idx, w, mode, (name,) * t)
        out[:, e] = old[name][:, j]
    return out
