"""The numpy restatement of the bootstrap contract (include/sknnr_hip.h, "Bootstrap"): the table draw, the copies, the
replicate values, the 64-partial fold and the outputs, line for line.  Vectorised over pixels and replicates; every sum the
contract calls sequential stays a Python loop over the list's columns (or over the passes of 64 replicates), so no pairwise
order can slip in, and every product is a rounded numpy product that is then added.

Shared by test_bootstrap_cpu.py, test_bootstrap_kernels_gpu.py and test_bootstrap_gpu.py."""

from __future__ import annotations

import numpy as np

CODES = {"boot_se": 0, "boot_mean": 1, "boot_bias": 2, "boot_count": 3}  # enum sknnr_bootstrap_statistic


def draw_table(n_replicates, n, seed=0, groups=None):
    """The table ``Bootstrap`` draws: per replicate in order one ``rng.integers(0, G, size=G)`` draw, counted; without
    groups every row is its own group, with them each row gets its group's count.  int64 ``(B, n)``."""
    rng = np.random.default_rng(seed)
    if groups is None:
        return np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(n_replicates)]).astype(np.int64)
    _, codes = np.unique(np.asarray(groups), return_inverse=True)
    g = int(codes.max()) + 1
    return np.stack([np.bincount(rng.integers(0, g, size=g), minlength=g)[codes] for _ in range(n_replicates)]).astype(np.int64)


def arrays(plan):
    """``[(target, name), ...]`` (``"boot_count"`` may stand alone) as the ``(cols, codes)`` the C entry takes."""
    plan = [(0, e) if isinstance(e, str) else e for e in plan]
    return np.array([j for j, _ in plan], dtype=np.int32), np.array([CODES[s] for _, s in plan], dtype=np.int32)


def base_weights(dist, shape, weights):
    """``(w, z, is_distance)``: the per-column weights ``predict`` would use before any mask, and the ``d == 0`` mask.
    ``weights``: ``"uniform"``, ``"distance"`` or a law of ``sknnr_amd.weights`` (called on the distances)."""
    if isinstance(weights, str) and weights == "uniform":
        return np.ones(shape), np.zeros(shape), False
    d = np.asarray(dist, dtype=np.float64)
    if isinstance(weights, str):
        assert weights == "distance"
        with np.errstate(divide="ignore"):
            return 1.0 / d, (d == 0.0).astype(np.float64), True
    return np.asarray(weights(d), dtype=np.float64), np.zeros(shape), False


def copies(M, idx, k):
    """``c`` int16 ``(nq, B, kw)`` and ``short`` bool ``(nq, B)``: left = k; for j ascending c_j = min(M[b, r_j], left)."""
    Mi = np.minimum(np.asarray(M), 255)[:, idx].transpose(1, 0, 2).astype(np.int16)
    nq, B, kw = Mi.shape
    left = np.full((nq, B), int(k), dtype=np.int16)
    c = np.zeros_like(Mi)
    for j in range(kw):
        c[:, :, j] = np.minimum(Mi[:, :, j], left)
        left -= c[:, :, j]
    return c, left > 0


def weighted(c, w, z, yv, distance):
    """``den`` ``(nq, B)`` and ``num`` ``(nq, B, nc)`` of copies ``c``: sequential over the taken columns from +0.0, with the
    0 / 1 mask of ``d == 0`` over the taken columns in place of the weights when one of them has ``d == 0``."""
    nq, B, kw = c.shape
    nc = yv.shape[2]
    den, num = np.zeros((nq, B)), np.zeros((nq, B, nc))
    denz, numz = np.zeros((nq, B)), np.zeros((nq, B, nc))
    anyz = np.zeros((nq, B), dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(kw):
            taken = c[:, :, j] > 0
            if not taken.any():
                continue
            cd = c[:, :, j].astype(np.float64)
            cw = cd * w[:, None, j]
            den = np.where(taken, den + cw, den)
            num = np.where(taken[:, :, None], num + cw[:, :, None] * yv[:, None, j, :], num)
            if distance:
                cz = cd * z[:, None, j]
                anyz |= taken & (z[:, None, j] != 0.0)
                denz = np.where(taken, denz + cz, denz)
                numz = np.where(taken[:, :, None], numz + cz[:, :, None] * yv[:, None, j, :], numz)
    if distance:
        den = np.where(anyz, denz, den)
        num = np.where(anyz[:, :, None], numz, num)
    return den, num


def fold64(a):
    """``(nq, B, nc)`` -> ``(nq, nc)``: partial l adds a_b over b = l, l + 64 ... ascending from +0.0; the partials are folded
    by P[l] = P[l] + P[l + s] for l < s, s = 32 .. 1."""
    nq, B, nc = a.shape
    P = np.zeros((nq, 64, nc))
    for b0 in range(0, B, 64):
        part = a[:, b0:b0 + 64]
        P[:, : part.shape[1]] = P[:, : part.shape[1]] + part
    s = 32
    while s >= 1:
        P[:, :s] = P[:, :s] + P[:, s:2 * s]
        s //= 2
    return P[:, 0]


def replicates(y, dist, idx, M, k, weights, cols):
    """Everything per (pixel, replicate) for target columns ``cols``: a dict of ``p`` ``(nq, B, nc)`` replicate values,
    ``valid`` and ``short`` ``(nq, B)``, ``c`` the copies, ``mult`` the multiplicities met ``(nq, B, kw)``, ``p0``
    ``(nq, nc)``, ``p0_ok`` and ``bad`` ``(nq,)``."""
    y = np.asarray(y, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    nq, kw = idx.shape
    bad = ((idx < 0) | (idx >= y.shape[0])).any(axis=1)
    safe = np.where((idx < 0) | (idx >= y.shape[0]), 0, idx)
    w, z, distance = base_weights(dist, idx.shape, weights)
    yv = y[safe][:, :, list(cols)]
    c, short = copies(M, safe, k)
    den, num = weighted(c, w, z, yv, distance)
    c0 = np.zeros((nq, 1, kw), dtype=np.int16)
    c0[:, :, :k] = 1
    den0, num0 = weighted(c0, w, z, yv, distance)
    p0_ok = (den0[:, 0] > 0.0) & ~bad
    with np.errstate(all="ignore"):
        p0 = num0[:, 0] / den0[:, 0, None]
        p = num / den[:, :, None]
    valid = ~short & (den > 0.0) & p0_ok[:, None]
    mult = np.minimum(np.asarray(M), 255)[:, safe].transpose(1, 0, 2)
    return dict(p=p, valid=valid, short=short, c=c, mult=mult, p0=p0, p0_ok=p0_ok, bad=bad)


def bootstrap_of(y, dist, idx, M, k, weights, plan, want_info=False):
    """``(out, tally)``: ``out`` ``(nq, n_out)`` float64 for ``plan`` = ``[(target, "boot_se" | "boot_mean" | "boot_bias"),
    "boot_count", ...]`` and ``tally`` the int64 pair (pixels reduced, valid replicates over them)."""
    plan = [(0, e) if isinstance(e, str) else e for e in plan]
    cols = sorted({j for j, s in plan if s != "boot_count"}) or [0]
    r = replicates(y, dist, idx, M, k, weights, cols)
    valid, p0, p0_ok = r["valid"], r["p0"], r["p0_ok"]
    with np.errstate(all="ignore"):
        a = np.where(valid[:, :, None], r["p"] - p0[:, None, :], 0.0)
        S1, S2 = fold64(a), fold64(a * a)
        m = valid.sum(axis=1)
        md = m.astype(np.float64)[:, None]
        bias = S1 / md
        mean = p0 + S1 / md
        se = np.sqrt(np.maximum((S2 - S1 * (S1 / md)) / (md - 1.0), 0.0))
    none = ~p0_ok | (m == 0)
    bias[none] = np.nan
    mean[none] = np.nan
    se[none | (m < 2)] = np.nan
    out = np.empty((idx.shape[0], len(plan)))
    for e, (j, s) in enumerate(plan):
        if s == "boot_count":
            out[:, e] = m
        else:
            out[:, e] = {"boot_se": se, "boot_mean": mean, "boot_bias": bias}[s][:, cols.index(j)]
    tally = np.array([(~r["bad"]).sum(), m[~r["bad"]].sum()], dtype=np.int64)
    if want_info:
        r["m"] = m
        return out, tally, r
    return out, tally
