"""The buffered leave-out contract (include/sknnr_hip.h, sknnr_index_set_buffer) in numpy, on top of tests/_groups.py.

``coords`` is ``(n_ref, c)`` float64, ``c`` 1 to 3; ``r2 = radius * radius``; for fitted rows i and r

    g(i, r) = ((x_i - x_r)*(x_i - x_r) + (y_i - y_r)*(y_i - y_r)) + (z_i - z_r)*(z_i - z_r)

every operation a separately rounded float64 operation (numpy's elementwise arithmetic is exactly that), a missing
column +0.0.  Row r is excluded for row i when ``g(i, r) <= r2`` or, with codes, when ``codes[r] == codes[i]``.  The
rest is the grouped model: ``_groups.value_rows`` -> mask -> the k smallest by (value, index) -> ``_groups.finish``.
"""

from __future__ import annotations

import numpy as np

import _groups


def positions3(coords):
    """``(n, 3)`` float64: ``coords`` with its missing columns as +0.0."""
    c = np.asarray(coords, dtype=np.float64)
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    assert c.ndim == 2 and 1 <= c.shape[1] <= 3
    out = np.zeros((c.shape[0], 3), dtype=np.float64)
    out[:, : c.shape[1]] = c
    return out


def excluded_mask(coords, radius, rows, codes=None):
    """``(len(rows), n_ref)`` bool: entry (i, r) says that row r is excluded for row ``rows[i]``."""
    p = positions3(coords)
    rows = np.asarray(rows, dtype=np.int64)
    r2 = np.float64(radius) * np.float64(radius)
    dx = p[rows, 0][:, None] - p[None, :, 0]
    dy = p[rows, 1][:, None] - p[None, :, 1]
    dz = p[rows, 2][:, None] - p[None, :, 2]
    g = (dx * dx + dy * dy) + dz * dz
    mask = g <= r2
    if codes is not None:
        codes = np.asarray(codes)
        mask |= codes[None, :] == codes[rows][:, None]
    return mask


def excluded_counts(coords, radius, codes=None, block=2048):
    """``excluded[]``: the row sums of the mask over all rows, int64."""
    n = positions3(coords).shape[0]
    out = np.empty(n, dtype=np.int64)
    for r0 in range(0, n, block):
        rows = np.arange(r0, min(n, r0 + block))
        out[rows] = excluded_mask(coords, radius, rows, codes).sum(axis=1)
    return out


def ranked_candidates(full, mask, kmax):
    """Excluded entries masked, then per row the ``kmax`` candidates smallest by (value, index), as
    ``_groups.ranked_candidates`` ranks them."""
    val = np.where(mask, np.inf, full)
    ids = np.broadcast_to(np.arange(full.shape[1]), full.shape)
    order = np.lexsort((ids, val), axis=1)[:, :kmax]
    return np.take_along_axis(val, order, axis=1), order.astype(np.int64)


def buffered_from_values(full, rows, coords, radius, k, *, codes=None, hamming=False, deterministic=True, decimals=10):
    val, idx = ranked_candidates(full, excluded_mask(coords, radius, rows, codes), k)
    return _groups.finish(val, idx, rows, hamming=hamming, deterministic=deterministic, decimals=decimals)


def buffered_kneighbors(fit, coords, radius, k, *, codes=None, formula="expanded", w=None, rows=None, deterministic=True,
                        decimals=10):
    """The model: ``(dist, idx)`` of fitted rows ``rows`` (default: all) under the buffer and, when given, the codes."""
    fit = np.asarray(fit)
    rows = np.arange(fit.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    full = _groups.value_rows(fit, rows, formula, w)
    return buffered_from_values(full, rows, coords, radius, k, codes=codes, hamming=formula == "hamming",
                                deterministic=deterministic, decimals=decimals)


# ---- position laws of the tests ----
def uniform_square(n, c=2, seed=0):
    """Uniform positions in the unit square (line, cube); :func:`radius_for` gives the radius that goes with them."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, c))


def radius_for(n, c=2, mean_excluded=5.0):
    """The radius at which a ball holds ``mean_excluded`` of ``n`` uniform rows of the unit cube in ``c`` dimensions
    (edge effects ignored): about that many rows are excluded per row on average."""
    share = min(mean_excluded / n, 0.5)
    unit_ball = {1: 2.0, 2: np.pi, 3: 4.0 * np.pi / 3.0}[c]
    return float((share / unit_ball) ** (1.0 / c))


def lattice(n, width):
    """Rows on the integer lattice, ``width`` to a line: row r sits at (r % width, r // width)."""
    r = np.arange(n)
    return np.stack([r % width, r // width], axis=1).astype(np.float64)


def lattice_counts(n, width, offsets):
    """``excluded[]`` on :func:`lattice` when exactly the lattice ``offsets`` (dx, dy) are within the radius: counted
    in integers, no float arithmetic."""
    r = np.arange(n)
    x, y = r % width, r // width
    out = np.zeros(n, dtype=np.int64)
    for dx, dy in offsets:
        xx, yy = x + dx, y + dy
        out += (xx >= 0) & (xx < width) & (yy >= 0) & (yy * width + xx < n)
    return out


def colocated_pairs(n, seed=0):
    """Rows 2j and 2j + 1 share a position; the pairs are uniform in the unit square."""
    base = np.random.default_rng(seed).uniform(0.0, 1.0, ((n + 1) // 2, 2))
    return np.repeat(base, 2, axis=0)[:n].copy()


def cluster(n, members, radius, seed=0, first=None):
    """``members`` rows inside one disc of diameter ``0.9 * radius`` around (10, 10) -- every pair of them is within
    ``radius`` -- and the other rows uniform in the unit square, farther than ``radius`` from the disc when ``radius < 6``.
    The members are a seeded choice, or rows ``first .. first + members - 1``.  Returns ``(coords, member rows)``."""
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0.0, 1.0, (n, 2))
    who = np.sort(rng.choice(n, members, replace=False)) if first is None else np.arange(first, first + members)
    ang = rng.uniform(0.0, 2.0 * np.pi, members)
    rad = 0.45 * radius * np.sqrt(rng.uniform(0.0, 1.0, members))
    coords[who] = 10.0 + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    return coords, who
