"""numpy restatement of the zonal-statistics contract (include/sknnr_hip.h, "Zonal statistics"; the device form is
sknnr_amd/csrc/zonal.hip.h).  Shared by test_zonal_cpu.py, test_zonal_kernels_gpu.py and test_zonal_gpu.py.  The
conversion is tests/_narrow.py's."""

from __future__ import annotations

import numpy as np

from _narrow import narrow_values

COUNT, SUM, SQ_LO, SQ_HI, MIN, MAX = range(6)
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
DTYPES = tuple(np.dtype(t) for t in (np.int16, np.uint16, np.uint8, np.int32))


def empty(n_zones, c, n_classes=None):
    """``(acc, hist)`` nothing was added to: zeros, the min / max sentinels, and the flat class blocks (None without)."""
    acc = np.zeros((n_zones, c, 6), dtype=np.int64)
    acc[..., MIN] = I64_MAX
    acc[..., MAX] = I64_MIN
    per_zone = 0 if n_classes is None else int(np.sum(n_classes))
    return acc, (np.zeros(n_zones * per_zone, dtype=np.int64) if per_zone else None)


def hist_blocks(hist, n_zones, n_classes):
    """The flat ``hist`` as ``{column: (n_zones, n_classes[column]) view}``."""
    out, at = {}, 0
    for j, nc in enumerate(n_classes):
        if nc > 0:
            out[j] = hist[at:at + n_zones * nc].reshape(n_zones, nc)
            at += n_zones * nc
    return out


def zonal(values, zones, dtype, scale, offset, n_zones, n_classes, acc=None, hist=None):
    """Add the tile to ``acc`` / ``hist`` (None: fresh ones) and return ``(acc, hist, n_nan, n_outside, n_other)``:
    NaN entries of pixels inside the zones, pixels outside the zones, class values outside their range."""
    values = np.asarray(values, dtype=np.float64)
    n, c = values.shape
    zones = np.asarray(zones).astype(np.int64).reshape(-1)
    assert zones.size == n
    if acc is None:
        acc, hist = empty(n_zones, c, n_classes)
    inside = (zones >= 0) & (zones < n_zones)
    n_outside = int((~inside).sum())
    v, z = values[inside], zones[inside]
    nan = np.isnan(v)  # (tested first, on the value itself)
    q = narrow_values(v, dtype, scale, offset, fill=None).astype(np.int64)
    sq = (q * q).astype(np.uint64)  # (|q| <= 2^31: exact in 64 bits)
    lo, hi = (sq & np.uint64(0xFFFFFFFF)).astype(np.int64), (sq >> np.uint64(32)).astype(np.int64)
    blocks = {} if n_classes is None or hist is None else hist_blocks(hist, n_zones, n_classes)
    n_other = 0
    for j in range(c):
        ok = ~nan[:, j]
        zj, qj = z[ok], q[ok, j]
        np.add.at(acc[:, j, COUNT], zj, 1)
        np.add.at(acc[:, j, SUM], zj, qj)
        np.add.at(acc[:, j, SQ_LO], zj, lo[ok, j])
        np.add.at(acc[:, j, SQ_HI], zj, hi[ok, j])
        np.minimum.at(acc[:, j, MIN], zj, qj)
        np.maximum.at(acc[:, j, MAX], zj, qj)
        if j in blocks:
            nc = blocks[j].shape[1]
            known = (qj >= 0) & (qj < nc)
            n_other += int((~known).sum())
            np.add.at(blocks[j], (zj[known], qj[known]), 1)
    return acc, hist, int(nan.sum()), n_outside, n_other


# The hand-written case: 12 pixels x 2 planes x 3 zones, int16, plane 0 scaled by 10, plane 1 a class plane of 3 classes.
HAND_VALUES = np.array([
    [1.0, 0.0], [2.0, 1.0], [3.04, 2.0],       # zone 0: stored 10, 20, 30
    [-1.5, 1.0], [np.nan, 1.0], [0.25, 5.0],   # zone 1: stored -15, (NaN), 2 (2.5 rounds to even); classes 1, 1, 5 (other)
    [4000.0, 0.0], [1.0, np.nan],              # zone 2: 40000 clamps to 32767; a NaN class entry
    [7.0, 2.0], [8.0, 2.0],                    # zone codes -1 and 3: outside
    [np.nan, np.nan], [0.0, -1.0],             # zone 2: a nodata pixel; stored 0 and class -1 (other)
])
HAND_ZONES = np.array([0, 0, 0, 1, 1, 1, 2, 2, -1, 3, 2, 2], dtype=np.int32)
HAND_SCALE, HAND_OFFSET = np.array([10.0, 1.0]), np.array([0.0, 0.0])
HAND_CLASSES = np.array([0, 3], dtype=np.int32)
# acc[z, j] = count, sum, sq_lo, sq_hi, min, max
HAND_ACC = np.array([
    [[3, 60, 1400, 0, 10, 30], [3, 3, 5, 0, 0, 2]],
    [[2, -13, 229, 0, -15, 2], [3, 7, 27, 0, 1, 5]],
    [[3, 32777, 32767 * 32767 + 100, 0, 0, 32767], [2, -1, 1, 0, -1, 0]],
], dtype=np.int64)
HAND_HIST = np.array([[1, 1, 1], [0, 2, 0], [1, 0, 0]], dtype=np.int64)
HAND_COUNTERS = (4, 2, 2)  # NaN entries inside the zones, pixels outside, class values outside their range
