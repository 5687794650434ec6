"""The distance-domain contract (include/sknnr_hip.h, "Distance domain") restated in numpy: the codes of a distance
tile, the 103 accumulators, and the prediction tile after the mask.  The device's results must equal these exactly --
every quantity is a comparison or an integer -- so the tests compare with ``assert_array_equal``."""

from __future__ import annotations

import numpy as np

N_ACC = 103
BEYOND, NODATA = 101, 102
NODATA_CODE = 255


def _score(dist, rank):
    dist = np.asarray(dist, dtype=np.float64)
    assert dist.ndim == 2 and 1 <= rank <= dist.shape[1]
    return dist[:, rank - 1]


def codes(dist, table, rank):
    """uint8 code per row of ``dist`` ``(n, k)``: 255 for a NaN score, else ``(100 * #{T < s}) // m``."""
    table = np.asarray(table, dtype=np.float64)
    assert table.ndim == 1 and table.size >= 1 and np.all(np.diff(table) >= 0)
    s = _score(dist, rank)
    nan = np.isnan(s)
    below = np.searchsorted(table, np.where(nan, 0.0, s), side="left").astype(np.int64)
    # (searchsorted's "left" is the strict count: the first position whose entry is not below s)
    code = (100 * below) // table.size
    return np.where(nan, NODATA_CODE, code).astype(np.uint8)


def beyond(dist, rank, threshold):
    """Boolean per row: the score is above the threshold (False for NaN, and always without a threshold)."""
    s = _score(dist, rank)
    if threshold is None:
        return np.zeros(len(s), dtype=bool)
    with np.errstate(invalid="ignore"):
        return s > threshold


def acc(dist, table, rank, threshold=None, into=None):
    """The int64[103] accumulators of the tile, added to ``into`` when given."""
    c = codes(dist, table, rank)
    out = np.zeros(N_ACC, dtype=np.int64) if into is None else np.array(into, dtype=np.int64)
    valid = c != NODATA_CODE
    out[:101] += np.bincount(c[valid], minlength=101)
    out[BEYOND] += int(beyond(dist, rank, threshold).sum())
    out[NODATA] += int((~valid).sum())
    return out


def masked_predictions(pred, dist, rank, threshold):
    """The float64 prediction tile ``(n, c)`` with the rows of beyond pixels NaN in every column."""
    out = np.array(pred, dtype=np.float64)
    out = out[:, None] if out.ndim == 1 else out
    out[beyond(dist, rank, threshold)] = np.nan
    return out
