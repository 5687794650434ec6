"""Distance domain: where a nearest-neighbour map extrapolates.

The contract of the numbers is stated once, in ``include/sknnr_hip.h`` ("Distance domain"); the device computes them
(``sknnr_amd/csrc/domain.hip.h``) and :class:`DistanceDomain` is the small host-side object they are collected in."""

from __future__ import annotations

import numpy as np

NODATA_CODE = 255  # the code of a pixel whose score is NaN
_N_ACC = 103       # codes 0 .. 100, beyond pixels, nodata pixels


class DistanceDomain:
    """A sorted table of reference-to-reference distances, and the tallies of the pixels placed within it.

    ``table``      distances between the reference plots in the estimator's own metric (``est.distance_domain()`` makes
                   one from honest leave-out neighbours): finite, ``>= 0``, any order -- stored sorted, float64, read-only
    ``threshold``  optional, finite and ``>= 0``: a pixel whose score is above it is *beyond* (yaImpute's "notably distant")
    ``rank``       which neighbour's distance is the pixel's score (1: the nearest)

    Pass one as ``domain=`` to ``kneighbors_chunks`` / ``predict_chunks`` (the call adds what it tallied on the device and
    returns exactly what it returns without it) or to ``domain_scores``.  A pixel's code is the percentage of table
    entries strictly below its score, ``(100 * searchsorted(table, s, "left")) // m``: 0 .. 100, and 100 exactly when the
    score is above every entry; 255 marks a nodata pixel.

    ``hist``          ``(101,)`` int64: pixels per code, nodata pixels excluded
    ``n_pixels``      ``hist.sum()``;  ``n_beyond``: pixels above the threshold (0 without one);  ``n_nodata``
    ``share_beyond``  ``n_beyond / n_pixels``, NaN with no pixels

    Instances compare by value, pickle, and merge with ``+=`` (equal table, threshold and rank only)."""

    __hash__ = None

    def __init__(self, table, threshold=None, rank=1):
        table = np.array(table, dtype=np.float64).reshape(-1)  # (a copy: the caller's array stays as it is)
        if table.size < 1:
            raise ValueError("the table of a DistanceDomain needs at least one distance")
        if table.size > 2**31 - 1:
            raise ValueError("the table of a DistanceDomain holds at most 2^31 - 1 distances")
        if not np.isfinite(table).all() or (table < 0).any():
            raise ValueError("the table of a DistanceDomain holds finite distances >= 0")
        table = np.sort(table) + 0.0  # (-0.0 is 0)
        table.setflags(write=False)
        if isinstance(rank, bool) or int(rank) != rank or int(rank) < 1:
            raise ValueError(f"rank must be an integer >= 1, got {rank!r}")
        if threshold is not None:
            threshold = float(threshold)
            if not np.isfinite(threshold) or threshold < 0:
                raise ValueError(f"threshold must be finite and >= 0, got {threshold!r}")
            threshold += 0.0
        self.table = table
        self.threshold = threshold
        self.rank = int(rank)
        self._acc = np.zeros(_N_ACC, dtype=np.int64)

    # -- the contract on the host ------------------------------------------------------------------
    def percent(self, s):
        """The codes of the scores ``s`` (any shape) as uint8: the numpy statement of the contract."""
        s = np.asarray(s, dtype=np.float64)
        nan = np.isnan(s)
        below = np.searchsorted(self.table, np.where(nan, 0.0, s), side="left").astype(np.int64)
        code = (100 * below) // self.table.size
        return np.where(nan, NODATA_CODE, code).astype(np.uint8)

    def _add(self, acc):
        """Add one tally (the C ABI's 103 accumulators)."""
        acc = np.asarray(acc, dtype=np.int64).reshape(-1)
        if acc.size != _N_ACC:
            raise ValueError(f"a domain tally has {_N_ACC} accumulators, got {acc.size}")
        self._acc += acc
        return self

    # -- the numbers ---------------------------------------------------------------------------------
    @property
    def hist(self):
        return self._acc[:101].copy()

    @property
    def n_pixels(self) -> int:
        return int(self._acc[:101].sum())

    @property
    def n_beyond(self) -> int:
        return int(self._acc[101])

    @property
    def n_nodata(self) -> int:
        return int(self._acc[102])

    @property
    def share_beyond(self) -> float:
        n = self.n_pixels
        return float("nan") if n == 0 else self.n_beyond / n

    # -- value semantics -----------------------------------------------------------------------------
    def _same_definition(self, other) -> bool:
        return bool(self.rank == other.rank and self.threshold == other.threshold
                    and np.array_equal(self.table, other.table))

    def __iadd__(self, other):
        if not isinstance(other, DistanceDomain):
            return NotImplemented
        if not self._same_definition(other):
            raise ValueError("only DistanceDomain objects of equal table, threshold and rank can be added")
        return self._add(other._acc)

    def __eq__(self, other):
        if not isinstance(other, DistanceDomain):
            return NotImplemented
        return self._same_definition(other) and bool(np.array_equal(self._acc, other._acc))

    def __getstate__(self):
        return dict(table=np.array(self.table), threshold=self.threshold, rank=self.rank, acc=self._acc)

    def __setstate__(self, state):
        table = np.array(state["table"], dtype=np.float64)
        table.setflags(write=False)
        self.table, self.threshold, self.rank = table, state["threshold"], int(state["rank"])
        self._acc = np.array(state["acc"], dtype=np.int64)

    def __repr__(self):
        thr = "None" if self.threshold is None else f"{self.threshold:.6g}"
        return (f"DistanceDomain(m={self.table.size}, rank={self.rank}, threshold={thr}, n_pixels={self.n_pixels}, "
                f"n_beyond={self.n_beyond}, n_nodata={self.n_nodata})")
