"""Neighbour usage: which reference rows made a map, how often at which rank, and how far they were imputed.

The contract of the numbers is stated once, in ``include/sknnr_hip.h`` ("Neighbour usage"); the device tallies them
(``sknnr_amd/csrc/tally.hip.h``) and :class:`NeighborUsage` is the small host-side object they are collected in."""

from __future__ import annotations

import numpy as np


class NeighborUsage:
    """Use counts of the reference rows over any number of tallied searches.

    Pass one as ``usage=`` to ``kneighbors_chunks`` / ``predict_chunks`` (the call adds what it tallied on the device and
    returns exactly what it returns without it), or get one from ``neighbor_usage()`` / ``independent_neighbor_usage()``.
    The first use binds ``(n_ref, k)``; a later use with another shape raises ``ValueError`` before any device work.

    ``counts``        ``(n_ref, k)`` int64: pixels each reference row served as first, second ... k-th neighbour
    ``max_distance``  ``(n_ref,)`` float64: the largest distance a row was imputed over, NaN where ``total == 0``
    ``total``         ``counts.sum(1)``;  ``unused``: ``total == 0``;  ``n_rows``: tallied query rows (``counts[:, 0].sum()``)
    ``ids``           the estimator's ``dataframe_index_in_`` when it was fitted with a dataframe, else None

    The tally is over row positions, never dataframe ids, and masked (nodata) pixels contribute nothing.  Instances
    compare by value, pickle, and merge with ``+=``."""

    __hash__ = None

    def __init__(self):
        self._counts = None  # (n_ref, k) int64
        self._max = None     # (n_ref,) float64, 0.0 where a row was never used (the C ABI's form)
        self.ids = None

    # -- binding -----------------------------------------------------------------------------
    @property
    def shape(self):
        """``(n_ref, k)`` once bound, else None."""
        return None if self._counts is None else self._counts.shape

    def _check(self, n_ref, k):
        if self._counts is not None and self._counts.shape != (int(n_ref), int(k)):
            raise ValueError(f"this NeighborUsage is bound to (n_ref, k) = {self._counts.shape}: it cannot take a tally of "
                             f"({int(n_ref)}, {int(k)})")

    def _bind(self, n_ref, k, ids=None):
        self._check(n_ref, k)
        if self._counts is None:
            self._counts = np.zeros((int(n_ref), int(k)), dtype=np.int64)
            self._max = np.zeros(int(n_ref), dtype=np.float64)
            self.ids = None if ids is None else np.asarray(ids)

    def _add(self, counts, max_dist, ids=None):
        """Add one tally (the C ABI's arrays: ``max_dist`` holds 0.0 for an unused row)."""
        counts = np.asarray(counts)
        self._bind(counts.shape[0], counts.shape[1], ids)
        self._counts += counts.astype(np.int64, copy=False)
        m = np.asarray(max_dist, dtype=np.float64)
        np.maximum(self._max, np.where(m > 0, m, 0.0), out=self._max)
        return self

    def _require(self):
        if self._counts is None:
            raise ValueError("this NeighborUsage has tallied nothing yet: it has no shape")

    # -- the numbers ---------------------------------------------------------------------------
    @property
    def counts(self):
        self._require()
        return self._counts

    @property
    def total(self):
        return self.counts.sum(axis=1)

    @property
    def unused(self):
        return self.total == 0

    @property
    def n_rows(self) -> int:
        return int(self.counts[:, 0].sum())

    @property
    def max_distance(self):
        self._require()
        return np.where(self.total == 0, np.nan, self._max)

    # -- value semantics ---------------------------------------------------------------------------
    def __iadd__(self, other):
        if not isinstance(other, NeighborUsage):
            return NotImplemented
        if other._counts is None:
            return self
        self._check(*other._counts.shape)
        return self._add(other._counts, other._max, other.ids)

    def __eq__(self, other):
        if not isinstance(other, NeighborUsage):
            return NotImplemented
        if self._counts is None or other._counts is None:
            return self._counts is None and other._counts is None
        same_ids = (self.ids is None) == (other.ids is None) and (self.ids is None or np.array_equal(self.ids, other.ids))
        return bool(self._counts.shape == other._counts.shape and np.array_equal(self._counts, other._counts)
                    and np.array_equal(self._max, other._max) and same_ids)

    def __repr__(self):
        if self._counts is None:
            return "NeighborUsage(unbound)"
        n_ref, k = self._counts.shape
        return f"NeighborUsage(n_ref={n_ref}, k={k}, n_rows={self.n_rows}, unused={int(self.unused.sum())})"
