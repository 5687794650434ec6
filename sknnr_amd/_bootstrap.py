"""Bootstrap standard errors per pixel: how uncertain a k-NN attribute map is because the plots are a sample.

The contract of the numbers is stated once, in ``include/sknnr_hip.h`` ("Bootstrap"); the device reduces all replicates of
a pixel from ONE neighbour list of ``n_candidates`` columns (``sknnr_amd/csrc/bootstrap.hip.h``) and :class:`Bootstrap` is
the small host-side object that holds the resampling table and collects the tallies."""

from __future__ import annotations

import numpy as np

MAX_REPLICATES = 4096  # kBootMaxB
MAX_CANDIDATES = 192   # kBootMaxKw: the search's own limit
BOOT_OUTPUTS = ("boot_se", "boot_mean", "boot_bias")  # take a target; "boot_count" takes none


class Bootstrap:
    """A bootstrap over the fitted rows (McRoberts et al. 2011), reduced per pixel on the device.

    Pass one as ``bootstrap=`` to ``summarize`` / ``predict_chunks``, or to ``bootstrap_neighbors_chunks`` /
    ``bootstrap_neighbors`` for a stored neighbour raster.
    Replicate ``b`` contains fitted row ``r`` ``multiplicity[b, r]`` times; its k nearest rows of a pixel are the first k
    copies met along the pixel's ordinary neighbour list, so one search at ``n_candidates`` columns serves every replicate.

    ``n_replicates``  B, 1 to 4096
    ``seed``          the table is drawn on the first use, when the number of fitted rows ``n`` is bound:
                      ``rng = np.random.default_rng(seed)``, then per replicate in order
                      ``np.bincount(rng.integers(0, n, size=n), minlength=n)``
    ``groups``        one label per fitted row: the draw is over the G groups and each row gets its group's count (a
                      cluster bootstrap)
    ``multiplicity``  a ready ``(B, n)`` table of non-negative integers instead of a draw, e.g. a delete-a-group
                      jackknife; counts above 255 are clamped (no result can tell: a replicate takes at most 192 copies)
    ``n_candidates``  columns of the one search, ``kw``.  Default ``min(n_samples_fit_, 192, 4 * k + 8)``: a STARTING value.
                      A replicate that meets fewer than k copies among a pixel's ``kw`` neighbours is *short* there and is
                      left out of that pixel's statistics; check ``share_short`` and widen ``n_candidates`` if it is not small.

    After use: ``multiplicity`` (the table, read-only: the device reduces from a copy of it), ``pixels`` (pixels reduced, masked ones not counted), ``replicates_used`` (valid
    (pixel, replicate) pairs) and ``share_short`` = ``1 - replicates_used / (pixels * B)``.

    The transform of a transformed estimator (CCA, CCorA, the forests) is the one fitted on all plots: it is not refitted per
    replicate.  Instances compare by value, pickle, and merge their tallies with ``+=``."""

    __hash__ = None

    def __init__(self, n_replicates=None, seed=0, groups=None, n_candidates=None, multiplicity=None):
        self._table = None
        if multiplicity is not None:
            m = np.asarray(multiplicity)
            if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
                raise ValueError(f"multiplicity must be a (B, n) table, got shape {m.shape}")
            if m.dtype.kind not in "iub":
                raise TypeError(f"multiplicity must hold integers, got dtype {m.dtype}")
            if m.dtype.kind == "i" and (m < 0).any():
                raise ValueError("multiplicity must not be negative")
            if groups is not None:
                raise ValueError("groups belong to a drawn table: a ready multiplicity takes none")
            if n_replicates is not None and int(n_replicates) != m.shape[0]:
                raise ValueError(f"n_replicates = {n_replicates}, but multiplicity has {m.shape[0]} rows")
            n_replicates = m.shape[0]
            self._table = np.ascontiguousarray(np.minimum(m, 255), dtype=np.uint8)
            self._table.setflags(write=False)  # (the device holds a copy of it: the table never changes once it exists)
        if n_replicates is None:
            raise TypeError("Bootstrap needs n_replicates (or a multiplicity table)")
        if isinstance(n_replicates, (bool, float)) or int(n_replicates) != n_replicates:
            raise TypeError(f"n_replicates must be an integer, got {n_replicates!r}")
        if not 1 <= int(n_replicates) <= MAX_REPLICATES:
            raise ValueError(f"n_replicates must lie in [1, {MAX_REPLICATES}], got {n_replicates}")
        if n_candidates is not None:
            if isinstance(n_candidates, (bool, float)) or int(n_candidates) != n_candidates:
                raise TypeError(f"n_candidates must be an integer, got {n_candidates!r}")
            if not 1 <= int(n_candidates) <= MAX_CANDIDATES:
                raise ValueError(f"n_candidates must lie in [1, {MAX_CANDIDATES}], got {n_candidates}")
        self.n_replicates = int(n_replicates)
        self.seed = seed
        self.groups = None if groups is None else (groups.to_numpy() if hasattr(groups, "to_numpy") else np.asarray(groups))
        self.n_candidates = None if n_candidates is None else int(n_candidates)
        self.given = multiplicity is not None
        self.pixels = 0
        self.replicates_used = 0

    # -- binding -----------------------------------------------------------------------------
    @property
    def n(self):
        """The fitted rows the table is bound to, else None."""
        return None if self._table is None else self._table.shape[1]

    def _bind(self, n):
        """Draw (or check) the table for ``n`` fitted rows; ``ValueError`` for another ``n``."""
        n = int(n)
        if self._table is not None:
            if self._table.shape[1] != n:
                raise ValueError(f"this Bootstrap is bound to n = {self._table.shape[1]} fitted rows: it cannot serve an "
                                 f"estimator with {n}")
            return self._table
        rng = np.random.default_rng(self.seed)
        if self.groups is None:
            rows = [np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(self.n_replicates)]
        else:
            from ._base import normalize_groups

            codes = normalize_groups(self.groups, n)
            g = int(codes.max()) + 1
            rows = [np.bincount(rng.integers(0, g, size=g), minlength=g)[codes] for _ in range(self.n_replicates)]
        self._table = np.ascontiguousarray(np.minimum(np.stack(rows), 255), dtype=np.uint8)
        self._table.setflags(write=False)
        return self._table

    def candidates(self, k, n_fit):
        """``kw`` of a call with replicate size ``k`` on ``n_fit`` searchable rows, refused when it cannot hold."""
        kw = min(int(n_fit), MAX_CANDIDATES, 4 * int(k) + 8) if self.n_candidates is None else self.n_candidates
        if k > kw:
            raise ValueError(f"bootstrap: n_neighbors = {k} exceeds n_candidates = {kw}: a replicate takes k of the kw "
                             "neighbours searched")
        if kw > n_fit:
            raise ValueError(f"bootstrap: n_candidates = {kw} exceeds the {n_fit} rows that can be neighbours")
        return kw

    @property
    def multiplicity(self):
        if self._table is None:
            raise ValueError("this Bootstrap has not been used yet: its table is drawn when the fitted rows are known")
        return self._table

    @property
    def share_short(self) -> float:
        total = self.pixels * self.n_replicates
        return float("nan") if total == 0 else 1.0 - self.replicates_used / total

    def _add(self, tally):
        self.pixels += int(tally[0])
        self.replicates_used += int(tally[1])
        return self

    # -- value semantics ---------------------------------------------------------------------------
    def __setstate__(self, state):
        self.__dict__.update(state)
        if self._table is not None:  # (an unpickled array comes back writable)
            self._table.setflags(write=False)

    def _key(self):
        g = None if self.groups is None else (str(self.groups.dtype), self.groups.tolist())
        t = None if not self.given else self._table.tobytes()
        return (self.n_replicates, self.seed if not self.given else None, g, self.n_candidates, self.given, t)

    def __iadd__(self, other):
        if not isinstance(other, Bootstrap):
            return NotImplemented
        if self._key() != other._key() or (self.n is not None and other.n is not None and self.n != other.n):
            raise ValueError("only the tallies of the same bootstrap (replicates, seed, groups, table, n_candidates) add up")
        return self._add((other.pixels, other.replicates_used))

    def __eq__(self, other):
        if not isinstance(other, Bootstrap):
            return NotImplemented
        same_table = (self._table is None) == (other._table is None) and (
            self._table is None or np.array_equal(self._table, other._table))
        return bool(self._key() == other._key() and same_table and self.pixels == other.pixels
                    and self.replicates_used == other.replicates_used)

    def __repr__(self):
        bound = "unbound" if self._table is None else f"n={self.n}"
        return (f"Bootstrap(n_replicates={self.n_replicates}, n_candidates={self.n_candidates}, {bound}, "
                f"pixels={self.pixels}, share_short={self.share_short:.4g})")


def normalize_boot_outputs(outputs, n_targets):
    """``outputs`` of a ``bootstrap=`` call as ``(cols, codes)`` int32 arrays (``_native.BOOT_STATISTICS`` codes): a sequence
    of ``(target, "boot_se" | "boot_mean" | "boot_bias")`` pairs and ``"boot_count"``; ``None``: ``boot_se`` of every target."""
    from ._native import BOOT_STATISTICS

    if outputs is None:
        outputs = [(j, "boot_se") for j in range(n_targets)]
    if isinstance(outputs, str) or not hasattr(outputs, "__iter__"):
        outputs = [outputs]
    outputs = list(outputs)
    if not 1 <= len(outputs) <= 1024:
        raise ValueError(f"outputs must hold 1 to 1024 entries, got {len(outputs)}")
    cols, codes = [], []
    for e, entry in enumerate(outputs):
        if isinstance(entry, str):
            if entry != "boot_count":
                raise ValueError(f"outputs[{e}] = {entry!r}: with bootstrap= an entry is (target, 'boot_se' | 'boot_mean' | "
                                 "'boot_bias') or 'boot_count'")
            cols.append(0)
            codes.append(BOOT_STATISTICS[entry])
            continue
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"outputs[{e}] = {entry!r}: an entry is a (target, statistic) pair or 'boot_count'")
        j, s = entry
        if not isinstance(s, str) or s not in BOOT_OUTPUTS:
            raise ValueError(f"outputs[{e}]: statistic {s!r} is not available with bootstrap=: use 'boot_se', 'boot_mean', "
                             "'boot_bias' or the entry 'boot_count'")
        if isinstance(j, (bool, float)) or not isinstance(j, (int, np.integer)):
            raise TypeError(f"outputs[{e}]: the target must be an integer column position, got {j!r}")
        if not 0 <= int(j) < n_targets:
            raise ValueError(f"outputs[{e}]: target {j} outside [0, {n_targets})")
        cols.append(int(j))
        codes.append(BOOT_STATISTICS[s])
    return np.array(cols, dtype=np.int32), np.array(codes, dtype=np.int32)


def has_boot_names(statistic, outputs) -> bool:
    """A ``boot_*`` name somewhere in ``statistic`` / ``outputs`` (of a call without ``bootstrap=``)."""
    def walk(x):
        if isinstance(x, str):
            return x.startswith("boot_")
        if isinstance(x, (tuple, list)):
            return any(walk(v) for v in x)
        return False

    return walk(statistic) or walk(outputs)
