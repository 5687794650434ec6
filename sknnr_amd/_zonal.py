"""Zonal statistics of a streamed map: per zone (stand, ownership, county ...) and output plane the count, sum, spread,
minimum and maximum of the stored values, and the class areas of class planes.

The contract of the numbers is stated once, in ``include/sknnr_hip.h`` ("Zonal statistics"); the device tallies them
(``sknnr_amd/csrc/zonal.hip.h``) and :class:`ZonalStats` is the small host-side object they are collected in."""

from __future__ import annotations

import numpy as np

_I64_MAX, _I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
_STORED_DTYPES = tuple(np.dtype(t) for t in (np.int16, np.uint16, np.uint8, np.int32))
COUNT, SUM, SQ_LO, SQ_HI, MIN, MAX = range(6)  # acc[z, j, :]


def empty_acc(n_zones, n_planes):
    """Accumulators nothing was added to: zeros, and the min / max sentinels INT64_MAX / INT64_MIN."""
    acc = np.zeros((int(n_zones), int(n_planes), 6), dtype=np.int64)
    acc[..., MIN] = _I64_MAX
    acc[..., MAX] = _I64_MIN
    return acc


class ZonalStats:
    """Zonal tables of any number of streamed ``predict_chunks`` calls over ``n_zones`` zones, codes ``0 .. n_zones - 1``.

    Pass one as ``zonal=`` with ``zones=`` (the zone codes of every tile) to ``predict_chunks``: the call adds what it
    tallied on the device and returns and writes exactly what it does without it.  The sums are over the STORED integer
    values of the typed output (``rint(pred * scale + offset)``, clamped), so they are exact, independent of tile cuts and
    equal to what a zonal-statistics tool computes from the written raster; nodata pixels and pixels whose zone code is
    outside ``[0, n_zones)`` contribute nothing.

    ``classes``: ``{plane: n_classes}`` -- those output planes are class codes (e.g. a ``mode`` statistic) and also get
    ``hist[plane]``, the pixels per zone and class ``0 .. n_classes - 1``.  ``labels``: one label per zone, kept for the
    user (``None``: the codes).

    The first use binds ``(n_planes, out_dtype, scale, offset, classes)``; a later use with another binding raises
    ``ValueError`` before any device work.

    Exact, int64 (Python ints where 64 bits may not do):
      ``count``, ``sum_stored``, ``min_stored``, ``max_stored``  ``(n_zones, n_planes)``; ``hist[plane]``
      ``(n_zones, n_classes)``.  ``min_stored`` / ``max_stored`` hold INT64_MAX / INT64_MIN where ``count == 0``.
    In data units, ``(stored - offset) / scale``, float64, NaN where ``count == 0``:
      ``mean``, ``total``, ``std`` (the population standard deviation; the variance's numerator ``count * sum(q^2) -
      sum(q)^2`` is computed in exact integer arithmetic before any float), ``min``, ``max``.

    Instances compare by value, pickle, and merge with ``+=``."""

    __hash__ = None

    def __init__(self, n_zones, classes=None, labels=None):
        n_zones = int(n_zones)
        if n_zones < 1:
            raise ValueError(f"n_zones must be >= 1, got {n_zones}")
        self.n_zones = n_zones
        self.classes = {}
        for plane, n in dict(classes or {}).items():
            if int(plane) != plane or int(plane) < 0 or int(n) != n or int(n) < 1:
                raise ValueError(f"classes maps a plane (>= 0) to its number of classes (>= 1), got {plane!r}: {n!r}")
            self.classes[int(plane)] = int(n)
        if labels is not None:
            labels = list(labels)
            if len(labels) != n_zones:
                raise ValueError(f"labels must hold one label per zone ({n_zones}), got {len(labels)}")
        self.labels = labels
        self._binding = None  # (n_planes, dtype, scale tuple, offset tuple)
        self._acc = None      # (n_zones, n_planes, 6) int64
        self._hist = {}       # plane -> (n_zones, n_classes) int64

    # -- binding -----------------------------------------------------------------------------
    @staticmethod
    def _normalize(n_planes, dtype, scale, offset):
        n_planes = int(n_planes)
        dtype = np.dtype(dtype)
        if dtype not in _STORED_DTYPES:
            raise ValueError(f"zonal sums are over stored integers: out_dtype must be int16, uint16, uint8 or int32, got {dtype}")

        def per_plane(v, default):
            v = np.full(n_planes, default, dtype=np.float64) if v is None else np.asarray(v, dtype=np.float64).reshape(-1)
            if v.size == 1:
                v = np.full(n_planes, v[0], dtype=np.float64)
            if v.size != n_planes:
                raise ValueError(f"scale / offset must be scalars or hold one value per plane ({n_planes}), got {v.size}")
            return tuple(float(x) for x in v)
        return n_planes, dtype, per_plane(scale, 1.0), per_plane(offset, 0.0)

    def _check(self, n_planes, dtype, scale=None, offset=None):
        """The binding this use needs; ``ValueError`` where the object is bound to another, or ``classes`` names a plane
        the output does not have."""
        binding = self._normalize(n_planes, dtype, scale, offset)
        missing = sorted(p for p in self.classes if p >= binding[0])
        if missing:
            raise ValueError(f"classes names plane {missing[0]}: the output has {binding[0]} plane(s)")
        if self._binding is not None and self._binding != binding:
            raise ValueError(f"this ZonalStats is bound to (n_planes, out_dtype, scale, offset) = {self._binding}: it cannot "
                             f"take a tally of {binding}")
        return binding

    def _bind(self, n_planes, dtype, scale=None, offset=None):
        binding = self._check(n_planes, dtype, scale, offset)
        if self._binding is None:
            self._binding = binding
            self._acc = empty_acc(self.n_zones, binding[0])
            self._hist = {p: np.zeros((self.n_zones, n), dtype=np.int64) for p, n in sorted(self.classes.items())}
        return self

    def n_classes(self, n_planes):
        """The C ABI's ``n_classes``: one count per plane, 0 for a numeric plane; None without classes."""
        if not self.classes:
            return None
        out = np.zeros(int(n_planes), dtype=np.int32)
        for p, n in self.classes.items():
            out[p] = n
        return out

    def _add(self, acc, hist=None):
        """Add one tally in the C ABI's form: ``acc`` ``(n_zones, n_planes, 6)``, ``hist`` the flat class blocks in plane
        order (or None).  The object must be bound."""
        self._require()
        acc = np.asarray(acc, dtype=np.int64)
        if acc.shape != self._acc.shape:
            raise ValueError(f"acc must be {self._acc.shape}, got {acc.shape}")
        self._acc[..., :MIN] += acc[..., :MIN]
        np.minimum(self._acc[..., MIN], acc[..., MIN], out=self._acc[..., MIN])
        np.maximum(self._acc[..., MAX], acc[..., MAX], out=self._acc[..., MAX])
        if self._hist:
            hist = np.asarray(hist, dtype=np.int64).reshape(-1)
            at = 0
            for p, block in self._hist.items():
                block += hist[at:at + block.size].reshape(block.shape)
                at += block.size
        return self

    def _require(self):
        if self._binding is None:
            raise ValueError("this ZonalStats has tallied nothing yet: it has no planes")

    # -- the exact numbers ---------------------------------------------------------------------
    @property
    def n_planes(self):
        """Output planes once bound, else None."""
        return None if self._binding is None else self._binding[0]

    @property
    def out_dtype(self):
        return None if self._binding is None else self._binding[1]

    @property
    def scale(self):
        self._require()
        return np.array(self._binding[2])

    @property
    def offset(self):
        self._require()
        return np.array(self._binding[3])

    @property
    def acc(self):
        """The accumulators as the C ABI holds them, ``(n_zones, n_planes, 6)`` int64."""
        self._require()
        return self._acc

    @property
    def count(self):
        return self.acc[..., COUNT]

    @property
    def sum_stored(self):
        return self.acc[..., SUM]

    @property
    def min_stored(self):
        return self.acc[..., MIN]

    @property
    def max_stored(self):
        return self.acc[..., MAX]

    @property
    def hist(self):
        """``{plane: (n_zones, n_classes) int64}`` of the class planes."""
        self._require()
        return self._hist

    def sum_squares_stored(self):
        """The exact sum of the squared stored values, as Python ints (object array): ``sq_hi * 2**32 + sq_lo``."""
        hi = self.acc[..., SQ_HI].astype(object)
        return hi * (1 << 32) + self.acc[..., SQ_LO].astype(object)

    # -- data units -------------------------------------------------------------------------------
    def _where_counted(self, values):
        return np.where(self.count > 0, values, np.nan)

    def _unscale(self, stored):
        return (stored - self.offset) / self.scale

    @property
    def mean(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._where_counted(self._unscale(self.sum_stored / self.count))

    @property
    def total(self):
        return self._where_counted((self.sum_stored - self.count * self.offset) / self.scale)

    @property
    def std(self):
        n = self.count.astype(object)
        s = self.sum_stored.astype(object)
        num = n * self.sum_squares_stored() - s * s  # exact: Python ints
        var = np.array([[int(a) / (int(b) * int(b)) if b else np.nan for a, b in zip(ra, rb)] for ra, rb in zip(num, n)],
                       dtype=np.float64).reshape(self.count.shape)
        return np.sqrt(var) / np.abs(self.scale)

    def _extreme(self, pick):
        lo, hi = self._unscale(self.min_stored.astype(np.float64)), self._unscale(self.max_stored.astype(np.float64))
        return self._where_counted(pick(lo, hi))  # (a negative scale turns the two around)

    @property
    def min(self):
        return self._extreme(np.minimum)

    @property
    def max(self):
        return self._extreme(np.maximum)

    # -- value semantics ---------------------------------------------------------------------------
    def __iadd__(self, other):
        if not isinstance(other, ZonalStats):
            return NotImplemented
        if other.n_zones != self.n_zones or other.classes != self.classes:
            raise ValueError(f"cannot merge ZonalStats of {other.n_zones} zones and classes {other.classes} into one of "
                             f"{self.n_zones} zones and classes {self.classes}")
        if other._binding is None:
            return self
        self._bind(other._binding[0], other._binding[1], other._binding[2], other._binding[3])
        flat = np.concatenate([h.reshape(-1) for h in other._hist.values()]) if other._hist else None
        return self._add(other._acc, flat)

    def __eq__(self, other):
        if not isinstance(other, ZonalStats):
            return NotImplemented
        if (self.n_zones, self.classes, self.labels, self._binding) != (other.n_zones, other.classes, other.labels,
                                                                          other._binding):
            return False
        if self._binding is None:
            return True
        return bool(np.array_equal(self._acc, other._acc)
                    and all(np.array_equal(h, other._hist[p]) for p, h in self._hist.items()))

    def __repr__(self):
        if self._binding is None:
            return f"ZonalStats(n_zones={self.n_zones}, unbound)"
        n_planes, dtype = self._binding[:2]
        return (f"ZonalStats(n_zones={self.n_zones}, n_planes={n_planes}, out_dtype={dtype}, "
                f"pixels={int(self.count[:, 0].sum())}, empty_zones={int((self.count[:, 0] == 0).sum())})")
