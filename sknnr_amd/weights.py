"""Distance-weight laws: ``weights=`` objects that are ordinary callables -- scikit-learn and the reference take them
as any ``weights`` function -- and that the engine recognises and evaluates on the device.

A plain Python callable runs on the host between the search and the reduction, so every streamed feature of
``predict_chunks`` (``nodata``, ``layout="bands"``, typed outputs, ``return_neighbors``) refuses it.  A law is a short
chain of correctly rounded float64 operations on the distance, which the device reproduces bit for bit
(``csrc/weights.hip.h``); an estimator fitted with one predicts wherever ``weights="distance"`` does.

===============================  ==========================  ==============================================
class                            parameters                  ``w(d)`` (float64, as numpy evaluates it)
===============================  ==========================  ==============================================
``InverseDistance(offset=1.0)``  ``offset`` finite, > 0      ``1.0 / (offset + d)`` (yaImpute's at ``offset=1``)
``InverseSquaredDistance(...)``  ``offset`` finite, > 0      ``1.0 / (offset + d * d)``
``Triangular(bandwidth)``        ``bandwidth`` finite, > 0   ``np.maximum(0.0, 1.0 - d / bandwidth)``
``Epanechnikov(bandwidth)``      ``bandwidth`` finite, > 0   ``u = d / bandwidth; np.maximum(0.0, 1.0 - u * u)``
===============================  ==========================  ==============================================

``Triangular`` and ``Epanechnikov`` are compact: every neighbour of a query may lie at or beyond the bandwidth, all
its weights are then zero and its prediction is NaN (``0 / 0``), exactly as scikit-learn gives it (``can_vanish``).
"""

from __future__ import annotations

import math

import numpy as np

__all__ = ["DistanceWeights", "InverseDistance", "InverseSquaredDistance", "Triangular", "Epanechnikov"]


def _is_torch(d) -> bool:
    return type(d).__module__.startswith("torch")


class DistanceWeights:
    """Base class of the laws.  A subclass names its one parameter (``_param``), its native code (``code``:
    ``sknnr_weight_law`` of ``include/sknnr_hip.h``) and evaluates the law in ``_law`` with operators that numpy arrays
    and torch tensors share; ``_floor`` clamps at zero in either."""

    code = 0  # sknnr_weight_law; ``name``: its key in ``_native.WEIGHT_LAWS``
    name = "none"
    can_vanish = False  # overridden (read-only) by the compact laws
    _param = "offset"

    def __init__(self, value):
        try:
            v = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{type(self).__name__}: {self._param} must be a finite number > 0, got {value!r}") from None
        if not math.isfinite(v) or not v > 0.0:
            raise ValueError(f"{type(self).__name__}: {self._param} must be finite and > 0, got {value!r}")
        self._value = v

    # ---- the law ---------------------------------------------------------------------------------------------------
    def _law(self, d, p):
        raise NotImplementedError

    @staticmethod
    def _floor(x):
        if _is_torch(x):
            import torch

            return torch.maximum(torch.zeros((), dtype=x.dtype, device=x.device), x)
        return np.maximum(0.0, x)

    def __call__(self, dist):
        """float64 weights of the input's shape: numpy array (or anything ``np.asarray`` takes) -> numpy array, torch
        tensor -> torch tensor on its device."""
        if _is_torch(dist):
            import torch

            # (the parameter as a 0-d tensor on the input's device: torch divides a CUDA tensor by a Python scalar by
            #  multiplying with its reciprocal, which rounds differently; tensor / tensor is the IEEE division)
            p = torch.full((), self._value, dtype=torch.float64, device=dist.device)
            return self._law(dist.to(torch.float64), p)
        d = np.asarray(dist, dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):  # (d * d may overflow to inf: the weight is then 0)
            return np.asarray(self._law(d, self._value), dtype=np.float64)

    # ---- what the engine reads -------------------------------------------------------------------------------------
    @property
    def params(self) -> tuple:
        """The two float64 parameters the kernel takes (the second is unused by every law so far)."""
        return (self._value, 0.0)

    # ---- value semantics: equality, hash, repr, clone, pickle --------------------------------------------------------
    def get_params(self, deep=True) -> dict:
        return {self._param: self._value}

    def set_params(self, **params):
        for name, v in params.items():
            if name != self._param:
                raise ValueError(f"invalid parameter {name!r} for {type(self).__name__}")
            type(self).__init__(self, v)
        return self

    def __eq__(self, other):
        if type(other) is not type(self):
            return NotImplemented
        return self._value == other._value

    def __hash__(self):
        return hash((type(self).__name__, self._value))

    def __repr__(self):
        return f"{type(self).__name__}({self._param}={self._value!r})"

    def __reduce__(self):
        return (type(self), (self._value,))


class _OffsetLaw(DistanceWeights):
    _param = "offset"

    def __init__(self, offset=1.0):
        super().__init__(offset)

    @property
    def offset(self) -> float:
        return self._value

    @property
    def can_vanish(self) -> bool:
        return False


class _BandwidthLaw(DistanceWeights):
    _param = "bandwidth"

    def __init__(self, bandwidth):
        super().__init__(bandwidth)

    @property
    def bandwidth(self) -> float:
        return self._value

    @property
    def can_vanish(self) -> bool:
        """True: a query whose neighbours all lie at or beyond the bandwidth has an all-zero row and predicts NaN."""
        return True


class InverseDistance(_OffsetLaw):
    """``1.0 / (offset + d)``; ``offset=1`` is yaImpute's distance weighting."""

    code = 1
    name = "inverse"

    def _law(self, d, p):
        return 1.0 / (p + d)


class InverseSquaredDistance(_OffsetLaw):
    """``1.0 / (offset + d * d)``."""

    code = 2
    name = "inverse_squared"

    def _law(self, d, p):
        return 1.0 / (p + d * d)


class Triangular(_BandwidthLaw):
    """``np.maximum(0.0, 1.0 - d / bandwidth)``."""

    code = 3
    name = "triangular"

    def _law(self, d, p):
        return self._floor(1.0 - d / p)


class Epanechnikov(_BandwidthLaw):
    """``u = d / bandwidth; np.maximum(0.0, 1.0 - u * u)``."""

    code = 4
    name = "epanechnikov"

    def _law(self, d, p):
        u = d / p
        return self._floor(1.0 - u * u)
