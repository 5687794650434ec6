"""Estimator surface of the MI355X backend: the reference's L3 layer re-stated over
:class:`sknnr_amd._engine.KNNEngine`.

Mirrors /root/reference/src/sknnr/_base.py -- same class names, constructor parameters,
method signatures, fitted attributes and error messages -- but no arithmetic of the
hot path happens in Python or scikit-learn: ``kneighbors`` / ``predict`` / the fit-time
independent prediction are launches of ``libsknnr_hip.so``.  There is no CPU fallback;
metrics other than Euclidean raise.

    RawKNNRegressor                  REF _base.py:43-182
    TransformedKNeighborsRegressor   REF _base.py:185-358
    YFitMixin                        REF _base.py:361-374
    OrdinationKNeighborsRegressor    REF _base.py:377-408
"""

from __future__ import annotations

import numbers
from abc import ABC, abstractmethod
from typing import NamedTuple

import numpy as np
from sklearn.base import BaseEstimator, MultiOutputMixin, RegressorMixin
from sklearn.exceptions import NotFittedError
from sklearn.metrics import r2_score
from sklearn.utils.validation import _is_arraylike, check_is_fitted, validate_data

from . import _config, _native
from ._engine import KNNEngine, default_device, is_torch_cuda_tensor
from ._usage import NeighborUsage
from ._domain import DistanceDomain
from ._bootstrap import MAX_CANDIDATES, Bootstrap, has_boot_names, normalize_boot_outputs
from ._products import StreamProducts, normalize_zone_tile  # noqa: F401  (normalize_zone_tile: the zone rule, beside the tile rules)
from .weights import DistanceWeights

# Element types query rows may keep on their way to the device (include/sknnr_hip.h, sknnr_dtype): the kernel that reads
# them widens to float64, exactly -- the reference's host-side conversion (validate_data(dtype=FLOAT_DTYPES) followed by
# float64 arithmetic, REF transformers/_cca_transformer.py:78-87) without the host pass and at the rows' own PCIe width.
# Anything else (int64, bool, float16, ...) is converted to float64 by validate_data as before.
_QUERY_DTYPES = [np.float64, np.float32, np.int16, np.uint16, np.uint8, np.int32]

_EUCLIDEAN_NAMES = {"euclidean", "l2"}
_ALGORITHMS = {"auto", "brute", "kd_tree", "ball_tree"}


def _effective_metric(metric, p, metric_params):
    """The Euclidean metric (SKL/neighbors/_base.py:429-472 maps minkowski/p=2 to 'euclidean') and the
    weighted Hamming metric of the tree-based estimators (REF _weighted_trees.py:53-59) exist on the
    device."""
    if metric == "hamming":
        extra = set(metric_params or {}) - {"w"}
        if extra:
            raise NotImplementedError(f"metric_params {sorted(extra)} are not supported with metric='hamming'")
        return "hamming"
    if metric_params:
        raise NotImplementedError(
            "metric_params are not supported by the MI355X backend (Euclidean metric only)")
    if callable(metric):
        raise NotImplementedError(
            "callable metrics are not supported by the MI355X backend (Euclidean metric only)")
    if metric == "minkowski":
        if p != 2:
            raise NotImplementedError(
                f"minkowski with p={p} is not supported by the MI355X backend (p must be 2)")
        return "euclidean"
    if metric in _EUCLIDEAN_NAMES:
        return "euclidean"
    raise NotImplementedError(
        f"metric={metric!r} is not supported by the MI355X backend (Euclidean metric only)")


def normalize_nodata(nodata, n_features, dtype):
    """The ``nodata`` argument of the streamed calls as float64 ``(n_features,)``: a scalar stands for every column, a
    sequence gives one value per RAW input column (before any affine or forest map).  A row is masked when any column
    equals its value; a NaN entry means "NaN in that column is nodata", which only float rows can hold: for an integer
    ``dtype`` it is refused."""
    try:
        arr = np.asarray(nodata, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError(f"nodata must be a number or a sequence of {n_features} numbers, got {nodata!r}") from err
    if arr.ndim == 0:
        arr = np.full(n_features, float(arr), dtype=np.float64)
    elif arr.ndim != 1 or arr.shape[0] != n_features:
        raise ValueError(f"nodata must be a scalar or hold one value per input column: expected {n_features}, "
                         f"got shape {arr.shape}")
    if np.dtype(dtype).kind in "iub":
        bad = np.flatnonzero(np.isnan(arr))
        if bad.size:
            raise ValueError(f"nodata for column {int(bad[0])} is NaN, but the rows are {np.dtype(dtype)}: an integer "
                             "column cannot hold NaN")
    return np.ascontiguousarray(arr)


_LAYOUTS = ("rows", "bands")


# typed outputs of the streamed calls: what the device narrows to (include/sknnr_hip.h, "typed outputs")
_OUT_VALUE_DTYPES = tuple(np.dtype(t) for t in (np.float32, np.int16, np.uint16, np.uint8, np.int32))


def _narrow_dtype(dt, wide, allowed, name):
    """``dt`` as a numpy dtype the device narrows ``wide`` results to; None for None or ``wide`` itself (as ever)."""
    if dt is None:
        return None
    try:
        dt = np.dtype(dt)
    except TypeError:
        raise ValueError(f"{name}={dt!r} is not a numpy dtype") from None
    if dt == np.dtype(wide):
        return None
    if dt not in allowed:
        raise ValueError(f"{name}={dt} is not supported: use {', '.join(str(a) for a in allowed)} or {np.dtype(wide)}")
    return dt


def _representable(value, dt) -> bool:
    """Can ``value`` be stored in ``dt`` exactly (NaN: in a float type)?"""
    dt = np.dtype(dt)
    try:
        value = float(value)
    except (TypeError, ValueError):
        return False
    if dt.kind == "f":
        return bool(np.isnan(value) or float(dt.type(value)) == value) if np.isfinite(value) or np.isnan(value) else True
    info = np.iinfo(dt)
    return bool(np.isfinite(value) and value == np.rint(value) and info.min <= value <= info.max)


def normalize_typed_output(out_dtype, scale, offset, out_nodata, n_targets, masked):
    """The ``output`` arguments of a typed prediction stream (:meth:`sknnr_amd._native.QueryStream.set_output`), or None
    when the predictions leave as ever.  ``masked``: the call has a ``nodata`` mask, so NaN predictions occur."""
    dt = _narrow_dtype(out_dtype, np.float64, _OUT_VALUE_DTYPES, "out_dtype")
    if dt is None:
        for name, v in (("scale", scale), ("offset", offset), ("out_nodata", out_nodata)):
            if v is not None:
                raise ValueError(f"{name} needs out_dtype: float64 predictions leave as they are computed")
        return None
    if scale is not None or offset is not None:
        def per_target(v, default, name):
            v = np.full(n_targets, default, dtype=np.float64) if v is None else np.asarray(v, dtype=np.float64).reshape(-1)
            if v.size == 1:
                v = np.full(n_targets, v[0], dtype=np.float64)
            if v.size != n_targets:
                raise ValueError(f"{name} must be a scalar or hold one value per target ({n_targets}), got {v.size}")
            return np.ascontiguousarray(v)
        scale, offset = per_target(scale, 1.0, "scale"), per_target(offset, 0.0, "offset")
    if out_nodata is None:
        if dt.kind != "f" and masked:
            raise ValueError(f"out_nodata is required with nodata and out_dtype={dt}: an integer type has no NaN for "
                             "the masked rows")
    elif not _representable(out_nodata, dt):
        raise ValueError(f"out_nodata={out_nodata!r} is not representable in out_dtype={dt}")
    elif dt.kind == "f" and np.isnan(float(out_nodata)):
        out_nodata = None  # (NaN stays NaN)
    return dict(pred_dtype=dt, scale=scale, offset=offset, fill=None if out_nodata is None else float(out_nodata))


def normalize_statistic(statistic, n_targets):
    """``statistic`` of ``summarize`` / ``predict_chunks`` -- one name of ``_native.STATISTICS`` or one name per target
    -- as the int32 codes the engine takes; every refusal comes before any device work."""
    names = [statistic] * n_targets if isinstance(statistic, str) else statistic
    try:
        names = list(names)
    except TypeError:
        raise ValueError(f"statistic must be a name or a sequence of names, one per target, got {statistic!r}") from None
    for name in names:
        if not isinstance(name, str):
            raise ValueError(f"statistic entries must be strings, got {name!r}")
        if name not in _native.STATISTICS:
            raise ValueError(f"unknown statistic {name!r}: use one of {', '.join(_native.STATISTICS)}")
    if len(names) != n_targets:
        raise ValueError(f"statistic must be one name or hold one name per target ({n_targets}), got {len(names)}")
    return np.array([_native.STATISTICS[name] for name in names], dtype=np.int32)


class OutputPlan(NamedTuple):
    """An output plan as the engine takes it (``cols`` int32, ``codes`` int32 of ``_native.PLAN_STATISTICS``, ``params``
    float64, one entry per output plane).  ``per_target``: it stands for a ``statistic=`` argument -- entry j is target j
    -- and the result keeps that argument's shape rules; else the result is always 2-D."""
    cols: np.ndarray
    codes: np.ndarray
    params: np.ndarray
    per_target: bool = False

    @property
    def n_out(self) -> int:
        return int(self.cols.size)

    @property
    def arrays(self):
        return self.cols, self.codes, self.params


def _is_quantile_spec(s) -> bool:
    return (isinstance(s, (tuple, list)) and len(s) == 2 and isinstance(s[0], str) and s[0] == "quantile"
            and isinstance(s[1], numbers.Real) and not isinstance(s[1], bool))


def _plan_statistic(s, where, median=True):
    """One statistic of a plan entry -- one of the six names, ``"median"`` (unless ``median`` is off) or
    ``("quantile", q)`` -- as (code, param)."""
    if _is_quantile_spec(s):
        q = float(s[1])
        if not (0.0 <= q <= 1.0):  # (NaN fails both comparisons)
            raise ValueError(f"{where}: a quantile's q must lie in [0, 1], got {s[1]!r}")
        return _native.PLAN_STATISTICS["quantile"], q
    if median and isinstance(s, str) and s == "median":
        return _native.PLAN_STATISTICS["quantile"], 0.5
    if isinstance(s, str) and s in _native.STATISTICS:
        return _native.STATISTICS[s], 0.0
    raise ValueError(f"{where}: unknown statistic {s!r}: use one of {', '.join(_native.STATISTICS)}"
                     f"{', ' + repr('median') if median else ''} or ('quantile', q)")


def normalize_outputs(outputs, n_targets):
    """``outputs`` of ``summarize`` / ``predict_chunks`` -- a sequence of ``(target, statistic)`` pairs: ``target`` an
    integer column position (it may repeat, in any order), ``statistic`` one of the ``_native.STATISTICS`` names,
    ``"median"`` or ``("quantile", q)`` with ``0 <= q <= 1`` -- as the ``(cols int32, codes int32, params float64)``
    arrays the engine takes; every refusal comes before any device work."""
    if isinstance(outputs, str):
        raise ValueError(f"outputs must be a sequence of (target, statistic) pairs, got {outputs!r}")
    try:
        entries = list(outputs)
    except TypeError:
        raise ValueError(f"outputs must be a sequence of (target, statistic) pairs, got {outputs!r}") from None
    if not entries:
        raise ValueError("outputs must hold at least one (target, statistic) pair")
    if len(entries) > _native.PLAN_MAX_OUT:
        raise ValueError(f"outputs must hold at most {_native.PLAN_MAX_OUT} entries, got {len(entries)}")
    cols, codes, params = [], [], []
    for e, entry in enumerate(entries):
        if isinstance(entry, str) or not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"outputs[{e}] must be a (target, statistic) pair, got {entry!r}")
        target, stat = entry
        if isinstance(target, bool) or not isinstance(target, numbers.Integral):
            raise ValueError(f"outputs[{e}]: the target must be an integer column position, got {target!r}")
        if not 0 <= int(target) < n_targets:
            raise ValueError(f"outputs[{e}]: target {int(target)} is outside [0, {n_targets})")
        code, param = _plan_statistic(stat, f"outputs[{e}]")
        cols.append(int(target))
        codes.append(code)
        params.append(param)
    return np.array(cols, dtype=np.int32), np.array(codes, dtype=np.int32), np.array(params, dtype=np.float64)


def resolve_statistic(statistic, outputs, n_targets):
    """What ``summarize`` / ``predict_chunks`` reduce: ``statistic`` as the int32 codes of :func:`normalize_statistic`
    when no entry is a ``("quantile", q)`` (the per-target path, unchanged, with its refusals -- ``"median"`` among them:
    in ``statistic`` the median is spelled ``("quantile", 0.5)``), an :class:`OutputPlan` for ``outputs`` or for a
    ``statistic`` that holds ``("quantile", q)`` entries (the plan ``[(0, s0), ..., (t-1, s_(t-1))]``), or None when
    neither is given."""
    if has_boot_names(statistic, outputs):
        raise ValueError("the 'boot_*' outputs need bootstrap=: pass a sknnr_amd.Bootstrap")
    if outputs is not None:
        if statistic is not None:
            raise ValueError("outputs and statistic cannot be given together: outputs names the statistic of every plane")
        return OutputPlan(*normalize_outputs(outputs, n_targets))
    if statistic is None:
        return None
    new = _is_quantile_spec
    if new(statistic):
        names = [statistic] * n_targets
    elif isinstance(statistic, str):
        return normalize_statistic(statistic, n_targets)
    else:
        try:
            names = list(statistic)
        except TypeError:
            return normalize_statistic(statistic, n_targets)
        if not any(new(s) or (isinstance(s, (tuple, list)) and len(s) > 0 and s[0] == "quantile") for s in names):
            return normalize_statistic(names, n_targets)
    if len(names) != n_targets:
        raise ValueError(f"statistic must be one name or hold one name per target ({n_targets}), got {len(names)}")
    pairs = [_plan_statistic(s, f"statistic[{j}]", median=False) for j, s in enumerate(names)]
    return OutputPlan(np.arange(n_targets, dtype=np.int32), np.array([c for c, _ in pairs], dtype=np.int32),
                      np.array([q for _, q in pairs], dtype=np.float64), per_target=True)


def _check_layout(layout):
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be 'rows' or 'bands', got {layout!r}")
    return layout == "bands"


def normalize_band_tile(tile, n_bands, *, forest=False, estimator="the estimator"):
    """A band-first tile of a streamed call (``layout="bands"``) as ``(bands, n)``: ``n_bands`` 1-D C-contiguous arrays of
    one dtype, and their length.  ``tile`` is an array ``(bands, ...)`` of any trailing shape -- ``(bands, n)``,
    ``(bands, h, w)``; pixels are taken in C order of the trailing axes -- or a sequence of ``bands`` arrays of one shape
    and dtype.  A band of a dtype the device does not read (:data:`_QUERY_DTYPES`) is converted to float64 (``forest``:
    64-bit integers to float32, as ``_validate_forest_query`` does), a band that is not contiguous is copied; both band
    by band.  Nothing is transposed on the host."""
    if is_torch_cuda_tensor(tile) or (isinstance(tile, (list, tuple)) and any(is_torch_cuda_tensor(b) for b in tile)):
        raise TypeError("streamed tiles are host arrays (they travel through the pinned "
                        "PCIe pipeline); pass CUDA tensors to kneighbors() / predict()")
    if isinstance(tile, np.ndarray):
        if tile.ndim < 2:
            raise ValueError(f"a band-first tile is an array (bands, ...) or a sequence of bands, got shape {tile.shape}")
        bands = [tile[j] for j in range(tile.shape[0])]
    else:
        try:
            bands = [np.asarray(b) for b in tile]
        except TypeError as err:
            raise ValueError("a band-first tile is an array (bands, ...) or a sequence of bands, got "
                             f"{type(tile).__name__}") from err
    if len(bands) != n_bands:
        raise ValueError(f"X has {len(bands)} features, but {estimator} is expecting {n_bands} features as input.")
    shape, dtype = bands[0].shape, bands[0].dtype
    for j, b in enumerate(bands):
        if b.shape != shape or b.dtype != dtype:
            raise ValueError(f"the bands of a tile must share one shape and dtype: band {j} is {b.dtype} {b.shape}, "
                             f"band 0 {dtype} {shape}")
    if dtype not in _QUERY_DTYPES:
        dtype = np.dtype(np.float32 if forest and dtype in (np.int64, np.uint64) else np.float64)
    # (ascontiguousarray copies only a band that is strided or of another dtype; reshape of a contiguous band is a view)
    bands = [np.ascontiguousarray(b, dtype=dtype).reshape(-1) for b in bands]
    return bands, int(bands[0].shape[0])


def _empty_row_tile(tile) -> bool:
    """A row tile ``(0, n_features)``: a window that holds no pixel.  A streamed call skips it, as it skips an empty
    band-first tile, before scikit-learn's validation, which refuses arrays without rows."""
    shape = getattr(tile, "shape", None)
    return shape is not None and len(shape) == 2 and shape[0] == 0


def _out_window(arr, row, n, cols, dtype, bands, noun):
    """Rows ``[row, row + n)`` of a preallocated output ``arr`` (None: None) of ``cols`` columns -- with ``bands`` its
    columns of ``cols`` planes, which stay one full row of ``arr`` apart -- refused unless C-contiguous, of ``dtype`` and
    long enough.  ``noun``: what the refusal calls the array."""
    if arr is None:
        return None
    if bands:
        if arr.ndim != 2 or arr.shape[0] != cols or arr.dtype != dtype or not arr.flags.c_contiguous \
                or arr.shape[1] < row + n:
            raise ValueError(f"{noun} must be C-contiguous, {np.dtype(dtype)}, with {cols} rows and at least "
                             f"{row + n} columns")
        return arr[:, row:row + n]
    w = arr[row:row + n]
    if w.shape != (n, cols) or w.dtype != dtype or not w.flags.c_contiguous:
        raise ValueError(f"{noun} must be C-contiguous, {np.dtype(dtype)}, with {cols} columns and at least "
                         f"{row + n} rows")
    return w


def _resolve_fit_method(algorithm, n_ref, d, k):
    """Which of the reference's engines -- hence which float64 distance expression -- the
    ``algorithm`` setting selects (SKL/neighbors/_base.py:620-648)."""
    if algorithm not in _ALGORITHMS:
        raise ValueError(f"unrecognized algorithm: {algorithm!r}")
    if algorithm != "auto":
        return algorithm
    if d > 15 or (k is not None and k >= n_ref // 2):
        return "brute"
    return "kd_tree"


def replay_reference_selection(full, kk, call_rows, self_query, deterministic, decimals):
    """The reference's selection on full distance rows, line by line, with this host's numpy.

    ``full`` (n, n_fit): float64 distance rows (computed on the device).  ``kk``: neighbours searched (k, + 1 for the X=None
    path).  ``call_rows`` (n): each row's position in the whole call (for X=None also its own reference index).
    Steps: ``_kneighbors_reduce_func`` (SKL/neighbors/_base.py:733-760: argpartition, then argsort of the kept
    distances), the X=None self removal (SKL/neighbors/_base.py:936-963) and sknnr's deterministic reorder
    (REF src/sknnr/_base.py:166-175).  Returns ``(dist, idx)`` with k columns.
    """
    n = full.shape[0]
    sample_range = np.arange(n)[:, None]
    neigh = np.argpartition(full, kk - 1, axis=1)[:, :kk]
    neigh = neigh[sample_range, np.argsort(full[sample_range, neigh])]
    nd = full[sample_range, neigh]
    return _finish_selection(nd, neigh, kk, call_rows, self_query, deterministic, decimals)


def _finish_selection(nd, neigh, kk, call_rows, self_query, deterministic, decimals):
    """The X=None self removal (SKL/neighbors/_base.py:936-963) and sknnr's deterministic reorder
    (REF src/sknnr/_base.py:166-175) on the ``kk`` selected rows of each query."""
    n = neigh.shape[0]
    call_rows = np.asarray(call_rows, dtype=np.int64)
    if self_query:
        sample_mask = neigh != call_rows[:, None]
        dup_gr_nbrs = np.all(sample_mask, axis=1)
        sample_mask[:, 0][dup_gr_nbrs] = False
        neigh = np.reshape(neigh[sample_mask], (n, kk - 1))
        nd = np.reshape(nd[sample_mask], (n, kk - 1))
    if deterministic:
        row_scale = np.maximum(nd.max(axis=1, keepdims=True), 1.0)
        rounded = np.round(nd / row_scale, decimals=decimals)
        diff = np.abs(neigh - call_rows[:, None])
        order = np.lexsort((neigh, diff, rounded), axis=1)
        nd = np.take_along_axis(nd, order, axis=1)
        neigh = np.take_along_axis(neigh, order, axis=1)
    return nd, neigh


def build_reference_tree(fit_X, algorithm, leaf_size):
    """The tree the reference's ``fit`` builds for ``algorithm`` (SKL/neighbors/_base.py:678-703; the Euclidean metric
    after the minkowski / p=2 mapping, SKL/neighbors/_base.py:544-559)."""
    from sklearn.neighbors import BallTree, KDTree

    cls = {"kd_tree": KDTree, "ball_tree": BallTree}[algorithm]
    return cls(np.ascontiguousarray(fit_X, dtype=np.float64), leaf_size, metric="euclidean")


def replay_tree_selection(fit_X, rows_X, kk, algorithm, leaf_size, call_rows, self_query, deterministic, decimals,
                          tree=None):
    """The reference's tree search for the rows ``rows_X`` (n, d), with its choice among exactly tied rows.

    ``fit_X``: the fitted (transformed) rows; ``rows_X``: the query rows in the same space (for X=None the fitted rows of
    the queries themselves).  ``kk``: neighbours searched (k, + 1 for the X=None path).  ``call_rows`` (n): each row's
    position in the whole call (for X=None also its own reference index).  Steps: ``KDTree`` / ``BallTree.query``
    (SKL/neighbors/_base.py:919-926), the X=None self removal and sknnr's reorder.  ``tree``: a tree from
    :func:`build_reference_tree` on the same ``fit_X`` (built here when None).  Returns ``(dist, idx)`` with k columns.
    """
    if tree is None:
        tree = build_reference_tree(fit_X, algorithm, leaf_size)
    rows_X = np.ascontiguousarray(rows_X, dtype=np.float64)
    nd, neigh = tree.query(rows_X, k=kk)
    return _finish_selection(nd, neigh.astype(np.int64, copy=False), kk, call_rows, self_query, deterministic, decimals)


def normalize_groups(groups, n_samples):
    """The int32 group codes of ``groups``, a 1-D array-like of ``n_samples`` labels (integers, strings, a pandas Series),
    as ``np.unique(..., return_inverse=True)`` numbers them.  ``ValueError`` for more than one dimension, a wrong length,
    a float array holding NaN and a single group."""
    g = groups.to_numpy() if hasattr(groups, "to_numpy") else np.asarray(groups)
    if g.ndim != 1:
        raise ValueError(f"groups must be 1-D with one label per fitted row, got an array of shape {g.shape}")
    if g.shape[0] != n_samples:
        raise ValueError(f"groups must hold one label per fitted row ({n_samples}), got {g.shape[0]}")
    if g.dtype.kind == "f" and np.isnan(g).any():
        raise ValueError(f"groups must not hold NaN, got {int(np.isnan(g).sum())} NaN labels")
    try:
        labels, codes = np.unique(g, return_inverse=True)
    except TypeError:
        raise ValueError(f"groups must hold labels that can be ordered, got dtype {g.dtype} with mixed types") from None
    if labels.size < 2:
        raise ValueError(f"groups must name at least two groups, got the single group {labels[0]!r}: "
                         "no fitted row would have a candidate")
    return np.ascontiguousarray(codes.reshape(-1), dtype=np.int32)


def normalize_buffer(buffer, n_samples):
    """``(coords, radius)`` of a buffered leave-out as the engine takes it: ``coords`` a C-contiguous float64
    ``(n_samples, c)`` array, ``c`` 1 to 3 (a 1-D array-like is one column), ``radius`` a float.  ``buffer`` is a pair
    ``(coords, radius)`` with ``coords`` an array-like or a pandas DataFrame of plot positions.  ``ValueError`` for anything
    but a pair, a wrong length, more than 3 or fewer than 1 columns, positions that are not finite numbers, and a radius that
    is negative, not finite or no scalar."""
    if not isinstance(buffer, (tuple, list)) or len(buffer) != 2:
        raise ValueError(f"buffer must be a pair (coords, radius), got {type(buffer).__name__}"
                         + (f" of length {len(buffer)}" if isinstance(buffer, (tuple, list)) else ""))
    coords, radius = buffer
    c = coords.to_numpy() if hasattr(coords, "to_numpy") else np.asarray(coords)
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    if c.ndim != 2:
        raise ValueError(f"buffer positions must be 2-D with one row per fitted row, got an array of shape {c.shape}")
    if c.shape[0] != n_samples:
        raise ValueError(f"buffer positions must hold one row per fitted row ({n_samples}), got {c.shape[0]}")
    if not 1 <= c.shape[1] <= 3:
        raise ValueError(f"buffer positions must have 1 to 3 columns, got {c.shape[1]}")
    try:
        c = np.ascontiguousarray(c, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"buffer positions must be numbers, got dtype {c.dtype}") from None
    if not np.isfinite(c).all():
        raise ValueError(f"buffer positions must be finite, got {int((~np.isfinite(c)).sum())} values that are not")
    if np.ndim(radius) != 0 or isinstance(radius, (str, bytes)) or radius is None:
        raise ValueError(f"buffer radius must be a scalar, got {radius!r}")
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"buffer radius must be a scalar, got {radius!r}") from None
    if not np.isfinite(r) or r < 0:
        raise ValueError(f"buffer radius must be finite and >= 0, got {r!r}")
    return c, r


def _reraise(err, estimator):
    """Map a native failure to the exception the reference raises for the same input."""
    if err.code == _native.ERR_K_TOO_LARGE:
        raise ValueError(err.message) from None
    if err.code == _native.ERR_NONFINITE:
        # scikit-learn's own wording, estimator-specific second sentence included
        # (SKL/utils/validation.py _assert_all_finite)
        from sklearn.utils.validation import check_array

        # (the forest map also reports values beyond the float32 range, as forest.apply's float32 validation does)
        bad = np.array([[np.nan if "NaN" in err.message else np.inf]],
                       dtype=np.float32 if "dtype('float32')" in err.message else np.float64)
        check_array(bad, estimator=estimator, input_name="X", ensure_min_features=1)
        raise ValueError(err.message) from None  # not reached
    raise err


class DFIndexCrosswalkMixin:
    """Capture of a dataframe's index at fit time (REF _base.py:23-30)."""

    def _set_dataframe_index_in(self, X) -> None:
        index = getattr(X, "index", None)
        if _is_arraylike(index):
            self.dataframe_index_in_ = np.asarray(index)


class RawKNNRegressor(DFIndexCrosswalkMixin, MultiOutputMixin, RegressorMixin, BaseEstimator):
    """k-nearest-neighbour regressor on the features as given, with sknnr's extras:
    dataframe-index crosswalk, fit-time independent prediction/score and deterministic
    neighbour ordering -- computed on the GPU.

    Same parameters as ``sklearn.neighbors.KNeighborsRegressor`` (REF _base.py:53-73);
    ``n_jobs`` is accepted and ignored (there is no thread pool), ``algorithm`` selects which of
    the reference's two float64 distance expressions is reproduced, and ``leaf_size`` shapes the
    host-side tree that ``tree_tie_policy("tree")`` queries for rows with exact ties (with the
    default policy there is no tree and ``leaf_size`` has no effect).
    """

    DISTANCE_PRECISION_DECIMALS = 10

    def __init__(self, n_neighbors=5, *, weights="uniform", algorithm="auto", leaf_size=30, p=2,
                 metric="minkowski", metric_params=None, n_jobs=None):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.p = p
        self.metric = metric
        self.metric_params = metric_params
        self.n_jobs = n_jobs

    # -- fitting -------------------------------------------------------------------------
    def _check_params(self):
        if not isinstance(self.n_neighbors, numbers.Integral) or isinstance(self.n_neighbors, bool):
            raise TypeError(
                f"n_neighbors does not take {type(self.n_neighbors)} value, enter integer value")
        if self.n_neighbors <= 0:
            raise ValueError(f"Expected n_neighbors > 0. Got {self.n_neighbors}")
        if not (self.weights in (None, "uniform", "distance") or callable(self.weights)):
            raise ValueError(
                "weights not recognized: should be 'uniform', 'distance', or a callable function")
        self.effective_metric_ = _effective_metric(self.metric, self.p, self.metric_params)
        self.effective_metric_params_ = dict(self.metric_params or {}) if self.effective_metric_ == "hamming" else {}
        if self.effective_metric_ == "hamming" and self.algorithm not in ("auto", "brute"):
            raise ValueError(f"Metric 'hamming' not valid. Use sorted(sklearn.neighbors.VALID_METRICS['{self.algorithm}']) "
                             "to get valid options. Metric can also be a callable function.")

    def fit(self, X, y):
        """Store the reference rows and targets in HBM and compute the independent
        (leave-self-out) prediction and score (REF _base.py:104-109)."""
        self._set_dataframe_index_in(X)
        return self._fit_arrays(X, y, affine=None)

    def _fit_arrays(self, X, y, affine, device=None, forest=None):
        self._check_params()
        X, y = validate_data(self, X, y, multi_output=True, order="C", dtype=np.float64,
                             ensure_all_finite=True, reset=True)
        self._y = y
        self._fit_X = X
        self.n_samples_fit_ = X.shape[0]
        self._fit_method = ("brute" if self.effective_metric_ == "hamming" else
                            _resolve_fit_method(self.algorithm, X.shape[0], X.shape[1], self.n_neighbors))
        if self.effective_metric_ == "hamming":
            w = self.effective_metric_params_.get("w")
            w = np.ones(X.shape[1]) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
            if w.size != X.shape[1]:
                raise ValueError(f"the Hamming weights have {w.size} entries for {X.shape[1]} columns")
            self._hamming_w = w
        self._affine = affine
        self._forest = forest  # forest image of a tree-node space (TreeNodeTransformer.forest_image), or None
        self._ref_tree = None  # tree_tie_policy("tree"): built on first use
        self._device = default_device() if device is None else device
        self._build_engine()
        self._set_independent_prediction_attributes(y)
        return self

    def _build_engine(self):
        y2 = self._y.reshape(-1, 1) if self._y.ndim == 1 else self._y
        self._engine = KNNEngine(self._fit_X, np.asarray(y2, dtype=np.float64), device=self._device,
                                 target_dtype=self._y.dtype)
        if getattr(self, "effective_metric_", "euclidean") == "hamming":
            self._engine.set_hamming_weights(self._hamming_w)
        if self._affine is not None:
            d_in, center, scale, proj = self._affine
            self._engine.set_affine(d_in, center, scale, proj)
        if getattr(self, "_forest", None) is not None:
            self._engine.set_forest(self._forest)

    @property
    def engine_(self) -> KNNEngine:
        """The device engine; rebuilt lazily after unpickling."""
        check_is_fitted(self, "_fit_X")
        if getattr(self, "_engine", None) is None:
            self._build_engine()
        return self._engine

    def __getstate__(self):
        state = dict(super().__getstate__())
        state["_engine"] = None  # device handles do not pickle; see engine_
        state["_ref_tree"] = None  # a cache, rebuilt on first use
        state["_replay_targets"] = None  # (table, attribute-only engine) of predict_neighbors_chunks(y=...): a device handle
        return state

    def _formula(self) -> str:
        if getattr(self, "effective_metric_", "euclidean") == "hamming":
            return "hamming"
        # both trees evaluate rdist = sum((x - y)^2) (SKL/metrics/_dist_metrics.pxd.tp); only brute expands the square
        return "expanded" if self._fit_method == "brute" else "direct"

    def _set_independent_prediction_attributes(self, y) -> None:
        """REF _base.py:37-40: predict and score with X=None."""
        self.independent_prediction_ = self.predict(None)
        self.independent_score_ = float(r2_score(y, self.independent_prediction_))

    # -- queries -------------------------------------------------------------------------
    def _validate_query(self, X):
        if is_torch_cuda_tensor(X):
            if X.ndim != 2 or X.shape[1] != self.n_features_in_:
                raise ValueError(
                    f"X has {X.shape[1] if X.ndim == 2 else '?'} features, but {type(self).__name__} "
                    f"is expecting {self.n_features_in_} features as input.")
            return X
        # feature count / names / dtype here; finiteness is tested by the kernels that read the rows
        # (check_finite), not by a second pass over them on the host
        return validate_data(self, X, reset=False, order="C", dtype=_QUERY_DTYPES, ensure_all_finite=False)

    def _resolve_k(self, n_neighbors):
        if n_neighbors is None:
            return self.n_neighbors
        if not isinstance(n_neighbors, numbers.Integral) or isinstance(n_neighbors, bool):
            raise TypeError(
                "n_neighbors does not take %s value, enter integer value" % type(n_neighbors))
        if n_neighbors <= 0:
            raise ValueError("Expected n_neighbors > 0. Got %d" % n_neighbors)
        return int(n_neighbors)

    def _numpy_ties(self) -> bool:
        """RFNN / GBNN under ``hamming_tie_policy("numpy")``: exactly tied rows as the reference's argpartition keeps them."""
        return (getattr(self, "effective_metric_", "euclidean") == "hamming"
                and _config.get_hamming_tie_policy() == "numpy")

    def _kneighbors_hamming_numpy_ties(self, X, k, use_deterministic_ordering, row_offset, n_self_rows, apply_affine=False):
        """Weighted-Hamming neighbours with the REFERENCE's choice among exactly tied rows.

        The device answers every row (tied rows lowest index first).  A second device search for one neighbour more, on the
        raw rows, shows which queries have an exact tie that the choice depends on (across the last slot; without the
        deterministic reorder, anywhere among the kept rows).  For those queries the device returns the full float64
        distance row (``sknnr_hamming_distances``: the matrix the reference's brute search materialises) and the
        selection is replayed line by line with this host's numpy: ``_kneighbors_reduce_func``
        (SKL/neighbors/_base.py:733-760: argpartition, argsort), the X=None self removal (SKL/neighbors/_base.py:936-963)
        and sknnr's reorder (REF src/sknnr/_base.py:166-175) -- reached in the reference from
        REF src/sknnr/_weighted_trees.py:53-59, :139-140 and pinned by REF tests/test_regressions.py:125-195.
        ``apply_affine``: ``X`` holds raw rows that the engine's forest map turns into node ids (the flagged rows' ids
        come from ``forest_apply``).
        """
        eng = self.engine_
        cuda_in = is_torch_cuda_tensor(X)
        X_host = X.cpu().numpy() if cuda_in else X
        self_query = X is None
        forest = bool(apply_affine) and not self_query
        kk = k + (1 if self_query else 0)
        n_fit = self.n_samples_fit_
        dist, idx = eng.kneighbors(X_host, k, exclude_self=self_query, deterministic=use_deterministic_ordering,
                                   decimals=self.DISTANCE_PRECISION_DECIMALS, formula="hamming", apply_affine=forest,
                                   row_offset=row_offset, n_self_rows=n_self_rows, check_finite=X is not None)
        nq = idx.shape[0]
        if nq:
            rows_q = self._fit_X[row_offset:row_offset + nq] if self_query else X_host
            probe = min(kk + 1, n_fit)
            pd, _ = eng.kneighbors(rows_q, probe, exclude_self=False, deterministic=False, formula="hamming",
                                   apply_affine=forest)
            if use_deterministic_ordering:  # only the SET of kept rows can differ: a tie across the last slot
                flagged = pd[:, kk - 1] == pd[:, kk] if probe > kk else np.zeros(nq, dtype=bool)
            else:  # the order among equal distances is argpartition's too
                flagged = (pd[:, :-1] == pd[:, 1:]).any(axis=1) if probe > 1 else np.zeros(nq, dtype=bool)
            rows = np.flatnonzero(flagged)
            step = max(1, (256 << 20) // (8 * n_fit))  # distance rows of at most ~256 MB at a time
            for a in range(0, rows.size, step):
                sel = rows[a:a + step]
                if forest:
                    full = eng.hamming_distances(eng.forest_apply(X_host[sel]))
                else:
                    full = eng.hamming_distances(None if self_query else X_host, sel + (row_offset if self_query else 0))
                dist[sel], idx[sel] = replay_reference_selection(full, kk, sel + row_offset, self_query,
                                                                  use_deterministic_ordering,
                                                                  self.DISTANCE_PRECISION_DECIMALS)
            self._last_numpy_tie_rows = int(rows.size)
        if cuda_in:
            import torch

            return torch.as_tensor(dist, device=X.device), torch.as_tensor(idx, device=X.device)
        return dist, idx

    def _tree_ties(self) -> bool:
        """Euclidean kd_tree / ball_tree under ``tree_tie_policy("tree")``: exactly tied rows as the reference's tree keeps them."""
        return (getattr(self, "effective_metric_", "euclidean") != "hamming"
                and self._fit_method in ("kd_tree", "ball_tree")
                and _config.get_tree_tie_policy() == "tree")

    def _reference_ties(self) -> bool:
        """Is one of the reference tie policies in force for this estimator (the choice among tied rows made on the host)?"""
        return self._numpy_ties() or self._tree_ties()

    def _check_reference_ties_supported(self, what):
        """Paths that cannot replay the reference's choice among tied rows refuse to run under a reference tie policy
        rather than answer with the device's lowest-index rule."""
        if self._numpy_ties():
            raise NotImplementedError(f"{what} does not support hamming_tie_policy('numpy'); use the default policy "
                                      "'lowest_index' or the estimator's own kneighbors / predict")
        if self._tree_ties():
            raise NotImplementedError(f"{what} does not support tree_tie_policy('tree'); use the default policy "
                                      "'lowest_index' or the estimator's own kneighbors / predict")

    def _reference_tree(self):
        """scikit-learn's tree over the fitted rows, as the reference's ``fit`` builds it (lazily, once per fit)."""
        if getattr(self, "_ref_tree", None) is None:
            self._ref_tree = build_reference_tree(self._fit_X, self._fit_method, self.leaf_size)
        return self._ref_tree

    def _kneighbors_tree_ties(self, X, k, use_deterministic_ordering, row_offset, n_self_rows, apply_affine):
        """Euclidean kd_tree / ball_tree neighbours with the REFERENCE's choice among exactly tied rows.

        The device answers every row (direct formula, the tree's arithmetic; tied rows lowest index first).  A second
        device search for one neighbour more shows which queries have an exact tie that the choice depends on (across
        the last slot; without the deterministic reorder, anywhere among the kept rows).  Those rows are queried in
        scikit-learn's tree over the fitted rows (:func:`replay_tree_selection`), in the space the device searched: the
        fitted rows, and for affine estimators the query rows mapped by the same device kernel as at fit time.
        """
        eng = self.engine_
        cuda_in = is_torch_cuda_tensor(X)
        X_host = X.cpu().numpy() if cuda_in else X
        self_query = X is None
        kk = k + (1 if self_query else 0)
        n_fit = self.n_samples_fit_
        formula = self._formula()
        dist, idx = eng.kneighbors(X_host, k, exclude_self=self_query, deterministic=use_deterministic_ordering,
                                   decimals=self.DISTANCE_PRECISION_DECIMALS, formula=formula,
                                   apply_affine=apply_affine and not self_query, row_offset=row_offset,
                                   n_self_rows=n_self_rows, check_finite=not self_query)
        nq = idx.shape[0]
        if nq:
            rows_q = self._fit_X[row_offset:row_offset + nq] if self_query else X_host
            probe = min(kk + 1, n_fit)
            pd, _ = eng.kneighbors(rows_q, probe, exclude_self=False, deterministic=False, formula=formula,
                                   apply_affine=apply_affine and not self_query)
            if use_deterministic_ordering:  # only the SET of kept rows can differ: a tie across the last slot
                flagged = pd[:, kk - 1] == pd[:, kk] if probe > kk else np.zeros(nq, dtype=bool)
            else:  # the order among equal distances is the tree's too
                flagged = (pd[:, :-1] == pd[:, 1:]).any(axis=1) if probe > 1 else np.zeros(nq, dtype=bool)
            rows = np.flatnonzero(flagged)
            if rows.size:
                rows_X = rows_q[rows]
                if apply_affine and not self_query:
                    d_in, center, scale, proj = self._affine
                    rows_X = _native.affine_transform_host(np.ascontiguousarray(rows_X, dtype=np.float64), center,
                                                           scale, proj, device=self._device)
                dist[rows], idx[rows] = replay_tree_selection(
                    self._fit_X, rows_X, kk, self._fit_method, self.leaf_size, rows + row_offset, self_query,
                    use_deterministic_ordering, self.DISTANCE_PRECISION_DECIMALS, tree=self._reference_tree())
            self._last_tree_tie_rows = int(rows.size)
        if cuda_in:
            import torch

            return torch.as_tensor(dist, device=X.device), torch.as_tensor(idx, device=X.device)
        return dist, idx

    def _kneighbors_reference_ties(self, X, k, use_deterministic_ordering, row_offset, n_self_rows, apply_affine):
        if self._numpy_ties():
            return self._kneighbors_hamming_numpy_ties(X, k, use_deterministic_ordering, row_offset, n_self_rows,
                                                       apply_affine)
        return self._kneighbors_tree_ties(X, k, use_deterministic_ordering, row_offset, n_self_rows, apply_affine)

    def _kneighbors_engine(self, X, k, *, apply_affine, use_deterministic_ordering, row_offset=0,
                           n_self_rows=None, return_distance=True, out=None, owner=None):
        if out is not None and self._reference_ties():
            self._check_reference_ties_supported("kneighbors into caller tensors (out=, ShardedKNN)")
        try:
            if self._reference_ties():
                return self._kneighbors_reference_ties(X, k, use_deterministic_ordering, row_offset, n_self_rows,
                                                       apply_affine)
            return self.engine_.kneighbors(
                X, k, exclude_self=X is None, deterministic=use_deterministic_ordering,
                decimals=self.DISTANCE_PRECISION_DECIMALS, formula=self._formula(),
                apply_affine=apply_affine, row_offset=row_offset, n_self_rows=n_self_rows,
                return_distance=return_distance, out=out, check_finite=X is not None)
        except _native.HipBackendError as err:
            _reraise(err, owner if owner is not None else self)

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True, return_dataframe_index=False,
                   use_deterministic_ordering=True):
        """Neighbours of ``X`` (or of every fitted row, itself excluded, when ``X`` is None);
        same contract as REF _base.py:111-182.  CUDA tensors in give CUDA tensors out."""
        check_is_fitted(self, "_fit_X")
        k = self._resolve_k(n_neighbors)
        if X is not None:
            X = self._validate_query(X)
        dist, idx = self._kneighbors_engine(X, k, apply_affine=False,
                                            use_deterministic_ordering=use_deterministic_ordering)
        return self._finish_kneighbors(dist, idx, return_distance, return_dataframe_index)

    def kneighbors_graph(self, X=None, n_neighbors=None, mode="connectivity"):
        """Sparse (n_queries, n_samples_fit) graph of the k neighbours of every row: ones, or the distances
        with ``mode="distance"`` -- the method the reference's estimator inherits from scikit-learn
        (SKL/neighbors/_base.py, KNeighborsMixin.kneighbors_graph), over this class's ``kneighbors``."""
        from scipy.sparse import csr_matrix

        check_is_fitted(self, "_fit_X")
        k = self._resolve_k(n_neighbors)
        if mode == "connectivity":
            ind = self.kneighbors(X, k, return_distance=False)
            ind = ind.cpu().numpy() if is_torch_cuda_tensor(ind) else ind
            data = np.ones(ind.shape[0] * k)
        elif mode == "distance":
            data, ind = self.kneighbors(X, k, return_distance=True)
            if is_torch_cuda_tensor(ind):
                data, ind = data.cpu().numpy(), ind.cpu().numpy()
            data = np.ravel(data)
        else:
            raise ValueError(
                f'Unsupported mode, must be one of "connectivity", or "distance" but got "{mode}" instead')
        n_queries = ind.shape[0]
        indptr = np.arange(0, n_queries * k + 1, k)
        return csr_matrix((data, ind.ravel(), indptr), shape=(n_queries, self.n_samples_fit_))

    def _finish_kneighbors(self, dist, idx, return_distance, return_dataframe_index):
        if return_dataframe_index:
            msg = "Dataframe indexes can only be returned when fitted with a dataframe."
            check_is_fitted(self, "dataframe_index_in_", msg=msg)
            table = self.dataframe_index_in_
            if table.dtype.kind in "iu" and table.dtype.itemsize <= 8 and table.dtype != np.uint64:
                idx = self.engine_.crosswalk(idx, table.astype(np.int64, copy=False)).reshape(idx.shape)
                if not is_torch_cuda_tensor(idx):
                    idx = idx.astype(table.dtype, copy=False)
            else:  # labels that are not 64-bit integers (strings, ...) cannot live on the device
                host_idx = idx.cpu().numpy() if is_torch_cuda_tensor(idx) else idx
                idx = table[host_idx]
        return (dist, idx) if return_distance else idx

    def _predict_engine(self, X, *, apply_affine, row_offset=0, n_self_rows=None, owner=None):
        weights = None if self.weights is None else self.weights
        try:
            if self._reference_ties():
                # the reference's predict() calls ITS kneighbors (deterministic ordering on): the same neighbours here,
                # then the reduction on the device (SKL/neighbors/_regression.py:224-268)
                dist, idx = self._kneighbors_reference_ties(X, self.n_neighbors, True, row_offset, n_self_rows,
                                                            apply_affine)
                cuda = is_torch_cuda_tensor(dist)
                if cuda:
                    dev = dist.device
                    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
                pred = self.engine_.predict_from_neighbors(dist, idx, "uniform" if weights is None else weights)
                if cuda:
                    import torch

                    pred = torch.as_tensor(pred, device=dev)
                return pred.reshape(-1) if self._y.ndim == 1 else pred
            pred = self.engine_.predict(
                X, self.n_neighbors, "uniform" if weights is None else weights, exclude_self=X is None,
                deterministic=True, decimals=self.DISTANCE_PRECISION_DECIMALS, formula=self._formula(),
                apply_affine=apply_affine, row_offset=row_offset, n_self_rows=n_self_rows,
                check_finite=X is not None)
        except _native.HipBackendError as err:
            _reraise(err, owner if owner is not None else self)
        if self._y.ndim == 1:
            pred = pred.reshape(-1)
        return pred

    def predict(self, X):
        """Weighted mean of the neighbours' targets (SKL/neighbors/_regression.py:224-268);
        ``X=None`` predicts every fitted row from its neighbours, itself excluded."""
        check_is_fitted(self, "_fit_X")
        if X is not None:
            X = self._validate_query(X)
        return self._predict_engine(X, apply_affine=False)

    def _n_targets(self) -> int:
        return 1 if self._y.ndim == 1 else self._y.shape[1]

    def _summarize_engine(self, X, stat, *, apply_affine, row_offset=0, n_self_rows=None, owner=None):
        """:meth:`_predict_engine` with the statistic codes ``stat`` in place of the mean; always float64.  ``stat`` may be
        an :class:`OutputPlan`: the result then is ``(n, n_out)``, 1-D only for a per-target plan of a 1-D ``y``."""
        weights = "uniform" if self.weights is None else self.weights
        plan = stat if isinstance(stat, OutputPlan) else None
        try:
            if self._reference_ties():
                # as _predict_engine: the policy's own neighbours, then the reduction on the device
                dist, idx = self._kneighbors_reference_ties(X, self.n_neighbors, True, row_offset, n_self_rows,
                                                            apply_affine)
                cuda = is_torch_cuda_tensor(dist)
                if cuda:
                    dev = dist.device
                    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
                if plan is not None:
                    out = self.engine_.summarize_plan_from_neighbors(dist, idx, weights, plan.arrays)
                else:
                    out = self.engine_.summarize_from_neighbors(dist, idx, weights, stat)
                if cuda:
                    import torch

                    out = torch.as_tensor(out, device=dev)
            else:
                out = (self.engine_.summarize if plan is None else self.engine_.summarize_plan)(
                    X, self.n_neighbors, weights, stat if plan is None else plan.arrays, exclude_self=X is None,
                    deterministic=True,
                    decimals=self.DISTANCE_PRECISION_DECIMALS, formula=self._formula(), apply_affine=apply_affine,
                    row_offset=row_offset, n_self_rows=n_self_rows, check_finite=X is not None)
        except _native.HipBackendError as err:
            _reraise(err, owner if owner is not None else self)
        if plan is not None and not plan.per_target:
            return out
        return out.reshape(-1) if self._y.ndim == 1 else out

    def _bootstrap_request(self, bootstrap, statistic, outputs, *, self_query=False, n_targets=None, stored=False, **others):
        """``(kw, plan, table)`` of a ``bootstrap=`` call, every refusal before any device work: ``others`` are the call's
        keywords that do not go with a bootstrap (name -> value, refused when set); ``n_targets``: the columns of a replay's
        own ``y``; ``stored``: the candidates are stored columns, so ``kw`` is settled by the first tile (None here)."""
        if not isinstance(bootstrap, Bootstrap):
            raise TypeError(f"bootstrap must be a sknnr_amd.Bootstrap, got {type(bootstrap).__name__}")
        if callable(self.weights) and not isinstance(self.weights, DistanceWeights):
            self._refuse_callable_weights("bootstrap is", "and a bootstrap weighs the copies each replicate takes on the device")
        self._check_stream_supported("bootstrap is")
        if statistic is not None:
            raise ValueError("statistic is not available with bootstrap=: name the planes in outputs, as (target, 'boot_se' | "
                             "'boot_mean' | 'boot_bias') pairs or 'boot_count'")
        for name, value in others.items():
            if name == "zonal" and value is not None:
                raise ValueError("zonal is not available with bootstrap=: a zonal sum of pixel standard errors is not the "
                                 "standard error of the zonal mean")
            if value is not None and value is not False:
                raise ValueError(f"{name} is not available with bootstrap=: the stream's reduction stage holds the bootstrap")
        plan = normalize_boot_outputs(outputs, self._n_targets() if n_targets is None else n_targets)
        n = self.n_samples_fit_
        table = bootstrap._bind(n)
        kw = None if stored else bootstrap.candidates(self.n_neighbors, n - (1 if self_query else 0))
        return kw, plan, table

    def _bootstrap_engine(self, X, bootstrap, request, *, apply_affine, owner=None):
        """One search at ``kw`` columns, then the bootstrap reduction on the device: float64 ``(n, n_out)``."""
        kw, plan, table = request
        dist, idx = self._kneighbors_engine(X, kw, apply_affine=apply_affine, use_deterministic_ordering=True, owner=owner)
        weights = "uniform" if self.weights is None else self.weights
        try:
            self.engine_.set_bootstrap(table)
            out, tally = self.engine_.bootstrap_from_neighbors(dist, idx, self.n_neighbors, weights, plan)
        except _native.HipBackendError as err:
            _reraise(err, owner if owner is not None else self)
        bootstrap._add(tally)
        return out

    def summarize(self, X=None, statistic=None, outputs=None, bootstrap=None):
        """A summary of each query's neighbours per target, reduced on the device from the neighbours ``kneighbors``
        finds (deterministic ordering on, as ``predict``); ``X=None`` summarises every fitted row's neighbours, itself
        excluded.  ``statistic``: one name, or one name per target -- ``"mean"`` (what ``predict`` gives, bit for bit), ``"mode"``
        (scikit-learn's ``KNeighborsClassifier.predict``: per distinct label the vote is the pairwise sum of the weights
        of the neighbours that carry it; the largest vote wins, the smaller label on equal votes; labels are the float64
        values in ``y``; all votes zero under a weights callable: NaN), ``"min"`` / ``"max"`` (of the neighbours' values,
        weights ignored), ``"nearest"`` (the first neighbour's value) and ``"std"`` (the weighted population standard
        deviation ``sqrt(sum((w * (v - m)) * (v - m)) / sum(w))`` around the float64 weighted mean ``m``, both sums
        numpy's pairwise sums over the k neighbours).  Weights are those of ``predict``: 1, ``1 / d`` (a row holding
        ``d == 0`` becomes its 0 / 1 mask) or the callable's; all arithmetic is float64.  Returns float64 ``(n, t)``, ``(n,)`` for a 1-D
        ``y``; numpy in gives numpy out, CUDA tensors in give CUDA tensors out.  Without ``statistic`` and ``outputs`` the
        statistic is ``"mean"``.

        A ``statistic`` entry may also be ``("quantile", q)``, ``0 <= q <= 1`` (the median is ``("quantile", 0.5)``): numpy's weighted
        ``inverted_cdf`` quantile of the neighbours' values, ``np.quantile(v, q, method="inverted_cdf", weights=w)`` --
        the values in stable ascending order, the weights' sequential running sum divided by its total, and the first
        value whose share is non-zero and at least ``q`` (NaN where the weights sum to 0).

        ``outputs`` (instead of ``statistic``): a sequence of ``(target, statistic)`` pairs -- ``target`` an integer
        column position that may repeat, ``statistic`` any of the above or ``"median"`` -- all reduced from ONE search, e.g.
        ``[(0, "mean"), (0, "std"), (0, ("quantile", .1)), (0, ("quantile", .9))]``.  Returns float64 ``(n, n_out)``,
        always 2-D; a plane with one of the six names equals that column of ``summarize(X, statistic=name)`` bit for bit.

        ``bootstrap`` (a :class:`sknnr_amd.Bootstrap`): the planes are bootstrap statistics over the fitted rows instead --
        ``outputs`` takes ``(target, "boot_se" | "boot_mean" | "boot_bias")`` pairs and ``"boot_count"``, by default
        ``boot_se`` of every target.  ONE search runs at ``bootstrap.n_candidates`` columns; every replicate's k nearest
        copies are taken from that list on the device (include/sknnr_hip.h, "Bootstrap").  Returns float64 ``(n, n_out)``."""
        check_is_fitted(self, "_fit_X")
        if bootstrap is not None:
            request = self._bootstrap_request(bootstrap, statistic, outputs, self_query=X is None)
            if X is not None:
                X = self._validate_query(X)
            return self._bootstrap_engine(X, bootstrap, request, apply_affine=False)
        if statistic is None and outputs is None:
            statistic = "mean"
        stat = resolve_statistic(statistic, outputs, self._n_targets())
        if X is not None:
            X = self._validate_query(X)
        return self._summarize_engine(X, stat, apply_affine=False)

    # -- leave-group-out: independent predictions that skip groups ------------------------------
    def _leave_out_masks(self, groups, buffer):
        """``(codes or None, (coords, radius) or None)`` of a leave-out call, refused before any device work.  Without a
        buffer ``groups`` is required, as it always was; with one it is optional."""
        check_is_fitted(self, "_fit_X")
        self._check_reference_ties_supported("independent_kneighbors with groups")
        if buffer is None:
            return normalize_groups(groups, self.n_samples_fit_), None
        buf = normalize_buffer(buffer, self.n_samples_fit_)
        return (None if groups is None else normalize_groups(groups, self.n_samples_fit_)), buf

    def _set_leave_out_masks(self, codes, buf):
        """Both masks on the engine: a mask the call does not name clears the one an earlier call left."""
        self.engine_.set_groups(codes)
        self.engine_.set_buffer(buf)

    def _independent_neighbors(self, groups, k, use_deterministic_ordering=True, buffer=None):
        """``(dist, idx)`` of :meth:`independent_kneighbors` as host arrays; everything is refused before device work."""
        codes, buf = self._leave_out_masks(groups, buffer)
        try:
            self._set_leave_out_masks(codes, buf)
            return self.engine_.kneighbors_grouped(k, deterministic=bool(use_deterministic_ordering),
                                                   decimals=self.DISTANCE_PRECISION_DECIMALS, formula=self._formula())
        except _native.HipBackendError as err:
            _reraise(err, self)

    def independent_kneighbors(self, groups=None, n_neighbors=None, return_distance=True, return_dataframe_index=False,
                               use_deterministic_ordering=True, *, buffer=None):
        """Leave-group-out neighbours: for every fitted row the ``n_neighbors`` nearest fitted rows of OTHER groups.

        ``groups``: a 1-D array-like of ``n_samples_fit_`` labels (integers, strings, a pandas Series) -- the plot of a
        re-measured row, the cluster of a subplot, the block of a spatial cross-validation.  For fitted row ``i`` the
        candidates are the fitted rows whose label differs from row ``i``'s, so never ``i`` itself.  Every pair has the
        float64 value ``kneighbors`` ranks it by; the answer is the ``k`` candidates smallest by (value, index), their
        distances, and -- with ``use_deterministic_ordering`` -- sknnr's reorder (REF _base.py:166-175).  Exact ties at the
        k-th value go to the lower index: the reference has no grouped search, so no choice of its is replayed, and the
        calls are refused under ``hamming_tie_policy("numpy")`` and ``tree_tie_policy("tree")``.  With every row in a
        group of its own this is ``kneighbors(X=None)`` wherever the k-th and (k+1)-th values differ.

        ``buffer=(coords, radius)``: buffered leave-out, with or without ``groups``.  ``coords`` holds the plot position
        of every fitted row -- an array-like or a pandas DataFrame of ``n_samples_fit_`` rows and 1 to 3 columns --
        and a fitted row ``r`` is no candidate of row ``i`` when ``((xi - xr)**2 + (yi - yr)**2) + (zi - zr)**2 <=
        radius * radius`` in float64 (a missing column counts as 0), so ``radius=0`` leaves out the co-located rows.
        Given together, either mask excludes.  :meth:`buffer_counts` tells how many rows a radius removes per row.

        ``ValueError`` for labels that are not 1-D, of another length, NaN, or all one group, for positions of another
        length, with no or more than 3 columns or not finite, for a radius that is negative, not finite or no scalar,
        and for ``n_neighbors`` above ``n_samples_fit_`` minus the largest number of rows excluded for one row (groups
        alone: the largest group).  Results are host arrays."""
        k = self._resolve_k(n_neighbors)
        dist, idx = self._independent_neighbors(groups, k, use_deterministic_ordering, buffer)
        return self._finish_kneighbors(dist, idx, return_distance, return_dataframe_index)

    def independent_predict(self, groups=None, *, buffer=None):
        """``predict`` of every fitted row from its :meth:`independent_kneighbors` (``n_neighbors`` of the estimator,
        deterministic ordering on) with the estimator's weights: what ``independent_prediction_`` is when every row is
        its own group, and the honest figure when it is not.  ``buffer``: as there."""
        dist, idx = self._independent_neighbors(groups, self.n_neighbors, buffer=buffer)
        pred = self.engine_.predict_from_neighbors(dist, idx, "uniform" if self.weights is None else self.weights)
        return pred.reshape(-1) if self._y.ndim == 1 else pred

    def independent_summarize(self, groups=None, statistic=None, outputs=None, *, buffer=None):
        """:meth:`summarize` of every fitted row over its :meth:`independent_kneighbors`; ``statistic`` / ``outputs`` as
        there, ``buffer`` as for :meth:`independent_kneighbors`."""
        check_is_fitted(self, "_fit_X")
        if statistic is None and outputs is None:
            statistic = "mean"
        stat = resolve_statistic(statistic, outputs, self._n_targets())
        dist, idx = self._independent_neighbors(groups, self.n_neighbors, buffer=buffer)
        weights = "uniform" if self.weights is None else self.weights
        if isinstance(stat, OutputPlan):
            out = self.engine_.summarize_plan_from_neighbors(dist, idx, weights, stat.arrays)
            if not stat.per_target:
                return out
        else:
            out = self.engine_.summarize_from_neighbors(dist, idx, weights, stat)
        return out.reshape(-1) if self._y.ndim == 1 else out

    def independent_score(self, groups=None, sample_weight=None, *, buffer=None):
        """R^2 of :meth:`independent_predict` against the fitted targets: ``independent_score_`` with groups, the plots
        inside a ``buffer``, or both left out."""
        return float(r2_score(self._y, self.independent_predict(groups, buffer=buffer), sample_weight=sample_weight))

    def buffer_counts(self, buffer, groups=None):
        """How many fitted rows ``buffer=(coords, radius)`` -- together with ``groups``, when given -- excludes for every
        fitted row, the row itself included: int64 ``(n_samples_fit_,)``, counted on the device from the positions and
        the codes alone.  Row ``i`` has ``n_samples_fit_ - counts[i]`` candidates in :meth:`independent_kneighbors`."""
        if buffer is None:
            raise ValueError("buffer_counts needs buffer=(coords, radius)")
        codes, buf = self._leave_out_masks(groups, buffer)
        try:
            self._set_leave_out_masks(codes, buf)
            return self.engine_.buffer_counts()
        except _native.HipBackendError as err:
            _reraise(err, self)

    # -- neighbour usage: which fitted rows made the map ------------------------------------------
    def _usage_from_neighbors(self, dist, idx):
        counts, max_dist = self.engine_.tally_from_neighbors(dist, idx)
        usage = NeighborUsage()
        return usage._add(counts, max_dist, getattr(self, "dataframe_index_in_", None))

    def neighbor_usage(self, X=None, n_neighbors=None):
        """The :class:`sknnr_amd.NeighborUsage` of ``kneighbors(X, n_neighbors)`` (deterministic ordering): per fitted
        row and rank the query rows it served, and the largest distance among them, tallied on the device from the
        neighbours the search returns.  ``X=None``: of every fitted row's neighbours, itself excluded.  For a raster,
        pass ``usage=`` to :meth:`kneighbors_chunks` / :meth:`predict_chunks` instead: the tally then costs no transfer."""
        dist, idx = self.kneighbors(X, n_neighbors=n_neighbors)
        try:
            return self._usage_from_neighbors(dist, idx)
        except _native.HipBackendError as err:
            _reraise(err, self)

    def independent_neighbor_usage(self, groups=None, n_neighbors=None, *, buffer=None):
        """The :class:`sknnr_amd.NeighborUsage` of :meth:`independent_kneighbors` ``(groups, n_neighbors, buffer=buffer)``:
        which fitted rows the leave-out predictions lean on."""
        k = self._resolve_k(n_neighbors)
        dist, idx = self._independent_neighbors(groups, k, buffer=buffer)
        try:
            return self._usage_from_neighbors(dist, idx)
        except _native.HipBackendError as err:
            _reraise(err, self)

    # -- distance domain: where the map extrapolates -------------------------------------------------
    def distance_domain(self, groups=None, *, buffer=None, rank=1, p=None, threshold=None):
        """A :class:`sknnr_amd.DistanceDomain` of this estimator's reference plots: its table is the sorted distance of
        every fitted row to its ``rank``-th :meth:`independent_kneighbors` neighbour -- itself (with neither ``groups``
        nor ``buffer``: every row a group of its own), its group or the plots inside ``buffer`` left out -- in the
        estimator's own metric.  ``p`` (``0 < p < 1``): the threshold is the
        ``1 - p`` quantile of the table (``np.quantile``), so about a share ``p`` of the plots lie beyond it, as
        yaImpute's "notably distant" targets are defined; ``threshold``: a distance of the caller's instead.  The two
        are mutually exclusive; with neither the object has no threshold and counts nothing as beyond."""
        if isinstance(rank, bool) or int(rank) != rank or int(rank) < 1:
            raise ValueError(f"rank must be an integer >= 1, got {rank!r}")
        if p is not None and threshold is not None:
            raise ValueError("p and threshold are mutually exclusive: p derives the threshold from the table")
        if p is not None and not 0.0 < float(p) < 1.0:
            raise ValueError(f"p must lie inside (0, 1), got {p!r}")
        rank = int(rank)
        check_is_fitted(self, "_fit_X")
        if groups is None and buffer is None:  # (self left out: every row a group of its own)
            groups = np.arange(self.n_samples_fit_)
        dist, _ = self.independent_kneighbors(groups, n_neighbors=rank, buffer=buffer)
        table = np.sort(np.asarray(dist, dtype=np.float64)[:, rank - 1])
        if p is not None:
            threshold = float(np.quantile(table, 1.0 - float(p)))
        return DistanceDomain(table, threshold=threshold, rank=rank)

    def _domain_scores(self, domain, dist):
        """The codes of neighbours already found, their tallies added to ``domain``."""
        if not isinstance(domain, DistanceDomain):
            raise TypeError(f"domain must be a sknnr_amd.DistanceDomain, got {type(domain).__name__}")
        k = dist.shape[1]
        if domain.rank > k:
            raise ValueError(f"domain.rank={domain.rank} is above n_neighbors={k}")
        try:
            codes, acc = self.engine_.domain_from_neighbors(dist, domain.table, domain.rank, domain.threshold)
        except _native.HipBackendError as err:
            _reraise(err, self)
        domain._add(acc)
        return codes

    def domain_scores(self, domain, X=None, n_neighbors=None):
        """The uint8 distance-domain codes of ``kneighbors(X, n_neighbors)`` (deterministic ordering) within ``domain``
        (a :class:`sknnr_amd.DistanceDomain`), computed on the device; the tallies are added to ``domain``.  ``X=None``:
        of every fitted row's neighbours, itself excluded.  For a raster, pass ``domain=`` to :meth:`kneighbors_chunks`
        / :meth:`predict_chunks` instead: the codes then cost one byte per pixel of transfer and no second pass."""
        if not isinstance(domain, DistanceDomain):
            raise TypeError(f"domain must be a sknnr_amd.DistanceDomain, got {type(domain).__name__}")
        if domain.rank > self._resolve_k(n_neighbors):
            raise ValueError(f"domain.rank={domain.rank} is above n_neighbors={self._resolve_k(n_neighbors)}")
        dist, _ = self.kneighbors(X, n_neighbors=n_neighbors)
        return self._domain_scores(domain, dist)

    # -- streamed tiles (raster ingestion; REF docs/pages/usage.md:101-128) --------------------
    def _check_stream_supported(self, feature):
        """The nodata mask, the band-first transposes and the typed conversions (``feature``: "nodata is", "layout='bands'
        is", "typed outputs are") run on the device, inside a native stream; the paths that answer tile by tile on the
        host refuse them."""
        for policy, on in (("hamming_tie_policy('numpy')", self._numpy_ties()), ("tree_tie_policy('tree')", self._tree_ties())):
            if on:
                raise NotImplementedError(f"{feature} not supported under {policy}: tied rows are chosen on the host, "
                                          "tile by tile; use the default policy 'lowest_index'")

    @staticmethod
    def _refuse_callable_weights(feature, how="tile by tile"):
        raise NotImplementedError(f"{feature} not supported with callable weights: the callable runs on the host between "
                                  f"the search and the reduction, {how}; use 'uniform', 'distance' or a law of "
                                  "sknnr_amd.weights (evaluated on the device)")

    def _stream_tiles(self, tiles, validate, k, *, products, apply_affine, weights, return_distance,
                      use_deterministic_ordering, out, owner, nodata=None, fill_index=-1, bands=False, output=None,
                      statistic=None, id_table=None, fill_id=-1, neighbors=False):
        """Push host tiles through one native query stream.  Returns (dist, idx, pred) arrays over all
        pushed rows (pieces of ``out`` when given, else concatenated).  ``nodata`` (float64, one value per column of the
        validated tiles): rows holding one are masked on the device and get ``fill_index`` / NaN.

        ``bands``: the tiles are band-first -- ``validate`` gives ``(bands, n)`` (:func:`normalize_band_tile`), the outputs
        are ``(k, N)`` / ``(t, N)``, pixels along axis 1, and tile ``i`` lands in columns ``[row, row + n_i)``; the
        ``out`` arrays must then share one ``N``, the stride between their planes.

        ``output``: keyword arguments of :meth:`sknnr_amd._native.QueryStream.set_output` -- the results are narrowed on
        the device and the arrays (``out`` included) have those element types.

        ``statistic``: int32 codes (:func:`normalize_statistic`), one per target -- the predictions are those summaries
        of the neighbours instead of the mean.

        ``id_table`` (:meth:`_device_id_table`): int64 dataframe ids, one per reference row -- the indices leave the
        device as ``id_table[idx]``, and with a mask ``fill_index`` must be -1: those rows get ``fill_id``.

        ``neighbors`` (with ``weights``): the indices (and, with ``return_distance``, the distances) the predictions are
        reduced from are delivered beside them, from the same stream; an output without an array in ``out`` is
        collected and concatenated.

        ``products`` (a :class:`sknnr_amd._products.StreamProducts` the caller has checked): the stream computes
        the call's side products -- usage, zonal statistics, the distance domain -- on the device beside its results and
        the call adds them to the user's objects once it has come through whole; nothing else about the call changes.
        With a bootstrap among them ``k`` is the number of candidates searched, the stream's reduction stage is the
        bootstrap with replicates of ``n_neighbors`` copies, and the prediction lane holds the request's planes.  Every
        product refuses the host-side tie policies, so the tile-by-tile branch below never sees one."""
        if output:
            self._check_stream_supported("typed outputs are")
        eng = self.engine_
        want_pred = weights is not None
        plan = statistic if isinstance(statistic, OutputPlan) else None  # (the prediction lane then has n_out columns)
        t_cols = eng.t if plan is None else plan.n_out
        if products.bootstrap is not None:
            t_cols = len(products.request[1][0])
        output = {key: v for key, v in (output or {}).items() if v is not None}
        idx_dt = np.dtype(output.get("index_dtype", np.int64))
        dist_dt = np.dtype(output.get("distance_dtype", np.float64))
        pred_dt = np.dtype(output.get("pred_dtype", np.float64))
        if nodata is not None:
            self._check_stream_supported("nodata is")
        if bands:
            self._check_stream_supported("layout='bands' is")
            widths = {a.shape[1] for a in (out or ()) if a is not None and a.ndim == 2 and a.shape[0] > 1}
            if len(widths) > 1:
                raise ValueError(f"out arrays must share one number of columns (the stride between planes), got {sorted(widths)}")
        if self._reference_ties():
            # the reference's choice among tied rows is made on the host, per call: tile by tile, positions carried
            # (no side product gets here: each of them has refused these policies)
            parts, row = [], 0
            for tile in tiles:
                if _empty_row_tile(tile):
                    continue
                tile = validate(tile)
                if tile.shape[0] == 0:
                    continue
                if want_pred and statistic is not None:
                    parts.append((None, None, np.reshape(self._summarize_engine(tile, statistic, apply_affine=apply_affine,
                                                                                 row_offset=row, owner=owner),
                                                         (tile.shape[0], -1))))
                elif want_pred:
                    parts.append((None, None, np.reshape(self._predict_engine(tile, apply_affine=apply_affine, row_offset=row,
                                                                               owner=owner), (tile.shape[0], -1))))
                else:
                    d_, i_ = self._kneighbors_engine(tile, k, apply_affine=apply_affine, row_offset=row,
                                                     use_deterministic_ordering=use_deterministic_ordering, owner=owner)
                    parts.append((d_, i_, None))
                row += tile.shape[0]
            cat = lambda j, cols, dt: (np.concatenate([p_[j] for p_ in parts]) if parts  # noqa: E731
                                       else np.empty((0, cols), dtype=dt))
            res = (cat(0, k, np.float64) if return_distance and not want_pred else None,
                   None if want_pred else cat(1, k, np.int64), cat(2, t_cols, np.float64) if want_pred else None)
            if out is not None:
                for dst, src in zip(out, res):
                    if dst is not None and src is not None:
                        dst[:row] = src
                res = tuple(None if (dst is None or src is None) else dst[:row] for dst, src in zip(out, res))
            return res
        o_dist, o_idx, o_pred = out if out is not None else (None, None, None)
        pieces = []
        row = 0
        stream = None
        stream_dtype = None
        try:
            for tile in tiles:
                if is_torch_cuda_tensor(tile):
                    raise TypeError("streamed tiles are host arrays (they travel through the pinned "
                                    "PCIe pipeline); pass CUDA tensors to kneighbors() / predict()")
                products.next_tile()
                if not bands and _empty_row_tile(tile):
                    continue
                if bands:  # (``tile``: the list of 1-D bands; ``first`` stands for its element type)
                    tile, n = validate(tile)
                    first, n_cols = tile[0], len(tile)
                else:
                    tile = first = validate(tile)
                    n, n_cols = tile.shape
                if n == 0:
                    continue
                if stream is None:
                    # the element type of the first tile is the stream's (narrow rasters travel at their own width)
                    code = eng.query_dtype_code(first, self._formula(), apply_affine)
                    stream_dtype = first.dtype if code else np.dtype(np.float64)
                    if nodata is not None:  # (a NaN entry needs rows that can hold NaN)
                        nodata = normalize_nodata(nodata, n_cols, stream_dtype)
                    stream = eng.open_stream(k, weights=weights, want_dist=return_distance,
                                             deterministic=use_deterministic_ordering,
                                             decimals=self.DISTANCE_PRECISION_DECIMALS, formula=self._formula(),
                                             apply_affine=apply_affine, check_finite=True, query_dtype=code,
                                             nodata=nodata, fill_index=fill_index, output=output,
                                             **(dict(statistic=statistic) if plan is None else dict(plan=plan.arrays)),
                                             **({} if id_table is None else dict(id_table=id_table, fill_id=fill_id)),
                                             **products.open_keywords(eng, self.n_neighbors))
                if first.dtype != stream_dtype:
                    if stream_dtype != np.float64:
                        raise ValueError(f"the tiles of one streamed call must share an element type: got {first.dtype} "
                                         f"after {stream_dtype}")
                    tile = ([np.ascontiguousarray(b, dtype=np.float64) for b in tile] if bands
                            else np.ascontiguousarray(tile, dtype=np.float64))
                products.feed(stream, row, n)
                window = lambda arr, cols, dtype: _out_window(arr, row, n, cols, dtype, bands, "out arrays")  # noqa: E731
                got = (stream.push_planes if bands else stream.push)(
                    tile, out_idx=window(o_idx, k, idx_dt),
                    out_dist=window(o_dist, k, dist_dt) if return_distance else None,
                    out_pred=window(o_pred, t_cols, pred_dt) if want_pred else None, need_idx=neighbors or not want_pred)
                if out is None or neighbors:
                    pieces.append(got)
                row += n
            products.end_of_tiles()
            if stream is not None:
                done, stream = stream, None
                try:
                    products.collect(done)
                finally:
                    done.close()
            products.commit(self, k)
        except _native.HipBackendError as err:
            _reraise(err, owner if owner is not None else self)
        finally:
            if stream is not None:  # an error on the way: free the native stream without masking it
                try:
                    stream.close()
                except _native.HipBackendError:
                    pass
        trim = lambda a: None if a is None else (a[:, :row] if bands else a[:row])  # noqa: E731
        if out is not None and not neighbors:
            return trim(o_dist) if return_distance else None, trim(o_idx), trim(o_pred) if want_pred else None
        cat = lambda i, cols, dt: (np.concatenate([p[i] for p in pieces], axis=1 if bands else 0) if pieces  # noqa: E731
                                   else np.empty((cols, 0) if bands else (0, cols), dtype=dt))
        if neighbors:  # (each output from its array in ``out`` where there is one, else collected)
            pick = lambda o_, i, cols, dt: trim(o_) if o_ is not None else cat(i, cols, dt)  # noqa: E731
            return (pick(o_dist, 1, k, dist_dt) if return_distance else None, pick(o_idx, 0, k, idx_dt),
                    pick(o_pred, 2, t_cols, pred_dt))
        return (cat(1, k, dist_dt) if return_distance else None,
                None if want_pred else cat(0, k, idx_dt),
                cat(2, t_cols, pred_dt) if want_pred else None)

    def _neighbor_output(self, index_dtype, distance_dtype, return_distance, return_dataframe_index, fill_index, masked):
        """The ``output`` arguments of a typed neighbour stream, or None; every refusal comes before any device work."""
        idt = _narrow_dtype(index_dtype, np.int64, (np.dtype(np.int32),), "index_dtype")
        ddt = _narrow_dtype(distance_dtype, np.float64, (np.dtype(np.float32),), "distance_dtype")
        if not return_distance:
            ddt = None
        if idt is not None:
            if masked and not _representable(fill_index, idt):
                raise ValueError(f"fill_index={fill_index!r} is not representable in index_dtype={idt}")
            if return_dataframe_index:
                msg = "Dataframe indexes can only be returned when fitted with a dataframe."
                check_is_fitted(self, "dataframe_index_in_", msg=msg)
                table = np.asarray(self.dataframe_index_in_)
                info = np.iinfo(idt)
                if table.dtype.kind not in "iu" or (table.size and (table.min() < info.min or table.max() > info.max)):
                    raise ValueError(f"index_dtype={idt} with return_dataframe_index=True needs integer dataframe ids "
                                     f"inside [{info.min}, {info.max}]")
        out = dict(index_dtype=idt, distance_dtype=ddt)
        return out if idt is not None or ddt is not None else None

    def _device_id_table(self, return_dataframe_index):
        """The dataframe ids as the int64 table a stream looks its indices up in on the device, or None: row indices
        were asked for, the labels are no integers of at most 64 bits (the rule of :meth:`_finish_kneighbors`; those are
        looked up on the host), or a reference tie policy answers tile by tile on the host."""
        if not return_dataframe_index:
            return None
        msg = "Dataframe indexes can only be returned when fitted with a dataframe."
        check_is_fitted(self, "dataframe_index_in_", msg=msg)
        table = np.asarray(self.dataframe_index_in_)
        if table.dtype.kind not in "iu" or table.dtype.itemsize > 8 or table.dtype == np.uint64 or self._reference_ties():
            return None
        return np.ascontiguousarray(table.astype(np.int64, copy=False))

    def kneighbors_chunks(self, tiles, n_neighbors=None, return_distance=True, return_dataframe_index=False,
                          use_deterministic_ordering=True, out=None, nodata=None, fill_index=-1, layout="rows",
                          index_dtype=None, distance_dtype=None, usage=None, domain=None, domain_out=None):
        """``kneighbors`` over an iterable of host tiles ``(n_i, n_features)`` -- windows of a raster,
        slices of a ``numpy.memmap`` -- as ONE logical call: the copy-in / kernels / copy-out pipeline
        stays full across tiles and row positions count over all tiles, so the result equals
        ``kneighbors(np.concatenate(tiles))`` bit for bit.  ``out=(dist, idx)`` (``dist`` may be None):
        preallocated arrays (e.g. memmaps) that receive the rows in order.

        ``nodata``: a scalar, or one value per input column (NaN: "NaN in that column").  Rows in which any column
        equals its nodata value are masked on the device: they cost no search, are not tested for finiteness and get
        ``fill_index`` (as index or dataframe id) and NaN distances; the other rows get exactly what
        ``kneighbors(X[valid])`` returns, row positions counting valid rows only.

        ``layout="bands"``: every tile is band-first, as raster readers deliver a window -- an array ``(bands, ...)`` of
        any trailing shape, or a sequence of ``bands`` arrays -- and the results are band-first too: ``(k, N)`` arrays
        (``out``: C-contiguous ``(k, N_total)``), concatenated along the pixel axis.  Both transpositions run on the
        device; ``[j, p]`` equals ``[p, j]`` of the row call on the transposed tiles, bit for bit.

        ``index_dtype=np.int32`` / ``distance_dtype=np.float32``: the results are narrowed on the device (plain
        narrowing; the C cast, round to nearest even) and only the narrow bytes cross PCIe; ``out`` arrays then have those
        types.  ``fill_index`` and, with ``return_dataframe_index``, every dataframe id must fit int32.

        ``return_dataframe_index=True`` with integer dataframe ids (at most 64 bits, not uint64): the ids are looked up
        on the device, inside the conversion every tile's indices leave through, so ``out`` receives ids (int64, or
        int32 with ``index_dtype``) and the host never walks the output again; other labels (strings, ...) and the
        host-side tie policies are looked up on the host afterwards, as before.

        ``usage`` (a :class:`sknnr_amd.NeighborUsage`): every tile's neighbours are tallied on the device -- per fitted
        row and rank the pixels it served, and the largest distance it was imputed over; masked pixels contribute
        nothing -- and the call adds the result to the object.  Everything the call returns or writes is bit-identical to
        the call without it; no index crosses PCIe for the tally.  The tally is over row positions whatever
        ``return_dataframe_index`` says.  Refused under the host-side tie policies.

        ``domain`` (a :class:`sknnr_amd.DistanceDomain`): every pixel's distance to its ``domain.rank``-th neighbour is
        placed within the domain's table on the device -- the percentage of table entries strictly below it, 0 .. 100,
        100 exactly when it is above them all, 255 for a masked pixel -- and the call adds the histogram of those codes
        and the count of pixels beyond the threshold to the object.  ``domain_out``: a preallocated C-contiguous uint8
        ``(N_total,)`` array (e.g. a memmap) that receives the codes tile by tile, in pixel order in either layout; one
        byte per pixel crosses PCIe for it, and nothing without it.  Everything the call returns or writes is
        bit-identical to the call without the keywords.  Refused under the host-side tie policies; ``domain.rank`` above
        ``n_neighbors`` and a ``domain_out`` of another type, too short or without ``domain`` are ``ValueError``."""
        bands = _check_layout(layout)
        check_is_fitted(self, "_fit_X")
        k = self._resolve_k(n_neighbors)
        products = StreamProducts(usage=usage, domain=domain, domain_out=domain_out)
        products.check_domain(self, k)
        if nodata is not None:
            nodata = normalize_nodata(nodata, self.n_features_in_, np.float64)
        output = self._neighbor_output(index_dtype, distance_dtype, return_distance, return_dataframe_index, fill_index,
                                       nodata is not None)
        o = None if out is None else (out[0], out[1], None)
        validate = self._validate_query
        if bands:
            validate = lambda t: normalize_band_tile(t, self.n_features_in_, estimator=type(self).__name__)  # noqa: E731
        # (dataframe ids: masked rows travel as -1, which no row index equals, and take fill_index in the crosswalk)
        table = self._device_id_table(return_dataframe_index)
        products.check_usage(self, k)
        dist, idx, _ = self._stream_tiles(tiles, validate, k, products=products, apply_affine=False, weights=None,
                                          return_distance=return_distance,
                                          use_deterministic_ordering=use_deterministic_ordering, out=o, owner=None,
                                          nodata=nodata, fill_index=-1 if return_dataframe_index else fill_index,
                                          bands=bands, output=output, id_table=table, fill_id=fill_index)
        return self._finish_chunks(dist, idx, return_distance, return_dataframe_index,
                                   fill_index=None if nodata is None else fill_index, on_device=table is not None)

    def _finish_chunks(self, dist, idx, return_distance, return_dataframe_index, fill_index=None, on_device=False):
        """``fill_index`` (a masked call): rows whose index is -1 are nodata rows and get it instead of a table entry.
        ``on_device``: the stream looked the ids up already (:meth:`_device_id_table`), fill included; what is left is
        the one ``astype`` of a table that is not int64, as in :meth:`_finish_kneighbors`."""
        if return_dataframe_index:
            msg = "Dataframe indexes can only be returned when fitted with a dataframe."
            check_is_fitted(self, "dataframe_index_in_", msg=msg)
            table = self.dataframe_index_in_
            if on_device:
                if idx.dtype == np.int64:  # (an int32 output keeps its type, as the in-place host lookup did)
                    idx = idx.astype(table.dtype, copy=False)
            elif fill_index is not None:
                if table.dtype == np.int64 or idx.dtype == np.int32:  # (int32: the ids were checked to fit)
                    step = 1 << 22
                    for a in range(0, idx.shape[0], step):
                        blk = idx[a:a + step]
                        masked = blk < 0
                        idx[a:a + step] = np.where(masked, fill_index, table[np.where(masked, 0, blk)])
                else:
                    masked = idx < 0
                    idx = table[np.where(masked, 0, idx)]
                    idx[masked] = fill_index
            elif table.dtype == np.int64 or idx.dtype == np.int32:
                step = 1 << 22  # in place, block by block: idx may be a memmap larger than memory
                for a in range(0, idx.shape[0], step):
                    idx[a:a + step] = table[idx[a:a + step]]
            else:
                idx = table[idx]
        return (dist, idx) if return_distance else idx

    @staticmethod
    def _neighbor_request(return_neighbors, return_distance, return_dataframe_index, neighbors_out, fill_index,
                          index_dtype, distance_dtype):
        """The neighbour keywords of ``predict_chunks`` as one dict, or None without ``return_neighbors``; any of them
        without it is refused, before any device work."""
        if return_neighbors:
            if neighbors_out is not None and len(neighbors_out) != 2:
                raise ValueError("neighbors_out must be (dist, idx); dist may be None")
            return dict(return_distance=bool(return_distance), return_dataframe_index=bool(return_dataframe_index),
                        neighbors_out=neighbors_out, fill_index=fill_index, index_dtype=index_dtype,
                        distance_dtype=distance_dtype)
        for name, given in (("neighbors_out", neighbors_out is not None), ("return_distance", return_distance is not True),
                            ("return_dataframe_index", return_dataframe_index is not False),
                            ("fill_index", fill_index != -1), ("index_dtype", index_dtype is not None),
                            ("distance_dtype", distance_dtype is not None)):
            if given:
                raise ValueError(f"{name} needs return_neighbors=True: predictions alone have no neighbour outputs")
        return None

    def predict_chunks(self, tiles, out=None, nodata=None, layout="rows", out_dtype=None, scale=None, offset=None,
                       out_nodata=None, statistic=None, return_neighbors=False, return_distance=True,
                       return_dataframe_index=False, neighbors_out=None, fill_index=-1, index_dtype=None,
                       distance_dtype=None, outputs=None, usage=None, zones=None, zonal=None, domain=None, domain_out=None,
                       beyond="keep", bootstrap=None):
        """``predict`` over an iterable of host tiles as one streamed call; ``out``: preallocated
        ``(n_rows, n_targets)`` float64 array (e.g. a memmap; float32 results are held exactly).  ``nodata`` as in
        :meth:`kneighbors_chunks`: masked rows are predicted NaN.  ``layout="bands"``: band-first tiles as in
        :meth:`kneighbors_chunks`, and ``(n_targets, N)`` predictions (``out``: C-contiguous ``(n_targets, N_total)``, e.g.
        ``raster.reshape(t, H * W)`` of a memmapped output raster); ``(N,)`` for a 1-D ``y`` as ever.

        ``out_dtype`` (float32, int16, uint16, uint8 or int32): the type the raster is stored in.  The device converts
        the predictions and only the narrow bytes cross PCIe; ``out`` must have that dtype.  ``scale`` / ``offset``
        (scalars or one value per target): the stored value is ``rint(pred * scale + offset)`` -- two float64 roundings,
        half to even -- clamped to the type's range (float32: ``pred * scale + offset`` rounded to float32, no ``rint``).
        Masked rows get ``out_nodata``, which must be representable in ``out_dtype``, is required for an integer type
        with ``nodata`` and defaults to NaN for float32.  The clamp does not avoid the nodata value.

        ``statistic`` (one name, or one name per target): what is reduced from each pixel's neighbours on the device in
        place of the mean, as :meth:`summarize` defines it -- ``"mean"`` (what ``predict`` gives, bit for bit), ``"mode"``
        (scikit-learn's ``KNeighborsClassifier.predict``: per distinct label the vote is the pairwise sum of the weights
        of the neighbours that carry it; the largest vote wins, the smaller label on equal votes; labels are the float64
        values in ``y``; all votes zero under a weights callable: NaN), ``"min"`` / ``"max"`` (of the neighbours' values,
        weights ignored), ``"nearest"`` (the first neighbour's value) and ``"std"`` (the weighted population standard
        deviation ``sqrt(sum((w * (v - m)) * (v - m)) / sum(w))`` around the float64 weighted mean ``m``, both sums
        numpy's pairwise sums over the k neighbours).  Weights are those of ``predict``: 1, ``1 / d`` (a row holding
        ``d == 0`` becomes its 0 / 1 mask) or the callable's; all arithmetic is float64.  The result equals ``summarize(np.concatenate(tiles),
        statistic)`` bit for bit (float64 unless ``out_dtype`` says otherwise) and is written where the prediction is, so
        ``nodata``, ``layout``, ``out`` and the typed outputs apply unchanged; e.g. ``statistic=["mean", "mean", "mode"]``
        maps two continuous attributes and a class code in one call.  An entry may also be ``("quantile", q)``
        (:meth:`summarize`).

        ``outputs`` (instead of ``statistic``): a sequence of ``(target, statistic)`` pairs as in :meth:`summarize` -- the
        ``n_out`` planes are all reduced inside the one streamed search, e.g. an attribute's mean, q10 and q90 and a class
        mode.  The result is ``(N, n_out)``, ``(n_out, N)`` with ``layout="bands"``, always 2-D, and equals
        ``summarize(np.concatenate(tiles), outputs=outputs)`` bit for bit; ``out``, ``out_dtype``, ``scale`` / ``offset``
        (scalars or one value per output plane), ``out_nodata``, ``nodata`` and ``return_neighbors`` apply unchanged.

        ``return_neighbors=True``: the neighbours the predictions are reduced from (``n_neighbors`` of them,
        deterministic ordering) are delivered beside them from the SAME search -- the call returns ``(pred, dist, idx)``,
        or ``(pred, idx)`` with ``return_distance=False`` -- so a plot-id raster, a distance raster and the attribute
        rasters cost one pass, not ``kneighbors_chunks`` and then ``predict_chunks``.  ``return_dataframe_index``,
        ``fill_index``, ``index_dtype`` and ``distance_dtype`` are those of :meth:`kneighbors_chunks`, and ``dist`` /
        ``idx`` equal its results with the same ``nodata`` and ``layout`` bit for bit; ``neighbors_out=(dist, idx)``
        (``dist`` may be None) are preallocated arrays under the rules of its ``out`` -- with ``layout="bands"`` they
        share ``N`` with ``out``, and the arrays come all or none: the planes of one tile leave with one stride.  An
        output without an array is collected tile by tile and returned concatenated.  ``pred`` is what the call returns without ``return_neighbors``.  Callable weights
        and the host-side tie policies are refused; so is any of these keywords without ``return_neighbors=True``.

        An estimator whose ``weights`` is a law of :mod:`sknnr_amd.weights` (``InverseDistance``, ...) is not a
        "callable" in the sense above: the device evaluates the law, and every keyword here applies as for
        ``weights="distance"``.  A compact law (``Triangular``, ``Epanechnikov``) predicts NaN where all k neighbours lie
        at or beyond its bandwidth, so an integer ``out_dtype`` then needs ``out_nodata`` even without ``nodata``.

        ``usage`` (a :class:`sknnr_amd.NeighborUsage`): as in :meth:`kneighbors_chunks` -- the neighbours the predictions
        are reduced from are tallied on the device, with or without ``return_neighbors``, and the predictions are
        bit-identical to the call without it.  Refused with callable weights and under the host-side tie policies.

        ``zones`` / ``zonal`` (together): ``zonal`` is a :class:`sknnr_amd.ZonalStats` and ``zones`` an iterable consumed
        in lockstep with ``tiles`` -- per tile the integer zone codes of its pixels, ``(n,)``, or ``(h, w)`` for
        ``layout="bands"``; any integer dtype whose values fit int32 (a skipped empty tile consumes its entry; one
        iterable ending before the other is a ``ValueError``).  Every tile's final values are tallied by zone on the
        device -- count, sum, sum of squares, min and max per zone and output plane, and the class counts of the planes
        ``zonal`` names as classes -- over the STORED integers of the typed output, so an integer ``out_dtype`` is
        required (a float atomic sum would depend on arrival order); nodata pixels and zone codes outside
        ``[0, n_zones)`` contribute nothing.  The call adds the result to ``zonal`` and returns and writes exactly what
        it does without it; it works with ``usage``, ``nodata``, ``outputs``, ``statistic`` and ``return_neighbors``.
        Refused with callable weights and under the host-side tie policies.

        ``domain`` / ``domain_out``: as in :meth:`kneighbors_chunks` -- the distances the predictions are reduced from are
        placed within the :class:`sknnr_amd.DistanceDomain`'s table on the device, with or without ``return_neighbors``,
        and ``domain_out`` (uint8, ``(N_total,)``) receives the codes.  ``beyond="nodata"`` (the domain needs a
        threshold): the predictions of the pixels whose distance is above it are blanked on the device before they are
        stored or enter ``zonal`` -- NaN, or ``out_nodata`` in a typed output, which an integer ``out_dtype`` then needs
        -- exactly as a nodata pixel's are; their neighbours, distances, ``usage`` and codes are untouched.  With
        ``beyond="keep"`` (the default) the call returns and writes exactly what it does without the keywords.  Refused
        with callable weights and under the host-side tie policies.

        ``bootstrap`` (a :class:`sknnr_amd.Bootstrap`): the planes are bootstrap statistics as :meth:`summarize` defines
        them -- ``outputs`` takes ``(target, "boot_se" | "boot_mean" | "boot_bias")`` and ``"boot_count"``, by default
        ``boot_se`` of every target; the stream searches ``bootstrap.n_candidates`` neighbours once and reduces every
        replicate from them on the device.  The result is ``(N, n_out)`` (``(n_out, N)`` with ``layout="bands"``), always
        2-D, and equals ``summarize(np.concatenate(tiles), outputs=outputs, bootstrap=...)`` bit for bit.  ``out``,
        ``nodata``, ``layout`` and ``out_dtype`` / ``scale`` / ``offset`` / ``out_nodata`` apply unchanged, except that an
        integer ``out_dtype`` always needs ``out_nodata``: the planes can be NaN.  ``statistic``, ``usage``, ``domain``,
        ``return_neighbors`` and ``zonal`` are refused."""
        bands = _check_layout(layout)
        check_is_fitted(self, "_fit_X")
        products = StreamProducts(usage, zones, zonal, domain, domain_out, beyond, bootstrap)
        if bootstrap is not None:
            products.bootstrap_request(self, statistic, outputs, return_neighbors=return_neighbors,
                                       return_dataframe_index=return_dataframe_index, neighbors_out=neighbors_out,
                                       index_dtype=index_dtype, distance_dtype=distance_dtype)
        else:
            neighbors = self._neighbor_request(return_neighbors, return_distance, return_dataframe_index, neighbors_out,
                                               fill_index, index_dtype, distance_dtype)
            statistic = resolve_statistic(statistic, outputs, self._n_targets())
        if nodata is not None:
            nodata = normalize_nodata(nodata, self.n_features_in_, np.float64)
        validate = self._validate_query
        if bands:
            validate = lambda t: normalize_band_tile(t, self.n_features_in_, estimator=type(self).__name__)  # noqa: E731
        typed = (out_dtype, scale, offset, out_nodata)
        if bootstrap is not None:
            return self._bootstrap_chunks(tiles, validate, products, apply_affine=False, out=out, owner=None, nodata=nodata,
                                          bands=bands, typed=typed)
        return self._predict_chunks(tiles, validate, products, apply_affine=False, out=out, owner=None, nodata=nodata,
                                    bands=bands, typed=typed, statistic=statistic, neighbors=neighbors)

    def _bootstrap_chunks(self, tiles, validate, products, *, apply_affine, out, owner, nodata, bands, typed):
        """``predict_chunks(bootstrap=...)``: one stream at ``kw`` candidates whose reduction stage is the bootstrap."""
        kw, plan, _ = products.request
        n_out = len(plan[0])
        output = normalize_typed_output(*typed, n_out, True)  # (a plane can be NaN without any mask)
        weights = "uniform" if self.weights is None else self.weights
        if out is not None and out.ndim != 2:
            raise ValueError(f"out must be 2-D, ({'n_out, N' if bands else 'N, n_out'}), with bootstrap=; got {out.ndim}-D")
        o = None if out is None else (None, None, out)
        _, _, pred = self._stream_tiles(tiles, validate, kw, products=products, apply_affine=apply_affine, weights=weights,
                                        return_distance=False, use_deterministic_ordering=True, out=o, owner=owner,
                                        nodata=nodata, bands=bands, output=output)
        return pred

    def _predict_chunks(self, tiles, validate, products, *, apply_affine, out, owner, nodata=None, bands=False, typed=None,
                        statistic=None, neighbors=None):
        """``neighbors``: :meth:`_neighbor_request`, or None -- predictions alone, exactly as before the keyword existed.
        ``products``: the call's :class:`sknnr_amd._products.StreamProducts`, checked here, every refusal before any
        device work."""
        weights = "uniform" if self.weights is None else self.weights
        # A distance-weight law (sknnr_amd.weights) is evaluated on the device inside the stream, so it goes wherever
        # "distance" goes; any other callable runs on the host and keeps every refusal below.
        law = isinstance(weights, DistanceWeights)
        host_callable = callable(weights) and not law
        output = None
        products.check_usage(self, self.n_neighbors, host_callable)
        blank = products.check_beyond()
        products.check_domain(self, self.n_neighbors, host_callable)
        plan = statistic if isinstance(statistic, OutputPlan) else None
        flat = self._y.ndim == 1 and (plan is None or plan.per_target)  # the result is 1-D
        if typed is not None:
            n_targets = plan.n_out if plan is not None else (1 if self._y.ndim == 1 else self._y.shape[1])
            # (a compact law can give an all-zero row: NaN predictions occur without any mask)
            # (so can the domain's mask: a blanked pixel is stored as a nodata pixel is)
            output = normalize_typed_output(*typed, n_targets, nodata is not None or (law and weights.can_vanish) or blank)
        products.check_zonal(self, plan.n_out if plan is not None else self._n_targets(), output, host_callable)
        if neighbors is not None:
            if host_callable:
                self._refuse_callable_weights("return_neighbors is")
            return self._predict_chunks_neighbors(tiles, validate, weights, neighbors, products, apply_affine=apply_affine,
                                                  out=out, owner=owner, nodata=nodata, bands=bands, output=output,
                                                  statistic=statistic)
        if host_callable and output:
            self._refuse_callable_weights("typed outputs are")
        if host_callable and bands:
            self._refuse_callable_weights("layout='bands' is", "on row-major neighbours")
        if host_callable and nodata is not None:
            self._refuse_callable_weights("nodata is")
        if host_callable:  # a Python callable runs between the search and the reduction: tile by tile
            # (every side product has refused it: ``products`` is empty here)
            # (the reorder's second key is the row's position in the WHOLE call: carry it from tile to tile)
            preds, row = [], 0
            for t in tiles:
                t = validate(t)
                if statistic is not None:
                    preds.append(self._summarize_engine(t, statistic, apply_affine=apply_affine, row_offset=row, owner=owner))
                else:
                    preds.append(self._predict_engine(t, apply_affine=apply_affine, row_offset=row, owner=owner))
                row += t.shape[0]
            pred = (np.concatenate([p.reshape(len(p), -1) for p in preds]) if preds
                    else np.empty((0, self.engine_.t if plan is None else plan.n_out)))
            if out is not None:
                out[:len(pred)] = pred.reshape((len(pred),) + out.shape[1:])  # (out is 1-D for a 1-D y)
                pred = out[:len(pred)]
        else:
            o = None if out is None else (None, None, out.reshape(out.shape[0], -1))
            if bands and out is not None and out.ndim == 1:  # (a 1-D y: the one target plane)
                o = (None, None, out.reshape(1, -1))
            _, _, pred = self._stream_tiles(tiles, validate, self.n_neighbors, products=products, apply_affine=apply_affine,
                                            weights=weights, return_distance=False,
                                            use_deterministic_ordering=True, out=o, owner=owner, nodata=nodata,
                                            bands=bands, output=output, statistic=statistic)
            if out is None and not output and statistic is None:  # the stream's float64 rows hold float32 values where scikit-learn returns float32
                pred = pred.astype(self.engine_.pred_dtype(weights), copy=False)
        return pred.reshape(-1) if flat else pred

    def _predict_chunks_neighbors(self, tiles, validate, weights, neighbors, products, *, apply_affine, out, owner, nodata,
                                  bands, output, statistic):
        """``predict_chunks(return_neighbors=True)``: one stream with all three outputs.  ``output``: the predictions'
        typed output (or None); the neighbours' types and the id table are worked out here, as ``kneighbors_chunks``
        does, every refusal before any device work."""
        self._check_stream_supported("return_neighbors is")
        return_distance, ids, fill_index = (neighbors[key] for key in ("return_distance", "return_dataframe_index", "fill_index"))
        n_output = self._neighbor_output(neighbors["index_dtype"], neighbors["distance_dtype"], return_distance, ids,
                                         fill_index, nodata is not None)
        table = self._device_id_table(ids)
        o_dist, o_idx = neighbors["neighbors_out"] or (None, None)
        o_pred = None if out is None else out.reshape(out.shape[0], -1)
        if bands and out is not None and out.ndim == 1:  # (a 1-D y: the one target plane)
            o_pred = out.reshape(1, -1)
        o = None if (o_dist is None and o_idx is None and o_pred is None) else (o_dist, o_idx, o_pred)
        merged = {**(output or {}), **(n_output or {})} or None
        dist, idx, pred = self._stream_tiles(tiles, validate, self.n_neighbors, products=products, apply_affine=apply_affine,
                                             weights=weights, return_distance=return_distance,
                                             use_deterministic_ordering=True, out=o, owner=owner, nodata=nodata,
                                             fill_index=-1 if ids else fill_index, bands=bands, output=merged,
                                             statistic=statistic, id_table=table, fill_id=fill_index, neighbors=True)
        if out is None and not output and statistic is None:  # (as without neighbours: float32 where scikit-learn returns it)
            pred = pred.astype(self.engine_.pred_dtype(weights), copy=False)
        if self._y.ndim == 1 and not (isinstance(statistic, OutputPlan) and not statistic.per_target):
            pred = pred.reshape(-1)
        found = self._finish_chunks(dist, idx, return_distance, ids, fill_index=None if nodata is None else fill_index,
                                    on_device=table is not None)
        return (pred, *found) if return_distance else (pred, found)

    # -- neighbour replay: attribute maps from stored neighbour rasters ---------------------------
    def _replay_target_engine(self, y):
        """How to get the engine whose targets a replay reduces (called when the first tile is pushed: after every
        refusal), whether the result is 1-D, the number of targets and their dtype: the estimator's own for ``y`` None,
        else an attribute-only engine on ``y``, cached by the table's identity."""
        if y is None:
            return (lambda: self.engine_), self._y.ndim == 1, self._n_targets(), self._y.dtype
        table = np.asarray(y)
        if table.dtype.kind not in "fiub" or table.ndim not in (1, 2):
            raise ValueError(f"y must be a numeric (n_samples, n_attributes) table, got {table.dtype} with shape {table.shape}")
        if table.shape[0] != self.n_samples_fit_:
            raise ValueError(f"y has {table.shape[0]} rows, but the estimator was fitted with {self.n_samples_fit_} samples")
        if table.size == 0:
            raise ValueError("y holds no attribute")
        n_targets = 1 if table.ndim == 1 else table.shape[1]

        def engine():
            held = getattr(self, "_replay_targets", None)
            if held is None or held[0] is not y:
                if held is not None:
                    held[1].close()
                eng = KNNEngine.for_targets(np.ascontiguousarray(table.reshape(len(table), -1), dtype=np.float64),
                                            device=self._device, target_dtype=table.dtype)
                self._replay_targets = held = (y, eng)
            return held[1]
        return engine, table.ndim == 1, n_targets, table.dtype

    def _replay_id_table(self, ids):
        """The fitted dataframe ids as the int64 table stored ids are looked up in (``ids=True``), or None."""
        if not ids:
            return None
        check_is_fitted(self, "dataframe_index_in_", msg="ids=True needs an estimator fitted with a dataframe: the stored "
                                                         "values are looked up in its index.")
        table = np.asarray(self.dataframe_index_in_)
        if table.dtype.kind not in "iu":
            raise NotImplementedError(f"ids=True needs integer dataframe ids, got {table.dtype}: labels of another kind "
                                      "are not looked up on the device")
        if table.dtype.itemsize > 8 or table.dtype == np.uint64:
            raise ValueError(f"ids=True needs dataframe ids that fit int64, got {table.dtype}")
        table = table.astype(np.int64)
        if np.unique(table).size != table.size:
            raise ValueError("ids=True needs unique dataframe ids: a stored id must name one reference row")
        return table

    @staticmethod
    def _replay_tile(tile, bands, number):
        """One tile of stored neighbours -- ``idx`` or ``(dist, idx)`` -- as ``(idx, dist or None)``: rows ``(n, ks)``, or
        with ``bands`` planes ``(ks, n)`` from any ``(ks, ...)`` trailing shape (the rule of :func:`normalize_band_tile`)."""
        dist = None
        if isinstance(tile, (tuple, list)) and len(tile) == 2 and all(hasattr(a, "shape") for a in tile):
            dist, tile = tile
        idx = np.asarray(tile)
        if idx.dtype.kind not in "iu" or idx.dtype in (np.uint32, np.uint64):
            raise ValueError(f"tile {number}: stored neighbours are int32 or int64 row positions or ids, got {idx.dtype}")
        if idx.dtype.itemsize < 4:
            idx = idx.astype(np.int32)
        if dist is not None:
            dist = np.asarray(dist)
            if dist.dtype not in (np.float32, np.float64):
                raise ValueError(f"tile {number}: stored distances are float32 or float64, got {dist.dtype}")
            if dist.shape != idx.shape:
                raise ValueError(f"tile {number}: the distances have shape {dist.shape}, the indices {idx.shape}")
        if idx.ndim < 2:
            raise ValueError(f"tile {number}: a tile of stored neighbours is (n, ks), or (ks, ...) with layout='bands', "
                             f"got shape {idx.shape}")
        if bands:
            idx = idx.reshape(idx.shape[0], int(np.prod(idx.shape[1:])))
            dist = None if dist is None else dist.reshape(idx.shape)
        elif idx.ndim != 2:
            raise ValueError(f"tile {number}: a row tile of stored neighbours is (n, ks), got shape {idx.shape}")
        return idx, dist

    def predict_neighbors_chunks(self, neighbor_tiles, y=None, n_neighbors=None, ids=False, fill_index=-1, unknown="raise",
                                 out=None, layout="rows", out_dtype=None, scale=None, offset=None, out_nodata=None,
                                 statistic=None, outputs=None, usage=None, zones=None, zonal=None, domain=None,
                                 domain_out=None, beyond="keep"):
        """``predict_chunks`` from STORED neighbours instead of feature rows: the neighbour raster that
        ``kneighbors_chunks(...)`` or ``predict_chunks(..., return_neighbors=True, neighbors_out=...)`` wrote is replayed
        through the same device pipeline, and no search runs.  The result is bit-identical to the search call that wrote
        those neighbours.

        ``neighbor_tiles``: an iterable of ``idx`` or ``(dist, idx)`` host arrays -- int32 / int64 row positions (or
        dataframe ids with ``ids=True``) and float32 / float64 distances; ``(n, ks)`` rows, or with ``layout="bands"``
        any ``(ks, ...)`` shape.  All tiles of a call share one dtype pair and one ``ks``.  ``n_neighbors``: the
        ``k <= ks`` leading columns in use, by default ``min(self.n_neighbors, ks)``; ``k < ks`` means "the first k
        stored columns", which need not equal a fresh k-search where neighbours tie.

        ``y``: an array-like or DataFrame ``(n_samples_fit_, t')`` reduced in place of the fitted targets -- a table the
        estimator was never fitted with; ``outputs``, ``statistic``, ``scale`` and ``offset`` then count its columns.
        A pixel whose first stored value equals ``fill_index`` is masked (NaN, or ``out_nodata``).  A stored value that
        names no reference row makes its pixel unknown: ``unknown="raise"`` raises a ``ValueError`` at the end of the
        call (the contents of ``out`` are then unspecified), ``unknown="nodata"`` stores it as a masked pixel -- an
        integer ``out_dtype`` then needs ``out_nodata`` -- and the count is ``self.replay_unknown_`` either way.
        ``uniform`` weights need no distances; ``distance`` weights, the laws of :mod:`sknnr_amd.weights`, ``usage`` and
        ``domain`` need them.  Every other keyword has the meaning and the refusals it has in :meth:`predict_chunks`.
        (Bootstrap planes from a stored raster: :meth:`bootstrap_neighbors_chunks`.)"""
        products = StreamProducts(usage, zones, zonal, domain, domain_out, beyond)
        return self._replay_chunks(neighbor_tiles, products, y=y, n_neighbors=n_neighbors, ids=ids, fill_index=fill_index,
                                   unknown=unknown, out=out, layout=layout, out_dtype=out_dtype, scale=scale, offset=offset,
                                   out_nodata=out_nodata, statistic=statistic, outputs=outputs)

    def bootstrap_neighbors_chunks(self, neighbor_tiles, bootstrap, y=None, n_neighbors=None, ids=False, fill_index=-1,
                                   unknown="raise", out=None, layout="rows", out_dtype=None, scale=None, offset=None,
                                   out_nodata=None, outputs=None):
        """``predict_chunks(..., bootstrap=bootstrap)`` from STORED neighbours: the bootstrap planes of a
        :class:`sknnr_amd.Bootstrap` reduced from the neighbour raster a search stream stored, through the replay pipeline of
        :meth:`predict_neighbors_chunks`; no search runs.  ``n_neighbors`` is the number of CANDIDATES ``kw`` taken from the
        stored columns (by default ``bootstrap.n_candidates``, else every stored column) and the replicate size is the
        estimator's ``n_neighbors``; the result equals the search-side bootstrap that searched those ``kw`` neighbours bit
        for bit.  ``outputs`` as in :meth:`summarize` with ``bootstrap=``; ``y``, ``ids``, ``fill_index``, ``unknown``,
        ``out``, ``layout`` and the typed-output keywords as in :meth:`predict_neighbors_chunks` (an integer ``out_dtype``
        always needs ``out_nodata``).  The result is ``(N, n_out)``, ``(n_out, N)`` with ``layout="bands"``."""
        if bootstrap is None:
            raise TypeError("bootstrap must be a sknnr_amd.Bootstrap, got NoneType")
        return self._replay_chunks(neighbor_tiles, StreamProducts(bootstrap=bootstrap), y=y, n_neighbors=n_neighbors, ids=ids,
                                   fill_index=fill_index, unknown=unknown, out=out, layout=layout, out_dtype=out_dtype,
                                   scale=scale, offset=offset, out_nodata=out_nodata, outputs=outputs)

    def bootstrap_neighbors(self, idx, dist=None, *, bootstrap, **kwargs):
        """:meth:`bootstrap_neighbors_chunks` on one tile of stored neighbours, through the same path."""
        return self.bootstrap_neighbors_chunks([idx if dist is None else (dist, idx)], bootstrap, **kwargs)

    def _replay_chunks(self, neighbor_tiles, products, y=None, n_neighbors=None, ids=False, fill_index=-1, unknown="raise",
                       out=None, layout="rows", out_dtype=None, scale=None, offset=None, out_nodata=None, statistic=None,
                       outputs=None):
        """The replay behind :meth:`predict_neighbors_chunks` and, with a bootstrap among ``products`` (the call's
        :class:`sknnr_amd._products.StreamProducts`), :meth:`bootstrap_neighbors_chunks`."""
        bands = _check_layout(layout)
        check_is_fitted(self, "_fit_X")
        if unknown not in ("raise", "nodata"):
            raise ValueError(f"unknown must be 'raise' or 'nodata', got {unknown!r}")
        blank = products.check_beyond()
        weights = "uniform" if self.weights is None else self.weights
        law = isinstance(weights, DistanceWeights)
        if callable(weights) and not law:
            self._refuse_callable_weights("predict_neighbors_chunks is")
        self._check_stream_supported("predict_neighbors_chunks is")
        if isinstance(fill_index, bool) or not isinstance(fill_index, numbers.Integral):
            raise ValueError(f"fill_index must be an integer, got {fill_index!r}")
        engine, flat, n_targets, target_dtype = self._replay_target_engine(y)
        id_table = self._replay_id_table(ids)
        bootstrap, boot = products.bootstrap, None
        if bootstrap is not None:  # (every refusal before any device work)
            boot = products.bootstrap_request(self, statistic, outputs, n_targets=n_targets, stored=True)
            statistic = outputs = None
        statistic = resolve_statistic(statistic, outputs, n_targets)
        plan = statistic if isinstance(statistic, OutputPlan) else None
        flat = flat and (plan is None or plan.per_target) and boot is None
        t_cols = n_targets if plan is None else plan.n_out
        if boot is not None:
            t_cols = len(boot[1][0])
        output = normalize_typed_output(out_dtype, scale, offset, out_nodata, t_cols,
                                        unknown == "nodata" or (law and weights.can_vanish) or blank or boot is not None)
        products.check_zonal(self, t_cols, output)
        products.check_usage(self)
        needs_dist = [name for name, on in (("weights='distance'", weights == "distance"), ("a weight law", law),
                                            ("usage", products.usage is not None),
                                            ("domain", products.domain is not None)) if on]

        def settle(k, has_dist):  # what needs k or the first tile, still before any device work
            products.settle(self, k)
            if needs_dist and not has_dist:
                raise ValueError(f"{' and '.join(needs_dist)} need{'s' if len(needs_dist) == 1 else ''} the stored "
                                 "distances: pass (dist, idx) tiles")
        if n_neighbors is not None and (isinstance(n_neighbors, bool) or not isinstance(n_neighbors, numbers.Integral)
                                        or n_neighbors < 1):
            raise ValueError(f"n_neighbors must be a positive integer, got {n_neighbors!r}")
        # (the rank is checked against k by settle(), once the first tile has shown ks)
        products.check_domain(self, None if n_neighbors is None else int(n_neighbors))
        out_kw = {key: v for key, v in (output or {}).items() if v is not None}
        pred_dt = np.dtype(out_kw.get("pred_dtype", np.float64))
        o_pred = None
        if out is not None:
            o_pred = out.reshape(1, -1) if bands and out.ndim == 1 else out.reshape(out.shape[0], -1)
        pieces, tile_of_push, row, stream, shape_key, k = [], [], 0, None, None, None
        counts = dict(unknown=0, first_unknown=-1)
        try:
            for number, tile in enumerate(neighbor_tiles):
                products.next_tile()
                idx, dist = self._replay_tile(tile, bands, number)
                ks, n = (idx.shape[0], idx.shape[1]) if bands else (idx.shape[1], idx.shape[0])
                key = (ks, idx.dtype, None if dist is None else dist.dtype)
                if shape_key is None:
                    shape_key = key
                    if ks < 1:
                        raise ValueError(f"tile {number}: the tile holds no neighbour column")
                    k = min(self.n_neighbors, ks) if n_neighbors is None else int(n_neighbors)
                    if boot is not None and n_neighbors is None:  # (k is the number of candidates)
                        k = ks if bootstrap.n_candidates is None else bootstrap.n_candidates
                    if k > ks:
                        raise ValueError(f"n_neighbors={k} is above the {ks} stored neighbour columns")
                    if boot is not None:  # (k is kw: the caps of Bootstrap.candidates, before any device work)
                        if self.n_neighbors > k:
                            raise ValueError(f"bootstrap: n_neighbors = {self.n_neighbors} exceeds the {k} candidates in use: a "
                                             "replicate takes k of the kw neighbours stored")
                        if k > MAX_CANDIDATES:
                            raise ValueError(f"bootstrap: {k} candidates in use exceed the limit of {MAX_CANDIDATES}: pass "
                                             "n_neighbors (or n_candidates) to take the leading columns")
                        if k > self.n_samples_fit_:
                            raise ValueError(f"bootstrap: {k} candidates in use exceed the {self.n_samples_fit_} rows that "
                                             "can be neighbours")
                    settle(k, dist is not None)
                elif key != shape_key:
                    raise ValueError(f"tile {number}: the tiles of one call share one ks and one dtype pair: got ks={ks}, "
                                     f"{idx.dtype} / {key[2]} after ks={shape_key[0]}, {shape_key[1]} / {shape_key[2]}")
                if n == 0:
                    continue
                if stream is None:
                    eng = engine()
                    if id_table is not None:
                        eng.set_replay_ids(id_table)
                    stream = eng.open_replay(k, ks, weights=weights, idx_dtype=idx.dtype,
                                             dist_dtype=None if dist is None else dist.dtype, fill_index=int(fill_index),
                                             ids=id_table is not None, output=out_kw,
                                             **(dict(statistic=statistic) if plan is None else dict(plan=plan.arrays)),
                                             **products.open_keywords(eng, self.n_neighbors))
                window = _out_window(o_pred, row, n, t_cols, pred_dt, bands, "out")
                products.feed(stream, row, n)
                got = (stream.push_planes if bands else stream.push)(idx, dist, out_pred=window)
                tile_of_push.append(number)
                if o_pred is None:
                    pieces.append(got[2])
                row += n
            products.end_of_tiles()
            if shape_key is None:  # (no tile at all: what can be checked without one)
                settle(self.n_neighbors if n_neighbors is None else int(n_neighbors), True)
            if stream is not None:
                done, stream = stream, None
                try:
                    counts = done.counts()
                    products.collect(done)
                finally:
                    done.close()
            self.replay_unknown_ = int(counts["unknown"])
            if counts["unknown"] and unknown == "raise":
                raise ValueError(f"{counts['unknown']} pixels hold stored neighbours that name no reference row (an id that "
                                 f"is not in the fitted index, or a position outside [0, {self.n_samples_fit_})); the first "
                                 f"of them are in tile {tile_of_push[counts['first_unknown']]}.  Pass unknown='nodata' to "
                                 "store them as nodata pixels")
            products.commit(self, k if k is not None else self.n_neighbors)
        except _native.HipBackendError as err:
            _reraise(err, self)
        finally:
            if stream is not None:  # an error on the way: free the native stream without masking it
                try:
                    stream.close()
                except _native.HipBackendError:
                    pass
        if o_pred is not None:
            pred = o_pred[:, :row] if bands else o_pred[:row]
            if out.ndim == 1:
                pred = pred.reshape(-1)
            return pred
        pred = (np.concatenate(pieces, axis=1 if bands else 0) if pieces
                else np.empty((t_cols, 0) if bands else (0, t_cols), dtype=pred_dt))
        if not output and statistic is None and target_dtype == np.float32 and weights == "uniform":
            pred = pred.astype(np.float32, copy=False)  # (float32 where scikit-learn returns it, as predict_chunks)
        return pred.reshape(-1) if flat else pred

    def predict_neighbors(self, idx, dist=None, **kwargs):
        """:meth:`predict_neighbors_chunks` on one tile of stored neighbours, through the same path."""
        return self.predict_neighbors_chunks([idx if dist is None else (dist, idx)], **kwargs)

    def score(self, X, y, sample_weight=None):
        """R^2 of ``predict(X)`` (``X`` may be None as in REF _base.py:40)."""
        pred = self.predict(X)
        if is_torch_cuda_tensor(pred):
            pred = pred.cpu().numpy()
        return float(r2_score(y, pred, sample_weight=sample_weight))

    def __sklearn_tags__(self):
        tags = super().__sklearn_tags__()
        tags.input_tags.sparse = False
        return tags


class TransformedKNeighborsRegressor(BaseEstimator, ABC):
    """kNN regressors that search in a transformed feature space (REF _base.py:185-358).

    ``fit`` learns the transformer on the host, maps the training rows through the GPU
    affine kernel, and installs the same map in the engine so that ``kneighbors`` /
    ``predict`` take *untransformed* rows and transform them inside the launch.  Tree-node
    spaces (RFNN / GBNN) install their forests instead: query rows are walked down every tree
    on the device (``sknnr_index_set_forest``) and never visit scikit-learn's ``apply``.
    """

    def __init__(self, n_neighbors=5, *, weights="uniform", algorithm="auto", leaf_size=30, p=2,
                 metric="minkowski", metric_params=None, n_jobs=None):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.p = p
        self.metric = metric
        self.metric_params = metric_params
        self.n_jobs = n_jobs

    @abstractmethod
    def _get_transformer(self):
        """The (unfitted) transformer that defines the feature space."""

    def _set_fitted_transformer(self, X, y) -> None:
        self.transformer_ = self._get_transformer().fit(X, y)

    def _get_additional_regressor_init_kwargs(self) -> dict:
        return {}

    def _transform_X(self, X):
        """Host-side transform, kept for API parity (REF _base.py:236-239); the hot path does
        not use it -- queries are transformed on the device."""
        check_is_fitted(self, "transformer_")
        return self.transformer_.transform(X) if X is not None else X

    def fit(self, X, y):
        validate_data(self, X=X, y=y, ensure_all_finite=True, multi_output=True)
        self._set_fitted_transformer(X, y)

        device = default_device()
        # Affine feature spaces are applied on the device (fit rows here, query rows inside the launch); tree-node spaces
        # (scikit-learn forests) map the fit rows on the host and install the forests for the query rows.
        self._device_affine = hasattr(self.transformer_, "affine_params")
        self._device_forest = hasattr(self.transformer_, "forest_image")
        if self._device_affine:
            center, scale, proj = self.transformer_.affine_params()
            X_arr = np.ascontiguousarray(
                validate_data(self.transformer_, X=X, reset=False, dtype=np.float64), dtype=np.float64)
            X_transformed = _native.affine_transform_host(X_arr, center, scale, proj, device=device)
            affine = (X_arr.shape[1], center, scale, proj)
        else:
            X_transformed = self.transformer_.transform(X)
            affine = None

        kwargs = {
            "n_neighbors": self.n_neighbors, "weights": self.weights, "algorithm": self.algorithm,
            "leaf_size": self.leaf_size, "p": self.p, "metric": self.metric,
            "metric_params": self.metric_params, "n_jobs": self.n_jobs,
        }
        kwargs.update(self._get_additional_regressor_init_kwargs())
        self.regressor_ = RawKNNRegressor(**kwargs)
        forest = self.transformer_.forest_image() if self._device_forest else None
        self.regressor_._fit_arrays(X_transformed, y, affine=affine, device=device, forest=forest)
        self.regressor_._set_dataframe_index_in(X)

        self.n_features_in_ = self.regressor_.n_features_in_
        self.independent_prediction_ = self.regressor_.independent_prediction_
        self.independent_score_ = self.regressor_.independent_score_
        if hasattr(self.regressor_, "dataframe_index_in_"):
            self.dataframe_index_in_ = self.regressor_.dataframe_index_in_
        return self

    def _map_on_device(self) -> bool:
        """Do query rows reach the engine raw, to be mapped there (affine map or forests)?"""
        return self._device_affine or getattr(self, "_device_forest", False)

    def _validate_raw_query(self, X, host_ids=False):
        """Same checks the transformer's ``transform`` applies (feature names/count, finiteness)
        without transforming on the host -- or, for host-side feature spaces, the transform itself.
        ``host_ids``: tree-node spaces return scikit-learn's node ids (the reference-sharded search takes those)."""
        check_is_fitted(self, "transformer_")
        if getattr(self, "_device_forest", False) and not host_ids:
            return self._validate_forest_query(X)
        if not getattr(self, "_device_affine", True):
            if is_torch_cuda_tensor(X):
                X = X.cpu().numpy()
            return np.ascontiguousarray(self.transformer_.transform(X), dtype=np.float64)
        if is_torch_cuda_tensor(X):
            d_in = self.regressor_.engine_.d_in
            if X.ndim != 2 or X.shape[1] != d_in:
                raise ValueError(f"X has {X.shape[-1]} features, but {type(self).__name__} is expecting "
                                 f"{d_in} features as input.")
            return X
        # finiteness is tested on the device by the kernel that reads the rows (check_finite)
        return validate_data(self.transformer_, X=X, reset=False, dtype=_QUERY_DTYPES, order="C",
                             ensure_all_finite=False)

    def _validate_forest_query(self, X):
        """Tree-node spaces: the checks of ``transform``'s ``validate_data`` (feature names / count; finiteness and the
        float32 range on the device), the rows kept at their own width.  ``apply`` converts them to float32 in one
        rounding; every kept type reaches float32 exactly that way through float64, 64-bit integers do not (two
        roundings above 2^53), so those are converted to float32 here, as ``apply`` would."""
        name = type(self.transformer_).__name__
        if is_torch_cuda_tensor(X):
            import torch

            d_in = self.regressor_.engine_.d_in
            if X.ndim != 2 or X.shape[1] != d_in:
                raise ValueError(f"X has {X.shape[-1]} features, but {name} is expecting {d_in} features as input.")
            return X.to(torch.float32) if X.dtype in (torch.int64, getattr(torch, "uint64", torch.int64)) else X
        X = validate_data(self.transformer_, X=X, reset=False, dtype=_QUERY_DTYPES + [np.int64, np.uint64], order="C",
                          ensure_all_finite=False)
        return X.astype(np.float32) if X.dtype in (np.int64, np.uint64) else X

    def _host_result(self, X, out):
        """Tree-node spaces answered CUDA-tensor queries with host arrays before their map moved to the device: so they
        still do."""
        if getattr(self, "_device_forest", False) and is_torch_cuda_tensor(X):
            return tuple(None if a is None else a.cpu().numpy() for a in out) if isinstance(out, tuple) else out.cpu().numpy()
        return out

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True, return_dataframe_index=False,
                   use_deterministic_ordering=True):
        """REF _base.py:285-344."""
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        k = reg._resolve_k(n_neighbors)
        if X is not None:
            X = self._validate_raw_query(X)
        dist, idx = self._host_result(X, reg._kneighbors_engine(X, k, apply_affine=X is not None and self._map_on_device(),
                                                                use_deterministic_ordering=use_deterministic_ordering,
                                                                owner=self.transformer_))
        return reg._finish_kneighbors(dist, idx, return_distance, return_dataframe_index)

    def predict(self, X):
        """REF _base.py:346-348 (``X=None``: the independent prediction, as the reference's
        ``_transform_X(None)`` passes None through to the regressor)."""
        check_is_fitted(self, "regressor_")
        if X is not None:
            X = self._validate_raw_query(X)
        return self._host_result(X, self.regressor_._predict_engine(X, apply_affine=X is not None and self._map_on_device(),
                                                                    owner=self.transformer_))

    def summarize(self, X=None, statistic=None, outputs=None, bootstrap=None):
        """Per-target summaries of each query's neighbours (:meth:`RawKNNRegressor.summarize`, also for the definitions
        of ``statistic`` and of ``outputs``, the ``(target, statistic)`` pairs reduced from one search, and for
        ``bootstrap``; the transform stays the one fitted on all plots); ``X=None``: of every fitted row's neighbours,
        itself excluded."""
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        if bootstrap is not None:
            request = reg._bootstrap_request(bootstrap, statistic, outputs, self_query=X is None)
            if X is not None:
                X = self._validate_raw_query(X)
            return self._host_result(X, reg._bootstrap_engine(X, bootstrap, request, owner=self.transformer_,
                                                              apply_affine=X is not None and self._map_on_device()))
        if statistic is None and outputs is None:
            statistic = "mean"
        stat = resolve_statistic(statistic, outputs, reg._n_targets())
        if X is not None:
            X = self._validate_raw_query(X)
        return self._host_result(X, reg._summarize_engine(X, stat, apply_affine=X is not None and self._map_on_device(),
                                                          owner=self.transformer_))

    def independent_kneighbors(self, groups=None, n_neighbors=None, return_distance=True, return_dataframe_index=False,
                               use_deterministic_ordering=True, *, buffer=None):
        """Leave-group-out and buffered leave-out neighbours of every fitted row, in the transformed space the estimator
        searches (:meth:`RawKNNRegressor.independent_kneighbors`, also for the contract and the tie rule)."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.independent_kneighbors(groups, n_neighbors, return_distance, return_dataframe_index,
                                                      use_deterministic_ordering, buffer=buffer)

    def independent_predict(self, groups=None, *, buffer=None):
        """:meth:`RawKNNRegressor.independent_predict` of the fitted regressor."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.independent_predict(groups, buffer=buffer)

    def independent_summarize(self, groups=None, statistic=None, outputs=None, *, buffer=None):
        """:meth:`RawKNNRegressor.independent_summarize` of the fitted regressor."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.independent_summarize(groups, statistic, outputs, buffer=buffer)

    def independent_score(self, groups=None, *, buffer=None):
        """R^2 of :meth:`independent_predict` against the fitted targets (no ``sample_weight``, as :meth:`score`)."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.independent_score(groups, buffer=buffer)

    def buffer_counts(self, buffer, groups=None):
        """:meth:`RawKNNRegressor.buffer_counts` of the fitted regressor."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.buffer_counts(buffer, groups)

    def neighbor_usage(self, X=None, n_neighbors=None):
        """The :class:`sknnr_amd.NeighborUsage` of ``kneighbors(X, n_neighbors)`` (:meth:`RawKNNRegressor.neighbor_usage`)."""
        dist, idx = self.kneighbors(X, n_neighbors=n_neighbors)
        reg = self.regressor_
        try:
            return reg._usage_from_neighbors(dist, idx)
        except _native.HipBackendError as err:
            _reraise(err, self)

    def independent_neighbor_usage(self, groups=None, n_neighbors=None, *, buffer=None):
        """:meth:`RawKNNRegressor.independent_neighbor_usage` of the fitted regressor."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.independent_neighbor_usage(groups, n_neighbors, buffer=buffer)

    def distance_domain(self, groups=None, *, buffer=None, rank=1, p=None, threshold=None):
        """:meth:`RawKNNRegressor.distance_domain` of the fitted regressor: the table holds distances in the transformed
        space the estimator searches in."""
        check_is_fitted(self, "regressor_")
        return self.regressor_.distance_domain(groups, buffer=buffer, rank=rank, p=p, threshold=threshold)

    def domain_scores(self, domain, X=None, n_neighbors=None):
        """The uint8 distance-domain codes of ``kneighbors(X, n_neighbors)`` within ``domain``, its tallies added to it
        (:meth:`RawKNNRegressor.domain_scores`)."""
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        if not isinstance(domain, DistanceDomain):
            raise TypeError(f"domain must be a sknnr_amd.DistanceDomain, got {type(domain).__name__}")
        if domain.rank > reg._resolve_k(n_neighbors):
            raise ValueError(f"domain.rank={domain.rank} is above n_neighbors={reg._resolve_k(n_neighbors)}")
        dist, _ = self.kneighbors(X, n_neighbors=n_neighbors)
        return reg._domain_scores(domain, dist)

    def _raw_nodata(self, nodata):
        """``nodata`` of a streamed call, one value per UNTRANSFORMED input column: the mask reads the raw rows, so they
        must reach the engine raw (affine map or forests on the device)."""
        if nodata is None:
            return None
        if not self._map_on_device():
            raise NotImplementedError(f"nodata is not supported by {type(self).__name__}: its transformer runs on the "
                                      "host, so the raw rows never reach the device")
        return normalize_nodata(nodata, self.regressor_.engine_.d_in, np.float64)

    def _band_validator(self, bands):
        """``layout="bands"``: the tiles' bands must reach the engine raw (affine map or forests on the device), where
        they are transposed; returns what turns a tile into ``(bands, n)``, or the row validator."""
        if not bands:
            return self._validate_raw_query
        if not self._map_on_device():
            raise NotImplementedError(f"layout='bands' is not supported by {type(self).__name__}: its transformer runs on "
                                      "the host, on row-major rows, so the bands never reach the device")
        d_in = self.regressor_.engine_.d_in
        forest = getattr(self, "_device_forest", False)
        name = type(self.transformer_).__name__ if forest else type(self).__name__
        return lambda t: normalize_band_tile(t, d_in, forest=forest, estimator=name)

    def kneighbors_chunks(self, tiles, n_neighbors=None, return_distance=True, return_dataframe_index=False,
                          use_deterministic_ordering=True, out=None, nodata=None, fill_index=-1, layout="rows",
                          index_dtype=None, distance_dtype=None, usage=None, domain=None, domain_out=None):
        """``kneighbors`` over an iterable of untransformed host tiles as one streamed call (see
        :meth:`RawKNNRegressor.kneighbors_chunks`, also for ``nodata`` / ``fill_index``: the nodata values are those of
        the untransformed columns -- for ``layout="bands"``, for ``index_dtype`` / ``distance_dtype``, for ``usage`` and
        for ``domain`` / ``domain_out``); each tile is transformed on the device."""
        bands = _check_layout(layout)
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        k = reg._resolve_k(n_neighbors)
        products = StreamProducts(usage=usage, domain=domain, domain_out=domain_out)
        products.check_domain(reg, k)
        validate = self._band_validator(bands)
        nodata = self._raw_nodata(nodata)
        output = reg._neighbor_output(index_dtype, distance_dtype, return_distance, return_dataframe_index, fill_index,
                                      nodata is not None)
        o = None if out is None else (out[0], out[1], None)
        table = reg._device_id_table(return_dataframe_index)
        products.check_usage(reg, k)
        dist, idx, _ = reg._stream_tiles(tiles, validate, k, products=products, apply_affine=self._map_on_device(),
                                         weights=None, return_distance=return_distance,
                                         use_deterministic_ordering=use_deterministic_ordering, out=o,
                                         owner=self.transformer_, nodata=nodata,
                                         fill_index=-1 if return_dataframe_index else fill_index, bands=bands,
                                         output=output, id_table=table, fill_id=fill_index)
        return reg._finish_chunks(dist, idx, return_distance, return_dataframe_index,
                                  fill_index=None if nodata is None else fill_index, on_device=table is not None)

    def predict_chunks(self, tiles, out=None, nodata=None, layout="rows", out_dtype=None, scale=None, offset=None,
                       out_nodata=None, statistic=None, return_neighbors=False, return_distance=True,
                       return_dataframe_index=False, neighbors_out=None, fill_index=-1, index_dtype=None,
                       distance_dtype=None, outputs=None, usage=None, zones=None, zonal=None, domain=None, domain_out=None,
                       beyond="keep", bootstrap=None):
        """``predict`` over an iterable of untransformed host tiles as one streamed call (``nodata``: masked rows are
        predicted NaN; ``layout="bands"``: band-first tiles and predictions; ``out_dtype`` / ``scale`` / ``offset`` /
        ``out_nodata``: predictions converted on the device to the type the raster is stored in; ``statistic``: one name
        or one per target -- mean, mode, min, max, nearest, std or ("quantile", q) of the neighbours in place of the
        mean; ``outputs``: ``(target, statistic)`` pairs instead, ``n_out`` planes from the one search;
        ``return_neighbors=True`` and the neighbour keywords: ``(pred, dist, idx)`` from one search; ``usage``: a
        :class:`sknnr_amd.NeighborUsage` the device's tally of the neighbours is added to; ``zones`` / ``zonal``: the zone
        codes of every tile and the :class:`sknnr_amd.ZonalStats` the device's zonal tables are added to; ``domain`` /
        ``domain_out`` / ``beyond``: the :class:`sknnr_amd.DistanceDomain` the pixels' distances are placed within on the
        device, the uint8 plane that receives the codes, and ``"nodata"`` to blank the predictions beyond its threshold;
        ``bootstrap``: a :class:`sknnr_amd.Bootstrap` -- the planes are bootstrap statistics reduced from one search at its
        ``n_candidates``, the transform staying the one fitted on all plots; see
        :meth:`RawKNNRegressor.kneighbors_chunks` / :meth:`RawKNNRegressor.predict_chunks`)."""
        bands = _check_layout(layout)
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        products = StreamProducts(usage, zones, zonal, domain, domain_out, beyond, bootstrap)
        common = dict(apply_affine=self._map_on_device(), out=out, owner=self.transformer_, bands=bands,
                      typed=(out_dtype, scale, offset, out_nodata))
        if bootstrap is not None:
            products.bootstrap_request(reg, statistic, outputs, return_neighbors=return_neighbors,
                                       return_dataframe_index=return_dataframe_index, neighbors_out=neighbors_out,
                                       index_dtype=index_dtype, distance_dtype=distance_dtype)
            return reg._bootstrap_chunks(tiles, self._band_validator(bands), products, nodata=self._raw_nodata(nodata),
                                         **common)
        neighbors = reg._neighbor_request(return_neighbors, return_distance, return_dataframe_index, neighbors_out,
                                          fill_index, index_dtype, distance_dtype)
        statistic = resolve_statistic(statistic, outputs, reg._n_targets())
        return reg._predict_chunks(tiles, self._band_validator(bands), products, nodata=self._raw_nodata(nodata),
                                   statistic=statistic, neighbors=neighbors, **common)

    def predict_neighbors_chunks(self, neighbor_tiles, **kwargs):
        """Attribute maps from STORED neighbours (:meth:`RawKNNRegressor.predict_neighbors_chunks`, with its keywords):
        the tiles hold neighbours, not feature rows, so nothing is transformed and nothing is searched; ``y=`` counts
        the fitted samples."""
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        try:
            return reg.predict_neighbors_chunks(neighbor_tiles, **kwargs)
        finally:
            self.replay_unknown_ = getattr(reg, "replay_unknown_", 0)

    def predict_neighbors(self, idx, dist=None, **kwargs):
        """:meth:`predict_neighbors_chunks` on one tile of stored neighbours, through the same path."""
        return self.predict_neighbors_chunks([idx if dist is None else (dist, idx)], **kwargs)

    def bootstrap_neighbors_chunks(self, neighbor_tiles, bootstrap, **kwargs):
        """Bootstrap planes from STORED neighbours (:meth:`RawKNNRegressor.bootstrap_neighbors_chunks`, with its keywords);
        nothing is transformed and nothing is searched, and the transform stays the one fitted on all plots."""
        check_is_fitted(self, "regressor_")
        reg = self.regressor_
        try:
            return reg.bootstrap_neighbors_chunks(neighbor_tiles, bootstrap, **kwargs)
        finally:
            self.replay_unknown_ = getattr(reg, "replay_unknown_", 0)

    def bootstrap_neighbors(self, idx, dist=None, *, bootstrap, **kwargs):
        """:meth:`bootstrap_neighbors_chunks` on one tile of stored neighbours, through the same path."""
        return self.bootstrap_neighbors_chunks([idx if dist is None else (dist, idx)], bootstrap, **kwargs)

    def score(self, X, y):
        """REF _base.py:350-352."""
        pred = self.predict(X)
        if is_torch_cuda_tensor(pred):
            pred = pred.cpu().numpy()
        return float(r2_score(y, pred))

    def __sklearn_tags__(self):
        tags = super().__sklearn_tags__()  # (as REF _base.py:354-358: a plain BaseEstimator that rejects sparse input)
        tags.input_tags.sparse = False
        return tags


class YFitMixin(TransformedKNeighborsRegressor):
    """Optional ``y_fit`` that only the transformer sees (REF _base.py:361-374)."""

    def _set_fitted_transformer(self, X, y) -> None:
        y_fit = self.y_fit_ if self.y_fit_ is not None else y
        self.transformer_ = self._get_transformer().fit(X, y_fit)

    def fit(self, X, y, y_fit=None):
        self.y_fit_ = y_fit
        return super().fit(X, y)


class OrdinationKNeighborsRegressor(TransformedKNeighborsRegressor, ABC):
    """Transformed regressors with an ``n_components`` knob (REF _base.py:377-408)."""

    def __init__(self, n_neighbors=5, *, n_components=None, weights="uniform", algorithm="auto",
                 leaf_size=30, p=2, metric="minkowski", metric_params=None, n_jobs=None):
        super().__init__(n_neighbors=n_neighbors, weights=weights, algorithm=algorithm,
                         leaf_size=leaf_size, p=p, metric=metric, metric_params=metric_params,
                         n_jobs=n_jobs)
        self.n_components = n_components


__all__ = [
    "RawKNNRegressor",
    "TransformedKNeighborsRegressor",
    "YFitMixin",
    "OrdinationKNeighborsRegressor",
    "NotFittedError",
]
