"""Device engine behind the estimators: one :class:`KNNEngine` per fitted regressor.

It owns the native index handle (reference rows, targets and the query-time affine map
resident in HBM) and moves queries/results as numpy arrays (staged through PCIe by the
library) or as PyTorch-ROCm CUDA tensors (zero copy, launched on torch's current stream).
All arithmetic happens in ``libsknnr_hip.so``; nothing here computes distances.
"""

from __future__ import annotations

import os

import numpy as np

from . import _native
from .weights import DistanceWeights

__all__ = ["KNNEngine", "default_device", "set_default_device", "is_torch_cuda_tensor"]

_default_device: int | None = None


def set_default_device(index: int | None) -> None:
    """Pin new engines to HIP device ``index`` (None = follow LOCAL_RANK / torch)."""
    global _default_device
    _default_device = index


def default_device() -> int:
    """Device for new engines: explicit override, else LOCAL_RANK (one process per GPU
    under ``torch.distributed.run``), else torch's current device, else 0."""
    if _default_device is not None:
        return _default_device
    import torch

    if torch.cuda.is_available():
        n = torch.cuda.device_count()
        if "LOCAL_RANK" in os.environ and n > 0:
            return int(os.environ["LOCAL_RANK"]) % n
        return torch.cuda.current_device()
    return 0


def is_torch_cuda_tensor(x) -> bool:
    mod = type(x).__module__
    return mod.startswith("torch") and hasattr(x, "is_cuda") and bool(x.is_cuda)


_WEIGHT_MODES = {"uniform": _native.WEIGHTS_UNIFORM, None: _native.WEIGHTS_UNIFORM,
                 "distance": _native.WEIGHTS_DISTANCE}


class KNNEngine:
    """HBM-resident kNN index + the kneighbors / predict launches.

    Parameters
    ----------
    fit_X : (n_ref, d) float64, the *transformed* reference rows (the reference's ``_fit_X``)
    y : (n_ref, t) targets or None
    target_dtype : dtype of the caller's targets when they were narrower than ``y`` (default: ``y``'s).  float32
        targets are reduced as numpy reduces them: the uniform mean in binary32, returned as float32
        (SKL/neighbors/_regression.py:254-255 keeps the dtype of ``_y``); other dtypes give float64.
    """

    def __init__(self, fit_X, y=None, device: int | None = None, target_dtype=None):
        self.device = default_device() if device is None else int(device)
        self._index = _native.Index(fit_X, y, device=self.device)
        self.n_ref = self._index.n_ref
        self.d = self._index.d
        self.t = self._index.t
        if target_dtype is None and y is not None:
            target_dtype = np.asarray(y).dtype
        self.y32 = target_dtype is not None and np.dtype(target_dtype) == np.float32
        self.d_in = self.d
        self.has_affine = False
        self.has_forest = False
        self._law_key = None  # (law code, p0, p1) the handle holds: weight_law()
        self._group_codes = None  # the group codes the handle holds: set_groups()
        self._buffer = None  # (positions, radius) the handle holds: set_buffer()

    def close(self):
        self._index.close()

    def set_affine(self, d_in, center=None, scale=None, proj=None):
        self._index.set_affine(int(d_in), center, scale, proj)
        self.d_in = int(d_in)
        self.has_affine = True

    def set_hamming_weights(self, w):
        """Per-column weights of the weighted-Hamming search over tree node ids (``formula="hamming"``)."""
        self._index.set_hamming_weights(w)

    def set_forest(self, image):
        """Install the query-time forest map: ``image`` as ``TreeNodeTransformer.forest_image()`` returns it.  Hamming
        calls with ``apply_affine=True`` then take raw feature rows and map them through the forests on the device."""
        self._index.set_forest(image["d_in"], image["tree_offset"], image["threshold"], image["feature"],
                               image["left"], image["right"])
        self.d_in = int(image["d_in"])
        self.has_forest = True

    def forest_apply(self, X):
        """Node ids ``(nq, n_trees)`` float64 of the raw rows ``X`` (numpy -> numpy, torch.cuda -> torch.cuda)."""
        if is_torch_cuda_tensor(X):
            import torch

            qdt = _native.dtype_code(X.dtype) or 0
            X = self._as_device_rows(X, True, qdt)
            out = torch.empty((X.shape[0], self.d), dtype=torch.float64, device=X.device)
            if X.shape[0]:
                torch.cuda.current_stream(X.device).synchronize()  # (the call runs on the default stream)
                self._index.forest_apply_device(X.data_ptr(), X.shape[0], qdt, out.data_ptr())
            return out
        qdt = _native.dtype_code(X.dtype) or 0
        X = np.ascontiguousarray(X) if qdt else np.ascontiguousarray(X, dtype=np.float64)
        self._check_columns(X, True)
        return self._index.forest_apply_host(X, qdt)

    def stats(self) -> dict:
        return self._index.stats()

    def reset_stats(self):
        self._index.reset_stats()

    # ------------------------------------------------------------------------------------
    def _opts(self, k, *, exclude_self, deterministic, decimals, formula, apply_affine,
              weight_mode=_native.WEIGHTS_UNIFORM, row_offset=0, check_finite=False, query_dtype=0, weight_law=0):
        return self._index.make_opts(
            k, exclude_self=exclude_self, deterministic=deterministic, decimals=decimals,
            formula={"direct": _native.FORMULA_DIRECT, "hamming": _native.FORMULA_HAMMING}.get(
                formula, _native.FORMULA_EXPANDED),
            apply_affine=apply_affine, weight_mode=weight_mode, row_offset=row_offset,
            check_finite=check_finite, query_dtype=query_dtype, weight_law=weight_law)

    def query_dtype_code(self, X, formula="expanded", apply_affine=False) -> int:
        """The sknnr_dtype under which the rows of ``X`` can be handed to the library as they are (float32, int16, uint16,
        uint8, int32: widened by the kernel that reads them, exactly), or 0 = float64 (convert first): narrow rows need
        the MFMA envelope (d <= 128) and a Euclidean formula, or the forest map (Hamming with ``apply_affine``)."""
        if X is None:
            return 0
        if formula == "hamming":
            return (_native.dtype_code(X.dtype) or 0) if apply_affine and self.has_forest else 0
        if self.d > 128:
            return 0
        return _native.dtype_code(X.dtype) or 0

    def _as_device_rows(self, X, apply_affine, query_dtype=0):
        """A contiguous CUDA tensor on the engine's device with the expected columns: float64, or the narrower element
        type ``query_dtype`` names (then left as it is)."""
        import torch

        if (query_dtype == 0 and X.dtype != torch.float64) or not X.is_contiguous():
            X = (X if query_dtype else X.to(torch.float64)).contiguous()
        if X.device.index != self.device:
            raise ValueError(f"X is on cuda:{X.device.index}, the engine on cuda:{self.device}")
        self._check_columns(X, apply_affine)
        return X

    def _check_columns(self, X, apply_affine):
        want = self.d_in if apply_affine else self.d
        if X.shape[1] != want:
            raise ValueError(f"X has {X.shape[1]} features, the engine expects {want}")

    def kneighbors(self, X, k, *, exclude_self=False, deterministic=True, decimals=10,
                   formula="expanded", apply_affine=False, row_offset=0, n_self_rows=None,
                   return_distance=True, out=None, check_finite=False, nodata=None, fill_index=-1):
        """Neighbours of the rows of ``X`` (numpy -> numpy, torch.cuda -> torch.cuda), or of
        the reference rows ``[row_offset, row_offset + n_self_rows)`` when ``X`` is None.
        ``out=(dist, idx)``: contiguous float64 / int64 CUDA tensors of shape ``(nq, k)`` to write
        into (torch.cuda input only), e.g. this rank's slot of an all-gather buffer.
        ``check_finite``: the kernels that read ``X`` also test it for NaN / infinity and the call
        raises ``HipBackendError(ERR_NONFINITE)`` (for CUDA tensors this synchronises the stream).
        ``nodata`` (float64, one value per column of ``X``; NaN: "is NaN"): rows holding a nodata value are masked on the
        device -- they get ``fill_index`` / NaN and cost no search -- and the others are answered as ``X[valid]`` would
        be (for CUDA tensors the stream is synchronised once, to read the valid count)."""
        if nodata is not None:
            if X is None:
                raise ValueError("nodata needs query rows: X=None has none")
            nodata = np.ascontiguousarray(nodata, dtype=np.float64).reshape(-1)
            if nodata.size != X.shape[1]:
                raise ValueError(f"nodata must hold one value per column of X ({X.shape[1]}), got {nodata.size}")
        qdt = self.query_dtype_code(X, formula, apply_affine)
        opts = self._opts(k, exclude_self=exclude_self, deterministic=deterministic,
                          decimals=decimals, formula=formula,
                          apply_affine=apply_affine and X is not None, row_offset=row_offset,
                          check_finite=check_finite and X is not None, query_dtype=qdt)
        if X is None:
            if not exclude_self:
                raise ValueError("X=None requires exclude_self=True")
            nq = self.n_ref - row_offset if n_self_rows is None else int(n_self_rows)
            return self._index.kneighbors_host(None, opts, nq=nq, return_distance=return_distance)
        if is_torch_cuda_tensor(X):
            import torch

            X = self._as_device_rows(X, apply_affine, qdt)
            nq = X.shape[0]
            if out is not None:
                dist, idx = out
                for t_, dt_ in ((dist, torch.float64), (idx, torch.int64)):
                    if t_ is None:
                        continue
                    if (tuple(t_.shape) != (nq, k) or t_.dtype != dt_ or not t_.is_contiguous()
                            or t_.device != X.device):
                        raise ValueError(f"out tensors must be contiguous ({nq}, {k}) {dt_} on {X.device}")
                if idx is None:
                    raise ValueError("out needs an index tensor")
            else:
                idx = torch.empty((nq, k), dtype=torch.int64, device=X.device)
                dist = torch.empty((nq, k), dtype=torch.float64, device=X.device) if return_distance else None
            if nq:
                stream = torch.cuda.current_stream(X.device).cuda_stream
                if nodata is not None:
                    self._index.kneighbors_masked_device(X.data_ptr(), nq, opts, nodata, fill_index,
                                                         dist.data_ptr() if dist is not None else 0, idx.data_ptr(), stream)
                else:
                    self._index.kneighbors_device(X.data_ptr(), nq, opts,
                                                  dist.data_ptr() if dist is not None else 0,
                                                  idx.data_ptr(), stream)
                if check_finite:
                    self._index.check_finite(stream)
            return dist, idx
        if out is not None:
            raise ValueError("out= is only supported for torch.cuda inputs")
        X = np.ascontiguousarray(X) if qdt else np.ascontiguousarray(X, dtype=np.float64)
        self._check_columns(X, apply_affine)
        if nodata is not None:
            return self._index.kneighbors_masked_host(X, opts, nodata, fill_index, return_distance=return_distance)[:2]
        return self._index.kneighbors_host(X, opts, return_distance=return_distance)

    def set_groups(self, codes):
        """The group code of every reference row for :meth:`kneighbors_grouped` (``n_ref`` integers >= 0, ``None``
        clears).  The engine keeps the last codes it uploaded and uploads again only when they change."""
        if codes is None:
            if self._group_codes is not None:
                self._index.set_groups(None)
                self._group_codes = None
            return
        codes = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        if self._group_codes is not None and np.array_equal(codes, self._group_codes):
            return
        self._index.set_groups(codes)
        self._group_codes = codes.copy()

    def set_buffer(self, buffer):
        """The ``(coords, radius)`` of a buffered :meth:`kneighbors_grouped` -- ``(n_ref, c)`` float64 positions, ``c`` 1
        to 3, and a float radius -- or ``None``, which clears a buffer left by an earlier call.  The engine keeps what
        it uploaded last and uploads again only when positions or radius change."""
        if buffer is None:
            if self._buffer is not None:
                self._index.set_buffer(None)
                self._buffer = None
            return
        coords, radius = buffer
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        radius = float(radius)
        if self._buffer is not None and radius == self._buffer[1] and np.array_equal(coords, self._buffer[0]):
            return
        self._index.set_buffer(coords, radius)
        self._buffer = (coords.copy(), radius)

    def buffer_counts(self):
        """``excluded[]`` under the masks of :meth:`set_groups` / :meth:`set_buffer`: int64 ``(n_ref,)``."""
        return self._index.buffer_counts()

    def debug_last_buffer(self) -> dict:
        return self._index.debug_last_buffer()

    def kneighbors_grouped(self, k, *, deterministic, decimals, formula, row_offset=0, n_rows=None, return_distance=True):
        """Leave-group-out neighbours of the reference rows ``[row_offset, row_offset + n_rows)`` under the codes of
        :meth:`set_groups`: per row the ``k`` rows of other groups smallest by (value, index) under ``formula``, the
        square root (not for Hamming), and sknnr's reorder with ``deterministic``.  Exact ties at the k-th value go to the
        lower index; scikit-learn's heap history is not replayed.  Numpy out: ``(dist or None, idx)``."""
        code = {"direct": _native.FORMULA_DIRECT, "hamming": _native.FORMULA_HAMMING}.get(formula, _native.FORMULA_EXPANDED)
        return self._index.kneighbors_grouped(k, deterministic=deterministic, decimals=decimals, formula=code,
                                              row_offset=row_offset, n_rows=n_rows, return_distance=return_distance)

    def debug_last_grouped(self) -> dict:
        return self._index.debug_last_grouped()

    def weight_mode(self, weights, w32=False) -> int:
        """The native weight mode of a ``uniform`` / ``distance`` / explicit (``"explicit"``) reduction, with the
        flags that make it reduce in the dtypes numpy would: float32 targets, float32 explicit weights ``w32``."""
        mode = _native.WEIGHTS_EXPLICIT if weights == "explicit" else _WEIGHT_MODES[weights]
        if self.y32:
            mode |= _native.WEIGHTS_F32_TARGETS
        if w32:
            mode |= _native.WEIGHTS_F32_WEIGHTS
        return mode

    def weight_law(self, weights) -> int:
        """The native code of a :class:`sknnr_amd.weights.DistanceWeights` instance -- its parameters are then on the
        handle (uploaded when they change) and a call made with ``weight_mode("explicit")`` and this code evaluates the
        law on the device -- or 0 for anything else (strings, plain callables)."""
        if not isinstance(weights, DistanceWeights):
            return 0
        key = (weights.code, *weights.params)
        if key != self._law_key:
            self._index.set_weight_law_params(*key)
            self._law_key = key
        return weights.code

    def pred_dtype(self, weights):
        """scikit-learn's result dtype: the float32 targets' own under uniform weights, else float64."""
        return np.float32 if self.y32 and weights in (None, "uniform") else np.float64

    def predict_from_neighbors(self, dist, idx, weights="uniform"):
        """The reduction alone on neighbours already found: ``(dist, idx)`` numpy -> numpy or torch.cuda -> torch.cuda,
        ``weights`` as in :meth:`predict` (a callable runs on the host, or on the tensors it is given)."""
        if self.t < 1:
            raise ValueError("the engine was built without targets")
        k = idx.shape[1]
        w, w32 = None, False
        if callable(weights):
            w = weights(dist)
            if not hasattr(w, "dtype"):
                w = np.asarray(w)
            w32 = str(getattr(w, "dtype", "")) in ("float32", "torch.float32")
            if tuple(w.shape) != tuple(dist.shape):
                raise ValueError("the weights callable must return an array shaped like its input")
            mode = self.weight_mode("explicit", w32)
        elif weights in _WEIGHT_MODES:
            mode = self.weight_mode(weights)
        else:
            raise ValueError(f"weights not recognized: should be 'uniform', 'distance', or a callable; got {weights!r}")
        out_dtype = np.float64 if w is not None else self.pred_dtype(weights)
        if is_torch_cuda_tensor(idx):
            import torch

            idx = idx.to(torch.int64).contiguous()
            dist = None if dist is None else dist.to(torch.float64).contiguous()
            if w is not None:
                w = torch.as_tensor(w, device=idx.device).to(torch.float64).contiguous()
            pred = torch.empty((idx.shape[0], self.t), dtype=torch.float64, device=idx.device)
            if idx.shape[0]:
                stream = torch.cuda.current_stream(idx.device).cuda_stream
                self._index.predict_from_neighbors_device(0 if dist is None else dist.data_ptr(), idx.data_ptr(),
                                                          0 if w is None else w.data_ptr(), idx.shape[0], k, mode,
                                                          pred.data_ptr(), stream)
            return pred if out_dtype == np.float64 else pred.to(torch.float32)
        w = None if w is None else np.asarray(w, dtype=np.float64)
        pred = self._index.predict_from_neighbors_host(dist, idx, w, mode)
        return pred if out_dtype == np.float64 else pred.astype(np.float32)

    def tally_from_neighbors(self, dist, idx):
        """Neighbour usage of neighbours already found (sknnr_tally_from_neighbors): ``(counts, max_dist)`` as host arrays,
        ``(n_ref, k)`` int64 and ``(n_ref,)`` float64 (0.0 where a row was never used), from numpy or torch.cuda
        ``(dist, idx)``."""
        if is_torch_cuda_tensor(idx):
            import torch

            idx = idx.to(torch.int64).contiguous()
            dist = dist.to(torch.float64).contiguous()
            nq, k = idx.shape
            counts = torch.empty((self._index.n_ref, k), dtype=torch.int64, device=idx.device)
            max_dist = torch.empty((self._index.n_ref,), dtype=torch.float64, device=idx.device)
            stream = torch.cuda.current_stream(idx.device)
            self._index.tally_from_neighbors_device(dist.data_ptr(), idx.data_ptr(), nq, k, counts.data_ptr(),
                                                    max_dist.data_ptr(), False, stream.cuda_stream)
            stream.synchronize()
            return counts.cpu().numpy(), max_dist.cpu().numpy()
        return self._index.tally_from_neighbors_host(dist, idx)

    def zonal_from_values(self, values, zones, dtype, n_zones, scale=None, offset=None, n_classes=None):
        """Zonal accumulators of values already computed (sknnr_zonal_from_values): ``values`` ``(n, c)`` float64 and
        ``zones`` ``(n,)`` int32, numpy or torch.cuda; the sums are over the stored values of ``dtype`` (int16, uint16,
        uint8 or int32) under ``scale`` / ``offset`` (host arrays, one value per column, or neither).  ``n_classes``: one
        class count per column (0: numeric), or None.  Returns host arrays ``(acc, hist)``: ``(n_zones, c, 6)`` int64 and
        the flat class blocks (None when no column has classes)."""
        if is_torch_cuda_tensor(values):
            import torch

            values = values.to(torch.float64).contiguous()
            zones = zones.to(device=values.device, dtype=torch.int32).contiguous().reshape(-1)
            n, c = values.shape
            if zones.numel() != n:
                raise ValueError(f"zones must hold one code per pixel ({n}), got {zones.numel()}")
            cls, per_zone = _native._zonal_classes(n_classes, c)
            acc = torch.empty((int(n_zones), c, _native.ZONAL_FIELDS), dtype=torch.int64, device=values.device)
            hist = torch.empty((int(n_zones) * per_zone,), dtype=torch.int64, device=values.device) if per_zone else None
            stream = torch.cuda.current_stream(values.device)
            self._index.zonal_from_values_device(values.data_ptr(), zones.data_ptr(), n, c, np.dtype(dtype), n_zones,
                                                 acc.data_ptr(), hist.data_ptr() if per_zone else 0, scale=scale,
                                                 offset=offset, n_classes=cls, accumulate=False,
                                                 stream=stream.cuda_stream)
            stream.synchronize()
            return acc.cpu().numpy(), hist.cpu().numpy() if per_zone else None
        return self._index.zonal_from_values_host(values, zones, dtype, n_zones, scale=scale, offset=offset,
                                                  n_classes=n_classes)

    def domain_from_neighbors(self, dist, table, rank=1, threshold=None):
        """Distance-domain codes of distances already found (sknnr_domain_from_neighbors): ``dist`` ``(nq, k)`` numpy or
        torch.cuda, ``table`` the sorted host table.  Returns host arrays ``(codes, acc)``: ``(nq,)`` uint8 and the 103
        int64 accumulators."""
        if is_torch_cuda_tensor(dist):
            import torch

            dist = dist.to(torch.float64).contiguous()
            nq, k = dist.shape
            codes = torch.empty((nq,), dtype=torch.uint8, device=dist.device)
            acc = torch.empty((_native.DOMAIN_ACC,), dtype=torch.int64, device=dist.device)
            stream = torch.cuda.current_stream(dist.device)
            self._index.domain_from_neighbors_device(dist.data_ptr(), nq, k, table, rank, threshold, codes.data_ptr(),
                                                     acc.data_ptr(), False, stream.cuda_stream)
            stream.synchronize()
            return codes.cpu().numpy(), acc.cpu().numpy()
        return self._index.domain_from_neighbors_host(dist, table, rank, threshold)

    def summarize_from_neighbors(self, dist, idx, weights, stat):
        """Per-target statistics (``stat``: one ``_native.STATISTICS`` code per target) of neighbours already found:
        :meth:`predict_from_neighbors` with the mean replaced column by column.  Always float64 ``(nq, t)``.  Explicit
        weights that are negative or not finite are refused."""
        return self._summarize_from_neighbors(dist, idx, weights, stat, None)

    def summarize_plan_from_neighbors(self, dist, idx, weights, plan):
        """An output plan (``plan``: ``(cols, codes, params)`` as :func:`sknnr_amd._base.normalize_outputs` gives them) of
        neighbours already found: :meth:`summarize_from_neighbors` with ``n_out`` planes, each one statistic of one target.
        Always float64 ``(nq, n_out)``; the same refusal of negative or non-finite explicit weights."""
        return self._summarize_from_neighbors(dist, idx, weights, None, plan)

    def _summarize_from_neighbors(self, dist, idx, weights, stat, plan):
        if self.t < 1:
            raise ValueError("the engine was built without targets")
        k = idx.shape[1]
        w = None
        cuda = is_torch_cuda_tensor(idx)
        if callable(weights):
            w = weights(dist)
            if not hasattr(w, "dtype"):
                w = np.asarray(w)
            w32 = str(getattr(w, "dtype", "")) in ("float32", "torch.float32")
            if tuple(w.shape) != tuple(dist.shape):
                raise ValueError("the weights callable must return an array shaped like its input")
            if is_torch_cuda_tensor(w):
                bad = bool(((w < 0) | ~w.isfinite()).any())
            else:
                wh = np.asarray(w)
                bad = bool(np.any(wh < 0) or not np.all(np.isfinite(wh)))
            if bad:
                raise ValueError("the weights callable returned negative or non-finite weights: the neighbour summaries "
                                 "are defined for finite weights >= 0")
            mode = self.weight_mode("explicit", w32)
        elif weights in _WEIGHT_MODES:
            mode = self.weight_mode(weights)
        else:
            raise ValueError(f"weights not recognized: should be 'uniform', 'distance', or a callable; got {weights!r}")
        if cuda:
            import torch

            idx = idx.to(torch.int64).contiguous()
            dist = None if dist is None else dist.to(torch.float64).contiguous()
            if w is not None:
                w = torch.as_tensor(w, device=idx.device).to(torch.float64).contiguous()
            width = self.t if plan is None else len(plan[0])
            out = torch.empty((idx.shape[0], width), dtype=torch.float64, device=idx.device)
            if idx.shape[0]:
                stream = torch.cuda.current_stream(idx.device).cuda_stream
                args = (0 if dist is None else dist.data_ptr(), idx.data_ptr(), 0 if w is None else w.data_ptr(),
                        idx.shape[0], k, mode)
                if plan is None:
                    self._index.summarize_from_neighbors_device(*args, stat, out.data_ptr(), stream)
                else:
                    self._index.summarize_plan_from_neighbors_device(*args, plan, out.data_ptr(), stream)
            return out
        w = None if w is None else np.asarray(w, dtype=np.float64)
        if plan is not None:
            return self._index.summarize_plan_from_neighbors_host(dist, idx, w, mode, plan)
        return self._index.summarize_from_neighbors_host(dist, idx, w, mode, stat)

    def summarize(self, X, k, weights, stat, *, exclude_self=False, deterministic=True, decimals=10,
                  formula="expanded", apply_affine=False, row_offset=0, n_self_rows=None, check_finite=False):
        """Search plus per-target statistics: :meth:`predict` with ``stat`` (one ``_native.STATISTICS`` code per target)
        choosing what is reduced from the neighbours.  Always float64 ``(nq, t)``."""
        return self._summarize(X, k, weights, stat, None, exclude_self=exclude_self, deterministic=deterministic,
                               decimals=decimals, formula=formula, apply_affine=apply_affine, row_offset=row_offset,
                               n_self_rows=n_self_rows, check_finite=check_finite)

    def summarize_plan(self, X, k, weights, plan, *, exclude_self=False, deterministic=True, decimals=10,
                       formula="expanded", apply_affine=False, row_offset=0, n_self_rows=None, check_finite=False):
        """Search plus output plan: :meth:`summarize` with ``n_out`` planes ``(cols, codes, params)``, all reduced behind
        the one search.  Always float64 ``(nq, n_out)``."""
        return self._summarize(X, k, weights, None, plan, exclude_self=exclude_self, deterministic=deterministic,
                               decimals=decimals, formula=formula, apply_affine=apply_affine, row_offset=row_offset,
                               n_self_rows=n_self_rows, check_finite=check_finite)

    def _summarize(self, X, k, weights, stat, plan, *, exclude_self, deterministic, decimals, formula, apply_affine,
                   row_offset, n_self_rows, check_finite):
        if self.t < 1:
            raise ValueError("the engine was built without targets")
        law = self.weight_law(weights)  # (a distance-weight law: the device evaluates it, in the single call below)
        if callable(weights) and not law:  # (as predict: the callable maps the distances to weights on the host)
            dist, idx = self.kneighbors(X, k, exclude_self=exclude_self, deterministic=deterministic,
                                        decimals=decimals, formula=formula, apply_affine=apply_affine,
                                        row_offset=row_offset, n_self_rows=n_self_rows, check_finite=check_finite)
            return self._summarize_from_neighbors(dist, idx, weights, stat, plan)
        if not law and weights not in _WEIGHT_MODES:
            raise ValueError(f"weights not recognized: should be 'uniform', 'distance', or a callable; got {weights!r}")
        qdt = self.query_dtype_code(X, formula, apply_affine)
        opts = self._opts(k, exclude_self=exclude_self, deterministic=deterministic, decimals=decimals,
                          formula=formula, apply_affine=apply_affine and X is not None,
                          weight_mode=self.weight_mode("explicit" if law else weights), row_offset=row_offset,
                          check_finite=check_finite and X is not None, query_dtype=qdt, weight_law=law)
        if X is None:
            nq = self.n_ref - row_offset if n_self_rows is None else int(n_self_rows)
            if plan is not None:
                return self._index.summarize_plan_host(None, opts, plan, nq=nq)
            return self._index.summarize_host(None, opts, stat, nq=nq)
        if is_torch_cuda_tensor(X):
            import torch

            X = self._as_device_rows(X, apply_affine, qdt)
            nq = X.shape[0]
            out = torch.empty((nq, self.t if plan is None else len(plan[0])), dtype=torch.float64, device=X.device)
            if nq:
                stream = torch.cuda.current_stream(X.device).cuda_stream
                if plan is None:
                    self._index.summarize_device(X.data_ptr(), nq, opts, stat, out.data_ptr(), stream)
                else:
                    self._index.summarize_plan_device(X.data_ptr(), nq, opts, plan, out.data_ptr(), stream)
                if check_finite:
                    self._index.check_finite(stream)
            return out
        X = np.ascontiguousarray(X) if qdt else np.ascontiguousarray(X, dtype=np.float64)
        self._check_columns(X, apply_affine)
        if plan is not None:
            return self._index.summarize_plan_host(X, opts, plan)
        return self._index.summarize_host(X, opts, stat)

    def predict(self, X, k, weights="uniform", *, exclude_self=False, deterministic=True, decimals=10,
                formula="expanded", apply_affine=False, row_offset=0, n_self_rows=None, check_finite=False,
                nodata=None):
        """Weighted multi-output mean of the neighbours' targets, in the dtype scikit-learn returns
        (:meth:`pred_dtype`).  ``nodata`` as in :meth:`kneighbors`: masked rows are predicted NaN.  ``weights``:
        ``"uniform"``, ``"distance"``, a :class:`sknnr_amd.weights.DistanceWeights` law (one device call: the law kernel
        makes the weights from the call's own distances) or any other callable (search, the callable on the host,
        reduction: three steps)."""
        if self.t < 1:
            raise ValueError("the engine was built without targets")
        if nodata is not None:
            if X is None:
                raise ValueError("nodata needs query rows: X=None has none")
            if callable(weights) and not isinstance(weights, DistanceWeights):
                raise NotImplementedError("nodata is not supported with callable weights")
            nodata = np.ascontiguousarray(nodata, dtype=np.float64).reshape(-1)
            if nodata.size != X.shape[1]:
                raise ValueError(f"nodata must hold one value per column of X ({X.shape[1]}), got {nodata.size}")
        law = self.weight_law(weights)  # (a distance-weight law: the device evaluates it, in the single call below)
        if callable(weights) and not law:
            # A Python callable cannot run on the device: find the neighbours on the GPU, let
            # the callable map the (nq, k) distances to weights on the host, reduce on the GPU.
            dist, idx = self.kneighbors(X, k, exclude_self=exclude_self, deterministic=deterministic,
                                        decimals=decimals, formula=formula, apply_affine=apply_affine,
                                        row_offset=row_offset, n_self_rows=n_self_rows, check_finite=check_finite)
            return self.predict_from_neighbors(dist, idx, weights)
        if not law and weights not in _WEIGHT_MODES:
            raise ValueError(f"weights not recognized: should be 'uniform', 'distance', or a callable; got {weights!r}")
        mode = self.weight_mode("explicit" if law else weights)
        to32 = self.pred_dtype(weights) == np.float32  # (a law's result is float64, as any callable's)
        qdt = self.query_dtype_code(X, formula, apply_affine)
        opts = self._opts(k, exclude_self=exclude_self, deterministic=deterministic, decimals=decimals,
                          formula=formula, apply_affine=apply_affine and X is not None,
                          weight_mode=mode, row_offset=row_offset, check_finite=check_finite and X is not None,
                          query_dtype=qdt, weight_law=law)
        if X is None:
            nq = self.n_ref - row_offset if n_self_rows is None else int(n_self_rows)
            pred = self._index.predict_host(None, opts, nq=nq)
            return pred.astype(np.float32) if to32 else pred
        if is_torch_cuda_tensor(X):
            import torch

            X = self._as_device_rows(X, apply_affine, qdt)
            nq = X.shape[0]
            pred = torch.empty((nq, self.t), dtype=torch.float64, device=X.device)
            if nq:
                stream = torch.cuda.current_stream(X.device).cuda_stream
                if nodata is not None:
                    self._index.predict_masked_device(X.data_ptr(), nq, opts, nodata, -1, pred.data_ptr(), 0, 0, stream)
                else:
                    self._index.predict_device(X.data_ptr(), nq, opts, pred.data_ptr(), 0, 0, stream)
                if check_finite:
                    self._index.check_finite(stream)
            return pred.to(torch.float32) if to32 else pred
        X = np.ascontiguousarray(X) if qdt else np.ascontiguousarray(X, dtype=np.float64)
        self._check_columns(X, apply_affine)
        pred = self._index.predict_masked_host(X, opts, nodata)[0] if nodata is not None else self._index.predict_host(X, opts)
        return pred.astype(np.float32) if to32 else pred

    # ---- reference-sharded search (sknnr_amd.distributed.RefShardedKNN) ------------------------------------
    def shard_candidates(self, X, kk, *, formula="expanded", apply_affine=False, index_offset=0, check_finite=False):
        """This engine's rows are one SHARD of a reference set: the ``kk`` nearest of them for every row of ``X`` as raw
        candidates -- values of the formula (squared distances) ascending by (value, index), indices +
        ``index_offset`` -- numpy in / numpy out or torch.cuda in / torch.cuda out."""
        opts = self._opts(kk, exclude_self=False, deterministic=False, decimals=10, formula=formula,
                          apply_affine=apply_affine, check_finite=check_finite)
        if is_torch_cuda_tensor(X):
            import torch

            X = self._as_device_rows(X, apply_affine)
            nq = X.shape[0]
            val = torch.empty((nq, kk), dtype=torch.float64, device=X.device)
            idx = torch.empty((nq, kk), dtype=torch.int64, device=X.device)
            if nq:
                stream = torch.cuda.current_stream(X.device).cuda_stream
                self._index.shard_candidates_device(X.data_ptr(), nq, opts, index_offset, val.data_ptr(), idx.data_ptr(), stream)
                if check_finite:
                    self._index.check_finite(stream)
            return val, idx
        X = np.ascontiguousarray(X, dtype=np.float64)
        self._check_columns(X, apply_affine)
        return self._index.shard_candidates_host(X, opts, index_offset)

    def merge_shards(self, X, k, shard_val, shard_idx, *, exclude_self=False, deterministic=True, decimals=10,
                     formula="expanded", apply_affine=False, row_offset=0, n_self_rows=None):
        """Merge the gathered candidates ``(n_shards, nq, k + exclude_self)`` of all shards into the call's final
        ``(dist, idx)``; this engine holds ALL reference rows and re-scans the rows whose merged answer is not unique."""
        opts = self._opts(k, exclude_self=exclude_self, deterministic=deterministic, decimals=decimals, formula=formula,
                          apply_affine=apply_affine and X is not None, row_offset=row_offset)
        if is_torch_cuda_tensor(shard_val):
            import torch

            n_shards, nq = shard_val.shape[0], shard_val.shape[1]
            Xd = None if X is None else self._as_device_rows(X, apply_affine)
            dist = torch.empty((nq, k), dtype=torch.float64, device=shard_val.device)
            idx = torch.empty((nq, k), dtype=torch.int64, device=shard_val.device)
            sv, si = shard_val.contiguous(), shard_idx.contiguous()
            if nq:
                stream = torch.cuda.current_stream(shard_val.device).cuda_stream
                self._index.merge_shards_device(0 if Xd is None else Xd.data_ptr(), nq, opts, n_shards, sv.data_ptr(),
                                                si.data_ptr(), dist.data_ptr(), idx.data_ptr(), stream)
            return dist, idx
        nq = shard_val.shape[1] if X is None else None
        if X is not None:
            X = np.ascontiguousarray(X, dtype=np.float64)
            self._check_columns(X, apply_affine)
        return self._index.merge_shards_host(X, opts, shard_val, shard_idx, nq=nq)

    def open_stream(self, k, *, weights=None, want_dist=True, deterministic=True, decimals=10,
                    formula="expanded", apply_affine=False, row_offset=0, check_finite=False, query_dtype=0,
                    nodata=None, fill_index=-1, output=None, statistic=None, id_table=None, fill_id=-1, plan=None,
                    tally=False, zonal=None, domain=None, bootstrap=None):
        """A :class:`sknnr_amd._native.QueryStream` over host tiles: ``push(tile)`` keeps the PCIe
        pipeline full across tiles and carries the global row offset.  ``weights`` (``"uniform"`` /
        ``"distance"`` / a :class:`sknnr_amd.weights.DistanceWeights` law, evaluated on the device tile by tile) also
        asks for predictions: float64 arrays, holding binary32 values where
        :meth:`pred_dtype` is float32.  ``nodata`` (float64, one value per column of the tiles): every tile is masked on
        the device, masked rows get ``fill_index`` / NaN and the row offset counts valid rows only.  ``output``: keyword
        arguments of :meth:`sknnr_amd._native.QueryStream.set_output` (typed results, narrowed on the device).
        ``statistic``: one ``_native.STATISTICS`` code per target; the predictions become those summaries of the
        neighbours (:meth:`summarize`), written where the predictions are.  ``id_table`` (int64, one dataframe id per
        reference row): the indices leave as ``id_table[idx]``, looked up on the device; keep ``fill_index`` negative,
        and masked rows get ``fill_id``.  ``plan``: an output plan ``(cols, codes, params)`` instead of ``statistic``; the
        prediction lane then holds its ``n_out`` planes (:meth:`summarize_plan`).  ``tally``: every tile's neighbours are
        tallied on the device (:meth:`sknnr_amd._native.QueryStream.set_tally`); ``stream.tally()`` reads the result.
        ``zonal``: ``(n_zones, n_classes)`` -- every tile's predictions are tallied by zone on the device
        (:meth:`sknnr_amd._native.QueryStream.set_zonal`; the stream needs an integer ``pred_dtype``); every push then
        needs ``stream.next_zones(codes)`` first, and ``stream.zonal()`` reads the result.  ``domain``: ``(table, rank,
        threshold, mask_beyond)`` -- every tile's distances are coded against the table on the device
        (:meth:`sknnr_amd._native.QueryStream.set_domain`); ``stream.next_domain_out(plane)`` names where a push's codes go
        and ``stream.domain()`` reads the accumulators.  ``bootstrap``: ``(k, (cols, codes))`` -- the stream's reduction
        stage is the bootstrap of the table of :meth:`set_bootstrap` (``k`` of this call is then the number of candidates
        searched); ``stream.bootstrap()`` reads its tallies."""
        want_pred = weights is not None
        law = self.weight_law(weights)  # (a distance-weight law: every tile's weights are made on the device)
        if want_pred and not law and weights not in _WEIGHT_MODES:
            raise ValueError("a stream predicts with 'uniform' or 'distance' weights, or a sknnr_amd.weights law, only")
        opts = self._opts(k, exclude_self=False, deterministic=deterministic, decimals=decimals,
                          formula=formula, apply_affine=apply_affine,
                          weight_mode=(self.weight_mode("explicit" if law else weights) if want_pred
                                       else _native.WEIGHTS_UNIFORM),
                          row_offset=row_offset, check_finite=check_finite, query_dtype=query_dtype, weight_law=law)
        if statistic is not None and not want_pred:
            raise ValueError("statistics need a stream that predicts: pass weights")
        if plan is not None and not want_pred:
            raise ValueError("an output plan needs a stream that predicts: pass weights")
        if plan is not None and statistic is not None:
            raise ValueError("a stream takes statistic or an output plan, not both")
        return self._index.open_stream(opts, want_dist=want_dist, want_pred=want_pred, nodata=nodata, fill_index=fill_index,
                                       output=output, statistic=statistic, id_table=id_table, fill_id=fill_id, plan=plan,
                                       tally=tally, zonal=zonal, domain=domain, bootstrap=bootstrap)

    @classmethod
    def for_targets(cls, y, device: int | None = None, target_dtype=None):
        """An attribute-only engine: it owns the ``(n_ref, t)`` table ``y`` (:class:`sknnr_amd._native.TargetIndex`) and
        serves :meth:`open_replay` and the from-neighbours reductions; it has no reference rows and searches nothing."""
        self = cls.__new__(cls)
        self.device = default_device() if device is None else int(device)
        self._index = _native.TargetIndex(y, device=self.device)
        self.n_ref, self.d, self.t = self._index.n_ref, 0, self._index.t
        self.y32 = target_dtype is not None and np.dtype(target_dtype) == np.float32
        self.d_in = 0
        self.has_affine = self.has_forest = False
        self._law_key = self._group_codes = self._buffer = None
        return self

    def set_replay_ids(self, ids):
        """The int64 dataframe ids replay streams look stored ids up in (None: none); uploaded when they change."""
        key = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        held = getattr(self, "_replay_ids", None)
        if (key is None) != (held is None) or (key is not None and not np.array_equal(key, held)):
            self._index.set_replay_ids(key)
            self._replay_ids = key

    def open_replay(self, k, ks, *, weights=None, idx_dtype=np.int64, dist_dtype=None, fill_index=-1, ids=False,
                    want_dist=False, output=None, statistic=None, id_table=None, fill_id=-1, plan=None, tally=False,
                    zonal=None, domain=None, bootstrap=None):
        """A :class:`sknnr_amd._native.ReplayStream`: tiles of ``ks`` stored neighbour columns (``idx_dtype`` int32 /
        int64, ``dist_dtype`` float32 / float64 or None) in place of feature rows, the leading ``k`` in use; ``ids``:
        the stored values are ids of :meth:`set_replay_ids`.  Every other keyword as in :meth:`open_stream`."""
        want_pred = weights is not None
        law = self.weight_law(weights)
        if want_pred and not law and weights not in _WEIGHT_MODES:
            raise ValueError("a stream predicts with 'uniform' or 'distance' weights, or a sknnr_amd.weights law, only")
        if (statistic is not None or plan is not None) and not want_pred:
            raise ValueError("statistics and output plans need a stream that predicts: pass weights")
        if plan is not None and statistic is not None:
            raise ValueError("a stream takes statistic or an output plan, not both")
        mode = self.weight_mode("explicit" if law else weights) if want_pred else _native.WEIGHTS_UNIFORM
        stream = self._index.open_replay(k, ks, weight_mode=mode, weight_law=law, idx_dtype=idx_dtype, dist_dtype=dist_dtype,
                                         fill_index=fill_index, ids=ids, want_dist=want_dist, want_pred=want_pred)
        return stream.configure(output=output, statistic=statistic, id_table=id_table, fill_id=fill_id, plan=plan,
                                tally=tally, zonal=zonal, domain=domain, bootstrap=bootstrap)

    def set_bootstrap(self, table):
        """The uint8 ``(B, n_ref)`` multiplicity table of bootstrap reductions (None: none); uploaded when it changes."""
        held = getattr(self, "_boot_table", None)
        if table is held:
            return
        if table is None or held is None or not np.array_equal(table, held):
            self._index.set_bootstrap(table)
        self._boot_table = table

    def bootstrap_weights(self, weights):
        """``(weight_mode, weight_law)`` of a bootstrap reduction: always float64, uniform / distance / a device law."""
        law = self.weight_law(weights)
        if law:
            return _native.WEIGHTS_EXPLICIT, law
        if callable(weights) or weights not in _WEIGHT_MODES:
            raise ValueError("a bootstrap reduces with 'uniform' or 'distance' weights, or a sknnr_amd.weights law, only")
        return _WEIGHT_MODES[weights], 0

    def bootstrap_from_neighbors(self, dist, idx, k, weights, plan):
        """The bootstrap reduction (include/sknnr_hip.h, "Bootstrap") of ``(dist, idx)`` of ``kw`` columns with replicates of
        ``k`` copies, from the table of :meth:`set_bootstrap`: ``(out, tally)`` -- ``out`` float64 ``(nq, n_out)`` for the plan
        ``(cols, codes)``, numpy -> numpy or torch.cuda -> torch.cuda, and ``tally`` the int64 pair (pixels, valid replicates)."""
        if self.t < 1:
            raise ValueError("the engine was built without targets")
        mode, law = self.bootstrap_weights(weights)
        kw = idx.shape[1]
        if is_torch_cuda_tensor(idx):
            import torch

            idx = idx.to(torch.int64).contiguous()
            dist = None if dist is None else dist.to(torch.float64).contiguous()
            out = torch.empty((idx.shape[0], len(plan[0])), dtype=torch.float64, device=idx.device)
            tally = torch.zeros(2, dtype=torch.int64, device=idx.device)
            stream = torch.cuda.current_stream(idx.device).cuda_stream
            self._index.bootstrap_from_neighbors_device(0 if dist is None else dist.data_ptr(), idx.data_ptr(), idx.shape[0], kw,
                                                        k, plan, out.data_ptr(), tally.data_ptr(), mode, law, stream)
            return out, tally.cpu().numpy()
        return self._index.bootstrap_from_neighbors_host(dist, idx, k, plan, mode, law)

    def hamming_distances(self, X, rows=None):
        """Full weighted-Hamming distance rows of ``X[rows]`` (``X`` None: of the fitted rows) from the device."""
        return self._index.hamming_distances_host(X, rows)

    def crosswalk(self, idx, table):
        """``table[idx]`` for int64 dataframe ids (REF _base.py:177-180)."""
        if is_torch_cuda_tensor(idx):
            import torch

            tab = torch.as_tensor(np.ascontiguousarray(table, dtype=np.int64), device=idx.device)
            out = torch.empty_like(idx)
            stream = torch.cuda.current_stream(idx.device).cuda_stream
            _native.crosswalk_device(tab.data_ptr(), tab.numel(), idx.data_ptr(), idx.numel(),
                                     out.data_ptr(), self.device, stream)
            torch.cuda.current_stream(idx.device).synchronize()  # tab dies with this frame
            return out
        return _native.crosswalk_host(table, idx, self.device)
