"""ctypes binding of the C ABI in ``include/sknnr_hip.h``.

The HIP library is the only engine: there is no CPU fallback.  Loading fails loudly
when ``libsknnr_hip.so`` is missing (build it with ``python -m sknnr_amd._build``) and
every compute call fails loudly when no MI355X is visible.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int32, c_int64, c_void_p

import numpy as np

from . import _build

MEM_HOST = 0
MEM_DEVICE = 1
FORMULA_EXPANDED = 0
FORMULA_DIRECT = 1
FORMULA_HAMMING = 2
WEIGHTS_UNIFORM = 0
WEIGHTS_DISTANCE = 1
WEIGHTS_EXPLICIT = 2
# flag bits OR-ed into a weight mode (include/sknnr_hip.h): the dtype scikit-learn reduces in
WEIGHTS_F32_TARGETS = 0x100
WEIGHTS_F32_WEIGHTS = 0x200

# sknnr_statistic (include/sknnr_hip.h): the per-target summaries of the neighbours
STATISTICS = {"mean": 0, "mode": 1, "min": 2, "max": 3, "nearest": 4, "std": 5}
# the statistics of an output plan's entries: those, and SKNNR_STAT_QUANTILE with its parameter q.  (A table of its own:
# the per-target tables of sknnr_summarize* / sknnr_stream_set_statistics take the six names above only.)
PLAN_STATISTICS = {**STATISTICS, "quantile": 6}
PLAN_MAX_OUT = 1024

# sknnr_weight_law (include/sknnr_hip.h): the distance-weight laws the device evaluates, by the header's short names; the
# classes of sknnr_amd.weights carry theirs as ``name`` / ``code``
WEIGHT_LAWS = {"inverse": 1, "inverse_squared": 2, "triangular": 3, "epanechnikov": 4}
WEIGHT_LAW_NONE = 0

ERR_INVALID = -1
ERR_K_TOO_LARGE = -2
ERR_NO_TARGETS = -3
ERR_UNSUPPORTED = -4
ERR_HIP = -5
ERR_NO_DEVICE = -6
ERR_NONFINITE = -7
ABI_VERSION = 5

# sknnr_dtype (include/sknnr_hip.h): query rows narrower than float64 are widened by the kernel that reads them
DTYPE_CODES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int16): 2, np.dtype(np.uint16): 3,
               np.dtype(np.uint8): 4, np.dtype(np.int32): 5}


def dtype_code(dt) -> int | None:
    """The sknnr_dtype of a numpy / torch dtype, or None when the rows must be converted to float64 first."""
    try:
        return DTYPE_CODES.get(np.dtype(dt))
    except TypeError:  # a torch dtype
        name = str(dt).replace("torch.", "")
        try:
            return DTYPE_CODES.get(np.dtype(name))
        except TypeError:
            return None


# every symbol include/sknnr_hip.h declares (checked by tests/test_cabi.py)
EXPORTED_SYMBOLS = (
    "sknnr_device_count",
    "sknnr_abi_version",
    "sknnr_last_error",
    "sknnr_index_create",
    "sknnr_index_destroy",
    "sknnr_index_set_affine",
    "sknnr_index_set_hamming_weights",
    "sknnr_index_set_forest",
    "sknnr_forest_apply",
    "sknnr_affine_transform",
    "sknnr_index_set_weight_law_params",
    "sknnr_index_shape",
    "sknnr_get_stats",
    "sknnr_reset_stats",
    "sknnr_check_finite",
    "sknnr_kneighbors",
    "sknnr_predict",
    "sknnr_predict_from_neighbors",
    "sknnr_summarize_from_neighbors",
    "sknnr_summarize",
    "sknnr_stream_set_statistics",
    "sknnr_debug_last_summary",
    "sknnr_summarize_plan_from_neighbors",
    "sknnr_summarize_plan",
    "sknnr_stream_set_plan",
    "sknnr_debug_last_plan",
    "sknnr_debug_last_weight_law",
    "sknnr_debug_weight_law",
    "sknnr_hamming_distances",
    "sknnr_index_set_groups",
    "sknnr_kneighbors_grouped",
    "sknnr_debug_last_grouped",
    "sknnr_index_set_buffer",
    "sknnr_buffer_counts",
    "sknnr_debug_last_buffer",
    "sknnr_shard_candidates",
    "sknnr_merge_shards",
    "sknnr_stream_begin",
    "sknnr_stream_push",
    "sknnr_stream_flush",
    "sknnr_stream_end",
    "sknnr_mask_rows",
    "sknnr_kneighbors_masked",
    "sknnr_predict_masked",
    "sknnr_stream_set_nodata",
    "sknnr_stream_valid_rows",
    "sknnr_planes_to_rows",
    "sknnr_rows_to_planes",
    "sknnr_stream_push_planes",
    "sknnr_debug_last_planes",
    "sknnr_narrow",
    "sknnr_stream_set_output",
    "sknnr_narrow_ids",
    "sknnr_stream_set_id_table",
    "sknnr_stream_push_typed",
    "sknnr_stream_push_planes_typed",
    "sknnr_tally_from_neighbors",
    "sknnr_stream_set_tally",
    "sknnr_stream_get_tally",
    "sknnr_debug_last_tally",
    "sknnr_zonal_from_values",
    "sknnr_stream_set_zonal",
    "sknnr_stream_next_zones",
    "sknnr_stream_get_zonal",
    "sknnr_debug_last_zonal",
    "sknnr_debug_zonal_geometry",
    "sknnr_domain_from_neighbors",
    "sknnr_stream_set_domain",
    "sknnr_stream_next_domain_out",
    "sknnr_stream_get_domain",
    "sknnr_debug_last_domain",
    "sknnr_debug_domain_geometry",
    "sknnr_index_create_targets",
    "sknnr_index_set_replay_ids",
    "sknnr_replay_begin",
    "sknnr_replay_push",
    "sknnr_replay_push_planes",
    "sknnr_replay_get_counts",
    "sknnr_debug_last_replay",
    "sknnr_index_set_bootstrap",
    "sknnr_bootstrap_from_neighbors",
    "sknnr_stream_set_bootstrap",
    "sknnr_stream_get_bootstrap",
    "sknnr_debug_last_bootstrap",
    "sknnr_debug_last_narrow",
    "sknnr_debug_last_mask",
    "sknnr_debug_mask_compact",
    "sknnr_debug_expand_rows",
    "sknnr_crosswalk",
    "sknnr_debug_coarse_matrix",
    "sknnr_debug_last_prefilter",
    "sknnr_debug_last_finalize",
    "sknnr_debug_last_hamming",
    "sknnr_debug_last_scan",
    "sknnr_debug_last_rescue",
    "sknnr_debug_hamming_candidates",
    "sknnr_debug_coarse_candidates",
    "sknnr_debug_last_prep",
    "sknnr_debug_query_prep",
    "sknnr_debug_image_constants",
    "sknnr_debug_search_plan",
)


# geometry of the neighbour-usage kernel (sknnr_amd/csrc/tally.hip.h: kTallyWgEntries, tally_rows_per_wg); the table's
# slots come from the library itself (Index.debug_last_tally()["slots"])
TALLY_WG_ENTRIES = 8192


def tally_rows_per_workgroup(k: int) -> int:
    """Consecutive rows one workgroup of the tally kernel takes at ``k`` neighbours."""
    return 1 if k >= TALLY_WG_ENTRIES else TALLY_WG_ENTRIES // int(k)


ZONAL_FIELDS = 6  # acc[z, j, :]: count, sum, sq_lo, sq_hi, min, max (include/sknnr_hip.h, "Zonal statistics")


def zonal_geometry(c: int) -> dict:
    """Geometry of the zonal kernel at ``c`` columns, from the library itself (sknnr_debug_zonal_geometry; no device work):
    pixels a workgroup takes, slots of its table, slots of its class table, slots an entry probes."""
    out = (c_int64 * 4)()
    check(load().sknnr_debug_zonal_geometry(int(c), out))
    return dict(zip(("pixels_per_workgroup", "slots", "hist_slots", "probes"), (int(v) for v in out)))


def _zonal_classes(n_classes, c):
    """``n_classes`` (None, or one count per column) as the C ABI takes it: int32 ``(c,)`` or None, and the histogram's length
    per zone."""
    if n_classes is None:
        return None, 0
    n_classes = np.ascontiguousarray(n_classes, dtype=np.int32).reshape(-1)
    if n_classes.size != c:
        raise ValueError(f"n_classes must hold one value per column ({c}), got {n_classes.size}")
    if not n_classes.any():
        return None, 0
    return n_classes, int(n_classes.astype(np.int64).sum())


DOMAIN_ACC = 103  # acc: codes 0 .. 100, beyond pixels, nodata pixels (include/sknnr_hip.h, "Distance domain")
DOMAIN_NODATA_CODE = 255


def domain_geometry(m: int) -> dict:
    """Geometry of the domain kernel for a table of ``m`` entries, from the library itself (sknnr_debug_domain_geometry; no
    device work): pixels a workgroup takes, the most entries of its skeleton of the table, table entries between two
    skeleton entries, skeleton entries in use."""
    out = (c_int64 * 4)()
    check(load().sknnr_debug_domain_geometry(int(m), out))
    return dict(zip(("pixels_per_workgroup", "skeleton", "stride", "skeleton_used"), (int(v) for v in out)))


def _domain_args(table, threshold):
    """``table`` / ``threshold`` as the C ABI takes them: a C-contiguous float64 array, its length, has_threshold and the
    threshold (0.0 without one).  The library validates them."""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
    return table, int(table.size), int(threshold is not None), float(0.0 if threshold is None else threshold)


class QueryOpts(ctypes.Structure):
    _fields_ = [
        ("n_neighbors", c_int32),
        ("exclude_self", c_int32),
        ("deterministic", c_int32),
        ("decimals", c_int32),
        ("formula", c_int32),
        ("apply_affine", c_int32),
        ("weight_mode", c_int32),
        ("check_finite", c_int32),
        ("query_dtype", c_int32),
        ("weight_law", c_int32),  # sknnr_weight_law, 0 = none (the field was reserved_)
        ("row_offset", c_int64),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("queries", c_int64),
        ("coarse_queries", c_int64),
        ("exact_fallbacks", c_int64),
        ("exact_only_queries", c_int64),
        ("last_kernel_ms", c_double),
        ("last_coarse_ms", c_double),
        ("total_kernel_ms", c_double),
        ("total_coarse_ms", c_double),
        ("timed_calls", c_int64),
        ("coarse_rows_timed", c_int64),
        ("mfma_executed_ratio", c_double),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class HipBackendError(RuntimeError):
    """A call into libsknnr_hip.so failed; ``code`` is the sknnr_status."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[sknnr_hip {code}] {message}")
        self.code = code
        self.message = message


_lib = None


def library_path() -> str:
    """The in-tree build, or the file named by SKNNR_HIP_LIBRARY (development variants)."""
    return os.environ.get("SKNNR_HIP_LIBRARY") or _build.LIB_PATH


def load(build_if_missing: bool = False):
    """Load libsknnr_hip.so (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm is the carrier of device memory and streams, and it bundles its own HIP
    # runtime (SONAME libamdhip64.so.7).  Importing it FIRST makes the dynamic loader bind
    # libsknnr_hip.so to that same runtime; loading ours first would put a second HIP/HSA
    # runtime in the process and torch would then see no device.
    import torch  # noqa: F401

    path = library_path()
    if not os.path.exists(path):
        if build_if_missing:
            _build.build()
        else:
            raise ImportError(
                f"{path} is missing: the MI355X backend has not been built. "
                "Run `python -m sknnr_amd._build` (needs hipcc); there is no CPU fallback."
            )
    lib = ctypes.CDLL(path)
    if lib.sknnr_abi_version() != ABI_VERSION:
        raise ImportError(
            f"{path} has ABI version {lib.sknnr_abi_version()}, this package needs {ABI_VERSION}: "
            "rebuild it with `python -m sknnr_amd._build --force`")
    vp = c_void_p
    lib.sknnr_device_count.restype = c_int32
    lib.sknnr_abi_version.restype = c_int32
    lib.sknnr_last_error.restype = c_char_p
    lib.sknnr_index_create.argtypes = [vp, c_int64, c_int32, vp, c_int32, c_int32, POINTER(vp)]
    lib.sknnr_index_destroy.argtypes = [vp]
    lib.sknnr_index_destroy.restype = None
    lib.sknnr_index_set_affine.argtypes = [vp, c_int32, vp, vp, vp]
    lib.sknnr_index_set_hamming_weights.argtypes = [vp, vp, c_int32]
    lib.sknnr_index_set_forest.argtypes = [vp, c_int32, c_int32, vp, vp, vp, vp, vp]
    lib.sknnr_forest_apply.argtypes = [vp, vp, c_int64, c_int32, c_int32, vp]
    lib.sknnr_affine_transform.argtypes = [vp, c_int64, c_int32, vp, vp, vp, c_int32, vp, c_int32]
    lib.sknnr_index_shape.argtypes = [vp, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32),
                                      POINTER(c_int32), POINTER(c_int32)]
    lib.sknnr_get_stats.argtypes = [vp, POINTER(Stats)]
    lib.sknnr_reset_stats.argtypes = [vp]
    lib.sknnr_check_finite.argtypes = [vp, vp]
    lib.sknnr_stream_begin.argtypes = [vp, POINTER(QueryOpts), c_int32, c_int32, POINTER(vp)]
    lib.sknnr_stream_push.argtypes = [vp, vp, c_int64, vp, vp, vp]
    lib.sknnr_stream_flush.argtypes = [vp]
    lib.sknnr_stream_end.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_mask_rows.argtypes = [vp, c_int64, c_int32, c_int32, vp, c_int32, c_int32, vp, vp, POINTER(c_int64)]
    lib.sknnr_kneighbors_masked.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), vp, c_int64, vp, vp, c_int32, vp,
                                            POINTER(c_int64)]
    lib.sknnr_predict_masked.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), vp, c_int64, vp, vp, vp, c_int32, vp,
                                         POINTER(c_int64)]
    lib.sknnr_stream_set_nodata.argtypes = [vp, vp, c_int64]
    lib.sknnr_stream_valid_rows.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_debug_last_mask.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_planes_to_rows.argtypes = [vp, c_int64, c_int32, c_int32, c_int64, vp, c_int32, vp]
    lib.sknnr_rows_to_planes.argtypes = [vp, c_int64, c_int32, vp, c_int64, c_int32, vp]
    lib.sknnr_stream_push_planes.argtypes = [vp, vp, c_int64, vp, vp, vp, c_int64]
    lib.sknnr_debug_last_planes.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_narrow.argtypes = [vp, c_int32, c_int64, c_int32, vp, c_int32, c_int64, vp, vp, c_int32, c_double, c_int32, vp,
                                 POINTER(c_int32)]
    lib.sknnr_stream_set_output.argtypes = [vp, c_int32, c_int32, c_int32, vp, vp, c_int32, c_double]
    lib.sknnr_narrow_ids.argtypes = [vp, c_int64, c_int32, vp, c_int64, c_int32, c_int64, vp, c_int32, c_int64, c_int32, vp,
                                     POINTER(c_int32)]
    lib.sknnr_stream_set_id_table.argtypes = [vp, vp, c_int64, c_int64]
    lib.sknnr_stream_push_typed.argtypes = [vp, vp, c_int64, vp, vp, vp]
    lib.sknnr_stream_push_planes_typed.argtypes = [vp, vp, c_int64, vp, vp, vp, c_int64]
    lib.sknnr_debug_last_narrow.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_debug_mask_compact.argtypes = [vp, c_int64, c_int32, c_int32, vp, c_int32, vp, vp, vp, vp, vp,
                                             POINTER(c_int32), POINTER(c_int64)]
    lib.sknnr_debug_expand_rows.argtypes = [c_int64, c_int32, c_int32, vp, vp, vp, vp, vp, vp, vp, vp, c_int64, vp]
    lib.sknnr_kneighbors.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), vp, vp, c_int32, vp]
    lib.sknnr_predict.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), vp, vp, vp, c_int32, vp]
    lib.sknnr_predict_from_neighbors.argtypes = [vp, vp, vp, vp, c_int64, c_int32, c_int32, vp,
                                                 c_int32, vp]
    if hasattr(lib, "sknnr_summarize"):  # (a SKNNR_HIP_LIBRARY variant built before the entry points existed)
        lib.sknnr_summarize_from_neighbors.argtypes = [vp, vp, vp, vp, c_int64, c_int32, c_int32, vp, vp, c_int32, vp]
        lib.sknnr_summarize.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), vp, vp, vp, vp, c_int32, vp]
        lib.sknnr_stream_set_statistics.argtypes = [vp, vp, c_int32]
        lib.sknnr_debug_last_summary.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_summarize_plan"):
        lib.sknnr_summarize_plan_from_neighbors.argtypes = [vp, vp, vp, vp, c_int64, c_int32, c_int32, vp, vp, vp, c_int32,
                                                            vp, c_int32, vp]
        lib.sknnr_summarize_plan.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), vp, vp, vp, c_int32, vp, vp, vp, c_int32, vp]
        lib.sknnr_stream_set_plan.argtypes = [vp, vp, vp, vp, c_int32]
        lib.sknnr_debug_last_plan.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_index_set_weight_law_params.argtypes = [vp, c_int32, c_double, c_double]
    lib.sknnr_debug_last_weight_law.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_debug_weight_law.argtypes = [c_int32, c_double, c_double, vp, c_int64, vp, c_int32, c_int32]
    lib.sknnr_hamming_distances.argtypes = [vp, vp, c_int64, vp, c_int64, vp, c_int32, vp]
    if hasattr(lib, "sknnr_kneighbors_grouped"):  # (a SKNNR_HIP_LIBRARY variant built before the entry points existed)
        lib.sknnr_index_set_groups.argtypes = [vp, vp, c_int64]
        lib.sknnr_kneighbors_grouped.argtypes = [vp, c_int64, POINTER(QueryOpts), vp, vp, c_int32, vp]
        lib.sknnr_debug_last_grouped.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_index_set_buffer"):  # (likewise)
        lib.sknnr_index_set_buffer.argtypes = [vp, vp, c_int64, c_int32, c_double]
        lib.sknnr_buffer_counts.argtypes = [vp, vp, c_int32, vp]
        lib.sknnr_debug_last_buffer.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_tally_from_neighbors"):  # (likewise)
        lib.sknnr_tally_from_neighbors.argtypes = [vp, vp, vp, c_int64, c_int32, vp, vp, c_int32, c_int32, vp]
        lib.sknnr_stream_set_tally.argtypes = [vp]
        lib.sknnr_stream_get_tally.argtypes = [vp, vp, vp]
        lib.sknnr_debug_last_tally.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_zonal_from_values"):  # (likewise)
        lib.sknnr_zonal_from_values.argtypes = [vp, vp, vp, c_int64, c_int32, c_int32, vp, vp, c_int64, vp, vp, vp, c_int32,
                                                c_int32, vp]
        lib.sknnr_stream_set_zonal.argtypes = [vp, c_int64, vp]
        lib.sknnr_stream_next_zones.argtypes = [vp, vp, c_int64]
        lib.sknnr_stream_get_zonal.argtypes = [vp, vp, vp]
        lib.sknnr_debug_last_zonal.argtypes = [vp, POINTER(c_int64)]
        lib.sknnr_debug_zonal_geometry.argtypes = [c_int32, POINTER(c_int64)]
    if hasattr(lib, "sknnr_domain_from_neighbors"):  # (likewise)
        lib.sknnr_domain_from_neighbors.argtypes = [vp, vp, c_int64, c_int32, c_int32, vp, c_int64, c_int32, c_double, vp, vp,
                                                    c_int32, c_int32, vp]
        lib.sknnr_stream_set_domain.argtypes = [vp, vp, c_int64, c_int32, c_int32, c_double, c_int32]
        lib.sknnr_stream_next_domain_out.argtypes = [vp, vp, c_int64]
        lib.sknnr_stream_get_domain.argtypes = [vp, vp]
        lib.sknnr_debug_last_domain.argtypes = [vp, POINTER(c_int64)]
        lib.sknnr_debug_domain_geometry.argtypes = [c_int64, POINTER(c_int64)]
    if hasattr(lib, "sknnr_replay_begin"):  # (likewise)
        lib.sknnr_index_create_targets.argtypes = [vp, c_int64, c_int32, c_int32, POINTER(vp)]
        lib.sknnr_index_set_replay_ids.argtypes = [vp, vp, c_int64]
        lib.sknnr_replay_begin.argtypes = [vp, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32, c_int32,
                                           c_int32, POINTER(vp)]
        lib.sknnr_replay_push.argtypes = [vp, vp, vp, c_int64, vp, vp, vp]
        lib.sknnr_replay_push_planes.argtypes = [vp, vp, vp, c_int64, c_int64, vp, vp, vp, c_int64]
        lib.sknnr_replay_get_counts.argtypes = [vp, POINTER(c_int64)]
        lib.sknnr_debug_last_replay.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_bootstrap_from_neighbors"):  # (likewise)
        lib.sknnr_index_set_bootstrap.argtypes = [vp, vp, c_int32, c_int64]
        lib.sknnr_bootstrap_from_neighbors.argtypes = [vp, vp, vp, c_int64, c_int32, c_int32, c_int32, c_int32, vp, vp, c_int32,
                                                       vp, vp, c_int32, vp]
        lib.sknnr_stream_set_bootstrap.argtypes = [vp, c_int32, vp, vp, c_int32]
        lib.sknnr_stream_get_bootstrap.argtypes = [vp, POINTER(c_int64)]
        lib.sknnr_debug_last_bootstrap.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_shard_candidates.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), c_int64, vp, vp, c_int32, vp]
    lib.sknnr_merge_shards.argtypes = [vp, vp, c_int64, POINTER(QueryOpts), c_int32, vp, vp, vp, vp, c_int32, vp]
    lib.sknnr_crosswalk.argtypes = [vp, c_int64, vp, c_int64, vp, c_int32, c_int32, vp]
    lib.sknnr_debug_coarse_matrix.argtypes = [vp, vp, c_int64, vp, vp, POINTER(c_double),
                                              POINTER(c_double)]
    lib.sknnr_debug_last_prefilter.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_debug_last_finalize"):  # (a SKNNR_HIP_LIBRARY variant built before the entry point existed)
        lib.sknnr_debug_last_finalize.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_debug_last_hamming.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_debug_last_scan"):  # (likewise)
        lib.sknnr_debug_last_scan.argtypes = [vp, POINTER(c_int64)]
    if hasattr(lib, "sknnr_debug_last_rescue"):  # (likewise)
        lib.sknnr_debug_last_rescue.argtypes = [vp, POINTER(c_int64)]
    lib.sknnr_debug_hamming_candidates.argtypes = [vp, vp, vp, c_int64]
    lib.sknnr_debug_coarse_candidates.argtypes = [vp, c_int64, vp, vp, vp]
    if hasattr(lib, "sknnr_debug_last_prep"):  # (likewise)
        lib.sknnr_debug_last_prep.argtypes = [vp, POINTER(c_int64)]
        lib.sknnr_debug_query_prep.argtypes = [vp, c_int64, vp, vp, vp, vp, vp, vp]
        lib.sknnr_debug_image_constants.argtypes = [vp, vp, POINTER(c_double), POINTER(c_int32), vp, vp, vp]
    if hasattr(lib, "sknnr_debug_search_plan"):  # (likewise)
        lib.sknnr_debug_search_plan.argtypes = [c_int64, c_int32, c_int32, c_int32, c_int64, c_int32, c_int32, POINTER(c_int64)]
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != 0:
        raise HipBackendError(code, load().sknnr_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return int(load().sknnr_device_count())


SEARCH_PLAN_FIELDS = ("generation", "ks", "m_list", "rank_extra", "cell_depth", "record", "rescue", "ham_int", "kk", "chunk",
                      "cap_pad", "to_xt", "d_x", "check_finite", "x_dtype", "row_bits")


def debug_search_plan(n_ref: int, d: int, kk: int, nq: int, cell_depth: int = 0, formula: int = FORMULA_EXPANDED,
                      exclude_self: bool = False, raw: bool = False, h16_ok: bool = False, rescue_enabled: bool = True) -> dict:
    """Debug only: the plan a search call works out before its first launch (sknnr_debug_search_plan), for an index of
    ``n_ref`` x ``d`` rows with ``cell_depth`` levels of cells and a call of ``nq`` rows searching ``kk`` neighbours
    (k, + 1 with ``exclude_self``).  No handle, no device."""
    flags = (1 if exclude_self else 0) | (2 if raw else 0) | (4 if h16_ok else 0) | (8 if rescue_enabled else 0)
    out = (c_int64 * 16)()
    check(load().sknnr_debug_search_plan(n_ref, d, cell_depth, kk, nq, formula, flags, out))
    return dict(zip(SEARCH_PLAN_FIELDS, out))


def _host_ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _c_f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _c_stat(stat):
    """Statistic codes (``STATISTICS`` values) as the C entry points read them, or None."""
    return None if stat is None else np.ascontiguousarray(stat, dtype=np.int32).reshape(-1)


def _c_plan(plan):
    """An output plan ``(cols, codes, params)`` as the C entry points read it: int32, int32 and float64 host arrays of one
    length (``PLAN_STATISTICS`` codes)."""
    cols, codes, params = plan
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    codes = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
    params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    if not (cols.size == codes.size == params.size):
        raise ValueError("an output plan's columns, codes and parameters must have one length")
    return cols, codes, params


# sknnr_bootstrap_statistic (include/sknnr_hip.h)
BOOT_STATISTICS = {"boot_se": 0, "boot_mean": 1, "boot_bias": 2, "boot_count": 3}


def bootstrap_pixels_per_wave(B: int, kw: int) -> int:
    """Pixels one wave of the bootstrap kernel reduces (sknnr_amd/csrc/bootstrap.hip.h: bootstrap_ppw)."""
    if B <= 16 and 4 * kw <= 192:
        return 4
    if B <= 32 and 2 * kw <= 192:
        return 2
    return 1


def _c_boot_plan(plan):
    """A bootstrap plan ``(cols, codes)`` as the C entry points read it: two int32 host arrays of one length."""
    cols, codes = plan
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    codes = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
    if cols.size != codes.size:
        raise ValueError("a bootstrap plan's columns and codes must have one length")
    return cols, codes


def _c_rows(a, opts):
    """Query rows as the call will read them: C-contiguous, of the element type ``opts.query_dtype`` names (the caller set
    it from the array's dtype: Index.make_opts(query_dtype=...)), else float64."""
    if a is None:
        return None
    for dt, code in DTYPE_CODES.items():
        if code == opts.query_dtype:
            return np.ascontiguousarray(a, dtype=dt)
    raise ValueError(f"unknown query_dtype {opts.query_dtype}")


class Index:
    """Owner of one ``sknnr_index*``.  Inputs/outputs are numpy arrays (host) or raw
    device pointers (ints) -- see :mod:`sknnr_amd._engine` for the torch-tensor layer."""

    def __init__(self, ref, y=None, device: int = 0):
        lib = load()
        ref = _c_f64(ref)
        if ref.ndim != 2:
            raise ValueError("ref must be 2-D")
        y2 = None
        if y is not None:
            y2 = _c_f64(y)
            if y2.ndim == 1:
                y2 = y2.reshape(-1, 1)
            if y2.shape[0] != ref.shape[0]:
                raise ValueError("y and ref row counts differ")
        self.n_ref, self.d = ref.shape
        self.t = 0 if y2 is None else y2.shape[1]
        self.device = device
        self.d_in = self.d
        self._h = c_void_p()
        check(lib.sknnr_index_create(_host_ptr(ref), self.n_ref, self.d, _host_ptr(y2), self.t,
                                     device, byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().sknnr_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("index is closed")
        return self._h

    def set_affine(self, d_in: int, center=None, scale=None, proj=None):
        center, scale, proj = _c_f64(center), _c_f64(scale), _c_f64(proj)
        if proj is not None and proj.shape != (d_in, self.d):
            raise ValueError(f"proj must be ({d_in}, {self.d}), got {proj.shape}")
        check(load().sknnr_index_set_affine(self.handle, d_in, _host_ptr(center), _host_ptr(scale),
                                            _host_ptr(proj)))
        self.d_in = d_in

    def set_hamming_weights(self, w):
        w = _c_f64(w).reshape(-1)
        check(load().sknnr_index_set_hamming_weights(self.handle, _host_ptr(w), w.size))

    def set_groups(self, codes):
        """The group code of every reference row for :meth:`kneighbors_grouped` (sknnr_index_set_groups): ``n_ref``
        integers >= 0, copied to the device and kept on the handle; ``None`` clears them."""
        if codes is None:
            check(load().sknnr_index_set_groups(self.handle, None, 0))
            return
        codes = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        check(load().sknnr_index_set_groups(self.handle, _host_ptr(codes), codes.size))

    def kneighbors_grouped(self, k, *, deterministic, decimals, formula, row_offset=0, n_rows=None, return_distance=True):
        """Leave-group-out neighbours of reference rows ``[row_offset, row_offset + n_rows)`` (sknnr_kneighbors_grouped;
        ``n_rows=None``: to the last row): for every row the ``k`` rows of OTHER groups smallest by (value, index) under
        ``formula``, then the square root (not for Hamming) and, with ``deterministic``, sknnr's reorder.  Exact ties at
        the k-th value go to the lower index -- no heap history is replayed.  Returns numpy ``(dist or None, idx)``."""
        if n_rows is None:
            n_rows = self.n_ref - int(row_offset)
        opts = self.make_opts(k, exclude_self=True, deterministic=deterministic, decimals=decimals, formula=formula,
                              row_offset=row_offset)
        n = max(int(n_rows), 0)
        idx = np.empty((n, int(k)), dtype=np.int64)
        dist = np.empty((n, int(k)), dtype=np.float64) if return_distance else None
        check(load().sknnr_kneighbors_grouped(self.handle, int(n_rows), byref(opts), _host_ptr(dist), _host_ptr(idx),
                                              MEM_HOST, None))
        return dist, idx

    GROUPED_FIELDS = ("formula_plus_1", "k", "workgroups", "lds_bytes", "rows", "slices", "largest_group", "n_groups")

    def debug_last_grouped(self) -> dict:
        """Debug only: the leave-group-out scan of the last search call (sknnr_debug_last_grouped): formula + 1 (0: no
        grouped scan ran), k, workgroups and dynamic LDS bytes of the launch, rows, slices (1: none), the rows of the
        largest group and the number of groups.  Every search call zeroes it first."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_grouped(self.handle, out))
        return dict(zip(self.GROUPED_FIELDS, (int(v) for v in out)))

    def set_buffer(self, coords, radius=0.0):
        """The plot positions and the radius of a buffered :meth:`kneighbors_grouped` (sknnr_index_set_buffer):
        ``(n_ref, c)`` float64 positions, ``c`` 1 to 3, and a finite radius >= 0; a row within the radius of the query
        row (``g <= radius * radius``, include/sknnr_hip.h) is no candidate.  ``None`` clears the buffer."""
        if coords is None:
            check(load().sknnr_index_set_buffer(self.handle, None, 0, 0, 0.0))
            return
        coords = _c_f64(coords)
        if coords.ndim == 1:
            coords = coords.reshape(-1, 1)
        check(load().sknnr_index_set_buffer(self.handle, _host_ptr(coords), coords.shape[0], coords.shape[1], float(radius)))

    def buffer_counts(self):
        """``excluded[]`` (sknnr_buffer_counts): per reference row the rows the masks now set exclude for it, itself
        included -- int64 ``(n_ref,)``.  Counted on the device once per change of either mask."""
        out = np.empty(self.n_ref, dtype=np.int64)
        check(load().sknnr_buffer_counts(self.handle, _host_ptr(out), MEM_HOST, None))
        return out

    BUFFER_FIELDS = ("mask", "c", "max_excluded", "min_excluded", "count_workgroups", "count_lds_bytes", "argmax_row", "reserved")

    def debug_last_buffer(self) -> dict:
        """Debug only: the masks of the leave-out scan of the last search call (sknnr_debug_last_buffer): mask mode (0:
        no grouped scan ran, 1 groups, 2 buffer, 3 both), position columns, max and min of ``excluded[]``, workgroups
        and LDS bytes of the launch that counted them, the first row that attains the maximum."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_buffer(self.handle, out))
        return dict(zip(self.BUFFER_FIELDS, (int(v) for v in out)))

    def set_forest(self, d_in, tree_offset, threshold, feature, left, right):
        """Install the query-time forest map (sknnr_index_set_forest): the flattened trees of
        ``TreeNodeTransformer.forest_image()``, one tree per column of the node-id rows."""
        off = np.ascontiguousarray(tree_offset, dtype=np.int64)
        thr = _c_f64(threshold)
        feat, lc, rc = (np.ascontiguousarray(a, dtype=np.int32) for a in (feature, left, right))
        n_nodes = int(off[-1]) if off.size else 0
        if off.ndim != 1 or off.size < 2 or any(a.shape != (n_nodes,) for a in (thr, feat, lc, rc)):
            raise ValueError("tree_offset must hold n_trees + 1 offsets and the node arrays tree_offset[-1] entries")
        check(load().sknnr_index_set_forest(self.handle, int(d_in), off.size - 1, _host_ptr(off), _host_ptr(thr),
                                            _host_ptr(feat), _host_ptr(lc), _host_ptr(rc)))
        self.d_in = int(d_in)

    def forest_apply_host(self, q, query_dtype=0):
        """Node ids ``(nq, n_trees)`` float64 of the raw rows ``q`` through the installed forests (sknnr_forest_apply)."""
        q = _c_rows(q, QueryOpts(query_dtype=int(query_dtype)))
        out = np.empty((q.shape[0], self.d), dtype=np.float64)
        check(load().sknnr_forest_apply(self.handle, _host_ptr(q), q.shape[0], int(query_dtype), MEM_HOST,
                                        _host_ptr(out)))
        return out

    def forest_apply_device(self, q_ptr, nq, query_dtype, out_ptr):
        check(load().sknnr_forest_apply(self.handle, c_void_p(q_ptr or None), nq, int(query_dtype), MEM_DEVICE,
                                        c_void_p(out_ptr or None)))

    def stats(self) -> dict:
        st = Stats()
        check(load().sknnr_get_stats(self.handle, byref(st)))
        out = st.as_dict()
        if hasattr(load(), "sknnr_debug_last_rescue"):
            out["rescued_rows"] = self.debug_last_rescue()["rescued_total"]
        return out

    def reset_stats(self):
        check(load().sknnr_reset_stats(self.handle))

    @staticmethod
    def make_opts(k, exclude_self=False, deterministic=True, decimals=10, formula=FORMULA_EXPANDED,
                  apply_affine=False, weight_mode=WEIGHTS_UNIFORM, row_offset=0,
                  check_finite=False, query_dtype=0, weight_law=WEIGHT_LAW_NONE) -> QueryOpts:
        """``weight_law``: a ``WEIGHT_LAWS`` code -- the predictions' weights are that law of the call's distances,
        computed on the device with the parameters of :meth:`set_weight_law_params`; ``weight_mode`` is then
        ``WEIGHTS_EXPLICIT`` (with ``WEIGHTS_F32_TARGETS`` where it applies)."""
        return QueryOpts(int(k), int(bool(exclude_self)), int(bool(deterministic)), int(decimals),
                         int(formula), int(bool(apply_affine)), int(weight_mode), int(bool(check_finite)),
                         int(query_dtype), int(weight_law), int(row_offset))

    def set_weight_law_params(self, law: int, p0: float = 0.0, p1: float = 0.0) -> None:
        """The handle's distance-weight law (a ``WEIGHT_LAWS`` code, 0 clears) and its two float64 parameters
        (sknnr_index_set_weight_law_params); calls whose opts name the law use them."""
        check(load().sknnr_index_set_weight_law_params(self.handle, int(law), float(p0), float(p1)))

    def set_replay_ids(self, ids) -> None:
        """The id table of replay streams whose stored values are ids (sknnr_index_set_replay_ids): one int64 id per
        reference row, unique; None removes it."""
        if ids is None:
            check(load().sknnr_index_set_replay_ids(self.handle, None, 0))
            return
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        check(load().sknnr_index_set_replay_ids(self.handle, _host_ptr(ids), int(ids.size)))

    def open_replay(self, k, ks, *, weight_mode=0, weight_law=0, idx_dtype=np.int64, dist_dtype=None, fill_index=-1,
                    ids=False, want_dist=False, want_pred=True):
        """A :class:`ReplayStream` on this handle (sknnr_replay_begin): tiles of ``ks`` stored neighbour columns of
        ``idx_dtype`` (int32 / int64) and ``dist_dtype`` (float32 / float64, None: no distances), of which the leading
        ``k`` are used."""
        return ReplayStream(self, k, ks, weight_mode, weight_law, idx_dtype, dist_dtype, fill_index, ids, want_dist, want_pred)

    def debug_last_replay(self) -> dict:
        """Debug only: the last replayed tile of the handle (sknnr_debug_last_replay)."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_replay(self.handle, out))
        return dict(zip(("pixels", "masked", "unknown", "instance", "skeleton", "search_launches", "k", "ks"), map(int, out)))

    # ---- bootstrap (include/sknnr_hip.h, "Bootstrap") --------------------------------------------
    def set_bootstrap(self, table) -> None:
        """The multiplicity table of bootstrap reductions (sknnr_index_set_bootstrap): ``(B, n_ref)`` non-negative
        integers, clamped to 255 (no result can tell, k <= 192); ``None`` removes it."""
        if table is None:
            check(load().sknnr_index_set_bootstrap(self.handle, None, 0, 0))
            return
        table = np.asarray(table)
        if table.ndim != 2:
            raise ValueError(f"a bootstrap table is (B, n_ref), got shape {table.shape}")
        table = np.ascontiguousarray(np.minimum(table, 255), dtype=np.uint8)
        check(load().sknnr_index_set_bootstrap(self.handle, _host_ptr(table), int(table.shape[0]), int(table.shape[1])))

    def bootstrap_from_neighbors_host(self, dist, idx, k, plan, weight_mode=0, weight_law=0):
        """The bootstrap reduction alone (sknnr_bootstrap_from_neighbors) on host ``(nq, kw)`` neighbours:
        ``(out, tally)`` with ``out`` ``(nq, n_out)`` float64 and ``tally`` the int64 pair (pixels, valid replicates).
        ``plan``: ``(cols, codes)`` (``BOOT_STATISTICS`` codes)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        dist = _c_f64(dist)
        cols, codes = _c_boot_plan(plan)
        nq, kw = idx.shape
        out = np.empty((nq, cols.size), dtype=np.float64)
        tally = np.zeros(2, dtype=np.int64)
        check(load().sknnr_bootstrap_from_neighbors(
            self.handle, _host_ptr(dist), _host_ptr(idx), nq, kw, int(k), int(weight_mode), int(weight_law), _host_ptr(cols),
            _host_ptr(codes), int(cols.size), _host_ptr(out), _host_ptr(tally), MEM_HOST, None))
        return out, tally

    def bootstrap_from_neighbors_device(self, dist_ptr, idx_ptr, nq, kw, k, plan, out_ptr, tally_ptr=0, weight_mode=0,
                                        weight_law=0, stream=0):
        """Device pointers in and out (``tally_ptr``: two int64 words, or 0); the plan stays host arrays."""
        cols, codes = _c_boot_plan(plan)
        check(load().sknnr_bootstrap_from_neighbors(
            self.handle, c_void_p(dist_ptr or None), c_void_p(idx_ptr), nq, kw, int(k), int(weight_mode), int(weight_law),
            _host_ptr(cols), _host_ptr(codes), int(cols.size), c_void_p(out_ptr), c_void_p(tally_ptr or None), MEM_DEVICE,
            c_void_p(stream or None)))

    BOOTSTRAP_FIELDS = ("rows", "B", "k", "kw", "n_out", "pixels_per_wave", "launches", "reserved")

    def debug_last_bootstrap(self) -> dict:
        """Debug only: the last bootstrap reduction of the handle (sknnr_debug_last_bootstrap)."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_bootstrap(self.handle, out))
        return dict(zip(self.BOOTSTRAP_FIELDS, (int(v) for v in out)))

    def check_finite(self, stream=0) -> None:
        """Poll the non-finite-input flag of device-memory calls made with ``check_finite``
        (synchronises ``stream``); raises :class:`HipBackendError` (``ERR_NONFINITE``)."""
        check(load().sknnr_check_finite(self.handle, c_void_p(stream or None)))

    def open_stream(self, opts: QueryOpts, want_dist=True, want_pred=False, nodata=None, fill_index=-1,
                    output=None, statistic=None, id_table=None, fill_id=-1, plan=None, tally=False,
                    zonal=None, domain=None, bootstrap=None) -> "QueryStream":
        """``nodata``: float64 ``(d_in,)``, one value per column of the pushed rows -- every tile is then masked on the
        device (sknnr_stream_set_nodata) and masked rows get ``fill_index`` / NaN.  ``output``: keyword arguments of
        :meth:`QueryStream.set_output` -- the results then leave the device at those types.  ``statistic``: one
        ``STATISTICS`` code per target (:meth:`QueryStream.set_statistics`) -- the predictions become those summaries.
        ``id_table`` / ``fill_id``: :meth:`QueryStream.set_id_table` -- the indices leave as those ids; ``fill_index``
        must then be negative, and masked rows get ``fill_id``.  ``plan``: an output plan ``(cols, codes, params)``
        (:meth:`QueryStream.set_plan`; not together with ``statistic``) -- the prediction lane then holds its planes, and
        ``output``'s ``scale`` / ``offset`` one value per plane.  ``tally``: :meth:`QueryStream.set_tally`.  ``zonal``:
        ``(n_zones, n_classes)``, the arguments of :meth:`QueryStream.set_zonal`.  ``domain``: ``(table, rank, threshold,
        mask_beyond)``, the arguments of :meth:`QueryStream.set_domain`.  ``bootstrap``: ``(k, (cols, codes))``, the
        arguments of :meth:`QueryStream.set_bootstrap` -- the stream searches ``opts.n_neighbors`` candidates."""
        return QueryStream(self, opts, want_dist, want_pred).configure(
            nodata=nodata, fill_index=fill_index, output=output, statistic=statistic, id_table=id_table, fill_id=fill_id,
            plan=plan, tally=tally, zonal=zonal, domain=domain, bootstrap=bootstrap)

    # ---- host (numpy) entry points --------------------------------------------------------
    def kneighbors_host(self, q, opts: QueryOpts, nq=None, return_distance=True):
        q = _c_rows(q, opts)
        if q is not None:
            nq = q.shape[0]
        k = opts.n_neighbors
        idx = np.empty((nq, k), dtype=np.int64)
        dist = np.empty((nq, k), dtype=np.float64) if return_distance else None
        check(load().sknnr_kneighbors(self.handle, _host_ptr(q), nq, byref(opts), _host_ptr(dist),
                                      _host_ptr(idx), MEM_HOST, None))
        return dist, idx

    def predict_host(self, q, opts: QueryOpts, nq=None, return_neighbors=False):
        q = _c_rows(q, opts)
        if q is not None:
            nq = q.shape[0]
        k = opts.n_neighbors
        pred = np.empty((nq, self.t), dtype=np.float64)
        dist = idx = None
        if return_neighbors:
            dist = np.empty((nq, k), dtype=np.float64)
            idx = np.empty((nq, k), dtype=np.int64)
        check(load().sknnr_predict(self.handle, _host_ptr(q), nq, byref(opts), _host_ptr(pred),
                                   _host_ptr(dist), _host_ptr(idx), MEM_HOST, None))
        return (pred, dist, idx) if return_neighbors else pred

    def predict_from_neighbors_host(self, dist, idx, w, weight_mode):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        dist, w = _c_f64(dist), _c_f64(w)
        nq, k = idx.shape
        pred = np.empty((nq, self.t), dtype=np.float64)
        check(load().sknnr_predict_from_neighbors(self.handle, _host_ptr(dist), _host_ptr(idx),
                                                  _host_ptr(w), nq, k, int(weight_mode),
                                                  _host_ptr(pred), MEM_HOST, None))
        return pred

    # ---- neighbour usage (include/sknnr_hip.h, "Neighbour usage") ----------------------------
    def tally_from_neighbors_host(self, dist, idx, counts=None, max_dist=None):
        """Per-row use counts of ``idx`` ``(nq, k)`` int64 and, with ``dist``, the largest distance per reference row
        (sknnr_tally_from_neighbors on host arrays).  ``counts`` ``(n_ref, k)`` int64 / ``max_dist`` ``(n_ref,)`` float64:
        arrays to ADD to (``accumulate = 1``); None: fresh ones.  ``dist`` None: counts only, and ``max_dist`` comes back
        None.  Entries outside ``[0, n_ref)`` are skipped.  Returns ``(counts, max_dist)``."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.ndim != 2:
            raise ValueError("idx must be (nq, k)")
        nq, k = idx.shape
        dist = _c_f64(dist)
        if dist is not None and dist.shape != idx.shape:
            raise ValueError(f"dist must have the shape of idx {idx.shape}, got {dist.shape}")
        accumulate = counts is not None
        if accumulate:
            if counts.dtype != np.int64 or counts.shape != (self.n_ref, k) or not counts.flags.c_contiguous:
                raise ValueError(f"counts must be C-contiguous int64 ({self.n_ref}, {k})")
            if dist is not None and (max_dist is None or max_dist.dtype != np.float64 or max_dist.shape != (self.n_ref,)
                                     or not max_dist.flags.c_contiguous):
                raise ValueError(f"max_dist must be C-contiguous float64 ({self.n_ref},)")
        else:
            counts = np.empty((self.n_ref, k), dtype=np.int64)
            max_dist = np.empty(self.n_ref, dtype=np.float64) if dist is not None else None
        if dist is None:
            max_dist = None
        check(load().sknnr_tally_from_neighbors(self.handle, _host_ptr(dist), _host_ptr(idx), nq, k, _host_ptr(counts),
                                                _host_ptr(max_dist), int(accumulate), MEM_HOST, None))
        return counts, max_dist

    def tally_from_neighbors_device(self, dist_ptr, idx_ptr, nq, k, counts_ptr, max_dist_ptr=0, accumulate=False, stream=0):
        """sknnr_tally_from_neighbors on device pointers: enqueues on ``stream`` and returns; ``dist_ptr`` and
        ``max_dist_ptr`` both 0 for counts only."""
        check(load().sknnr_tally_from_neighbors(self.handle, c_void_p(dist_ptr or None), c_void_p(idx_ptr or None), int(nq),
                                                int(k), c_void_p(counts_ptr or None), c_void_p(max_dist_ptr or None),
                                                int(bool(accumulate)), MEM_DEVICE, c_void_p(stream or None)))

    TALLY_FIELDS = ("ran", "rows", "k", "tallied", "skipped", "global_atomics", "overflowed", "slots")

    def debug_last_tally(self) -> dict:
        """Debug only (sknnr_debug_last_tally; synchronises the device): the last :meth:`tally_from_neighbors_host` /
        ``_device`` call, or the open tallying stream so far -- ran, rows, k, entries tallied, entries skipped (outside
        ``[0, n_ref)``), global atomics issued on the accumulators, entries that found no slot in their workgroup's table,
        and the slots of that table."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_tally(self.handle, out))
        return dict(zip(self.TALLY_FIELDS, (int(v) for v in out)))

    # ---- zonal statistics (include/sknnr_hip.h, "Zonal statistics") ---------------------------
    def zonal_from_values_host(self, values, zones, dtype, n_zones, scale=None, offset=None, n_classes=None, acc=None,
                               hist=None):
        """Zonal accumulators of a float64 value tile ``(n, c)`` and its ``(n,)`` int32 zone codes over the stored values of
        ``dtype`` (int16 / uint16 / uint8 / int32) with ``scale`` / ``offset`` (``(c,)`` each, or neither):
        sknnr_zonal_from_values on host arrays.  ``n_classes``: one class count per column (0: numeric), or None.  ``acc``
        ``(n_zones, c, 6)`` int64 / ``hist`` (the class blocks, flat int64): arrays to ADD to (``accumulate = 1``); None:
        fresh ones.  Returns ``(acc, hist)``, ``hist`` None when no column has classes."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        if values.ndim != 2:
            raise ValueError("values must be (n, c)")
        n, c = values.shape
        zones = np.ascontiguousarray(zones, dtype=np.int32).reshape(-1)
        if zones.size != n:
            raise ValueError(f"zones must hold one code per pixel ({n}), got {zones.size}")
        scale, offset = _c_f64(scale), _c_f64(offset)
        n_classes, per_zone = _zonal_classes(n_classes, c)
        accumulate = acc is not None
        if accumulate:
            if acc.dtype != np.int64 or acc.shape != (n_zones, c, ZONAL_FIELDS) or not acc.flags.c_contiguous:
                raise ValueError(f"acc must be C-contiguous int64 ({n_zones}, {c}, {ZONAL_FIELDS})")
            if per_zone and (hist is None or hist.dtype != np.int64 or hist.shape != (n_zones * per_zone,)
                             or not hist.flags.c_contiguous):
                raise ValueError(f"hist must be C-contiguous int64 ({n_zones * per_zone},)")
        else:
            acc = np.empty((n_zones, c, ZONAL_FIELDS), dtype=np.int64)
            hist = np.empty(n_zones * per_zone, dtype=np.int64) if per_zone else None
        if not per_zone:
            hist = None
        check(load().sknnr_zonal_from_values(self.handle, _host_ptr(values), _host_ptr(zones), n, c,
                                             DTYPE_CODES.get(np.dtype(dtype), -1), _host_ptr(scale), _host_ptr(offset),
                                             int(n_zones), _host_ptr(n_classes), _host_ptr(acc), _host_ptr(hist),
                                             int(accumulate), MEM_HOST, None))
        return acc, hist

    def zonal_from_values_device(self, values_ptr, zones_ptr, n, c, dtype, n_zones, acc_ptr, hist_ptr=0, scale=None,
                                 offset=None, n_classes=None, accumulate=False, stream=0):
        """sknnr_zonal_from_values on device pointers: enqueues on ``stream`` and returns.  ``scale`` / ``offset`` /
        ``n_classes`` are host arrays, as in the host form."""
        scale, offset = _c_f64(scale), _c_f64(offset)
        n_classes, _ = _zonal_classes(n_classes, c)
        code = dtype if isinstance(dtype, int) else DTYPE_CODES.get(np.dtype(dtype), -1)
        check(load().sknnr_zonal_from_values(self.handle, c_void_p(values_ptr or None), c_void_p(zones_ptr or None), int(n),
                                             int(c), code, _host_ptr(scale), _host_ptr(offset), int(n_zones),
                                             _host_ptr(n_classes), c_void_p(acc_ptr or None), c_void_p(hist_ptr or None),
                                             int(bool(accumulate)), MEM_DEVICE, c_void_p(stream or None)))

    ZONAL_RECORD = ("ran", "pixels", "c", "tallied", "nan", "outside", "other", "global_atomics")

    def debug_last_zonal(self) -> dict:
        """Debug only (sknnr_debug_last_zonal; synchronises the device): the last :meth:`zonal_from_values_host` /
        ``_device`` call, or the open zonal stream so far -- ran, pixels, c, entries tallied, NaN entries, pixels outside
        ``[0, n_zones)``, class values outside their range, global atomics issued on the accumulators."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_zonal(self.handle, out))
        return dict(zip(self.ZONAL_RECORD, (int(v) for v in out)))

    # ---- distance domain (include/sknnr_hip.h, "Distance domain") -----------------------------
    def domain_from_neighbors_host(self, dist, table, rank=1, threshold=None, acc=None, want_codes=True):
        """Percentile codes of ``dist`` ``(nq, k)`` float64 at ``rank`` within the sorted ``table``, and the accumulators
        (sknnr_domain_from_neighbors on host arrays).  ``acc`` ``(103,)`` int64: an array to ADD to (``accumulate = 1``);
        None: a fresh one.  ``want_codes=False``: tallies only, and the codes come back None.  Returns ``(codes, acc)``."""
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        if dist.ndim != 2:
            raise ValueError("dist must be (nq, k)")
        nq, k = dist.shape
        table, m, has_thr, thr = _domain_args(table, threshold)
        accumulate = acc is not None
        if accumulate:
            if acc.dtype != np.int64 or acc.shape != (DOMAIN_ACC,) or not acc.flags.c_contiguous:
                raise ValueError(f"acc must be C-contiguous int64 ({DOMAIN_ACC},)")
        else:
            acc = np.empty(DOMAIN_ACC, dtype=np.int64)
        codes = np.empty(nq, dtype=np.uint8) if want_codes else None
        check(load().sknnr_domain_from_neighbors(self.handle, _host_ptr(dist), nq, k, int(rank), _host_ptr(table), m, has_thr,
                                                 thr, _host_ptr(codes), _host_ptr(acc), int(accumulate), MEM_HOST, None))
        return codes, acc

    def domain_from_neighbors_device(self, dist_ptr, nq, k, table, rank, threshold, codes_ptr, acc_ptr, accumulate=False,
                                     stream=0):
        """sknnr_domain_from_neighbors on device pointers: enqueues on ``stream`` and returns.  ``table`` is a host array,
        as in the host form; ``codes_ptr`` 0: tallies only."""
        table, m, has_thr, thr = _domain_args(table, threshold)
        check(load().sknnr_domain_from_neighbors(self.handle, c_void_p(dist_ptr or None), int(nq), int(k), int(rank),
                                                 _host_ptr(table), m, has_thr, thr, c_void_p(codes_ptr or None),
                                                 c_void_p(acc_ptr or None), int(bool(accumulate)), MEM_DEVICE,
                                                 c_void_p(stream or None)))

    DOMAIN_RECORD = ("ran", "pixels", "k", "rank", "m", "nodata", "global_atomics", "blanked")

    def debug_last_domain(self) -> dict:
        """Debug only (sknnr_debug_last_domain; synchronises the device): the last :meth:`domain_from_neighbors_host` /
        ``_device`` call, or the open domain stream so far -- ran, pixels, k, rank, m, nodata pixels, global atomics issued
        on the accumulators, prediction rows blanked by the mask."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_domain(self.handle, out))
        return dict(zip(self.DOMAIN_RECORD, (int(v) for v in out)))

    # ---- per-target neighbour summaries (include/sknnr_hip.h) --------------------------------
    def summarize_host(self, q, opts: QueryOpts, stat, nq=None):
        """Search plus per-target statistic (sknnr_summarize) on host rows, or on the index's own rows (``q`` None)."""
        q = _c_rows(q, opts)
        if q is not None:
            nq = q.shape[0]
        stat = _c_stat(stat)
        out = np.empty((nq, self.t), dtype=np.float64)
        check(load().sknnr_summarize(self.handle, _host_ptr(q), nq, byref(opts), _host_ptr(stat), _host_ptr(out),
                                     None, None, MEM_HOST, None))
        return out

    def summarize_device(self, q_ptr, nq, opts: QueryOpts, stat, out_ptr, stream=0):
        stat = _c_stat(stat)
        check(load().sknnr_summarize(self.handle, c_void_p(q_ptr or None), nq, byref(opts), _host_ptr(stat),
                                     c_void_p(out_ptr), None, None, MEM_DEVICE, c_void_p(stream or None)))

    def summarize_from_neighbors_host(self, dist, idx, w, weight_mode, stat):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        dist, w, stat = _c_f64(dist), _c_f64(w), _c_stat(stat)
        nq, k = idx.shape
        out = np.empty((nq, self.t), dtype=np.float64)
        check(load().sknnr_summarize_from_neighbors(self.handle, _host_ptr(dist), _host_ptr(idx), _host_ptr(w), nq, k,
                                                    int(weight_mode), _host_ptr(stat), _host_ptr(out), MEM_HOST, None))
        return out

    def summarize_from_neighbors_device(self, dist_ptr, idx_ptr, w_ptr, nq, k, weight_mode, stat, out_ptr, stream=0):
        """Device pointers in and out; ``stat`` stays a host array of codes."""
        stat = _c_stat(stat)
        check(load().sknnr_summarize_from_neighbors(
            self.handle, c_void_p(dist_ptr or None), c_void_p(idx_ptr), c_void_p(w_ptr or None), nq, k,
            int(weight_mode), _host_ptr(stat), c_void_p(out_ptr), MEM_DEVICE, c_void_p(stream or None)))

    # ---- output plans (include/sknnr_hip.h) ------------------------------------------------------
    def summarize_plan_host(self, q, opts: QueryOpts, plan, nq=None):
        """Search plus output plan (sknnr_summarize_plan) on host rows, or on the index's own rows (``q`` None):
        ``(nq, n_out)`` float64.  ``plan``: ``(cols, codes, params)``."""
        q = _c_rows(q, opts)
        if q is not None:
            nq = q.shape[0]
        cols, codes, params = _c_plan(plan)
        out = np.empty((nq, cols.size), dtype=np.float64)
        check(load().sknnr_summarize_plan(self.handle, _host_ptr(q), nq, byref(opts), _host_ptr(cols), _host_ptr(codes),
                                          _host_ptr(params), int(cols.size), _host_ptr(out), None, None, MEM_HOST, None))
        return out

    def summarize_plan_device(self, q_ptr, nq, opts: QueryOpts, plan, out_ptr, stream=0):
        cols, codes, params = _c_plan(plan)
        check(load().sknnr_summarize_plan(self.handle, c_void_p(q_ptr or None), nq, byref(opts), _host_ptr(cols),
                                          _host_ptr(codes), _host_ptr(params), int(cols.size), c_void_p(out_ptr), None, None,
                                          MEM_DEVICE, c_void_p(stream or None)))

    def summarize_plan_from_neighbors_host(self, dist, idx, w, weight_mode, plan):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        dist, w = _c_f64(dist), _c_f64(w)
        cols, codes, params = _c_plan(plan)
        nq, k = idx.shape
        out = np.empty((nq, cols.size), dtype=np.float64)
        check(load().sknnr_summarize_plan_from_neighbors(
            self.handle, _host_ptr(dist), _host_ptr(idx), _host_ptr(w), nq, k, int(weight_mode), _host_ptr(cols),
            _host_ptr(codes), _host_ptr(params), int(cols.size), _host_ptr(out), MEM_HOST, None))
        return out

    def summarize_plan_from_neighbors_device(self, dist_ptr, idx_ptr, w_ptr, nq, k, weight_mode, plan, out_ptr, stream=0):
        """Device pointers in and out; the plan stays host arrays."""
        cols, codes, params = _c_plan(plan)
        check(load().sknnr_summarize_plan_from_neighbors(
            self.handle, c_void_p(dist_ptr or None), c_void_p(idx_ptr), c_void_p(w_ptr or None), nq, k, int(weight_mode),
            _host_ptr(cols), _host_ptr(codes), _host_ptr(params), int(cols.size), c_void_p(out_ptr), MEM_DEVICE,
            c_void_p(stream or None)))

    PLAN_FIELDS = ("ran", "path", "rows", "n_out", "k", "n_mean", "predict_ran", "reserved")

    def debug_last_plan(self) -> dict:
        """Debug only: the plan side of the last reduction of the handle (sknnr_debug_last_plan): whether the plan kernel
        ran, its path (1 registers, 2 wide), rows, n_out, k, the mean entries, and whether the predict kernels ran."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_plan(self.handle, out))
        return dict(zip(self.PLAN_FIELDS, (int(v) for v in out)))

    SUMMARY_FIELDS = ("path", "rows", "cols", "k", "predict_ran", "t", "weight_mode", "reserved")

    def debug_last_summary(self) -> dict:
        """Debug only: the last reduction of the handle (sknnr_debug_last_summary): the summary kernel that ran (0 none,
        1 registers, 2 wide), rows, the columns it handled, k, and whether the predict kernels ran."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_summary(self.handle, out))
        return dict(zip(self.SUMMARY_FIELDS, (int(v) for v in out)))

    WEIGHT_LAW_FIELDS = ("law", "rows", "k", "ran", "r4", "r5", "r6", "r7")

    def debug_last_weight_law(self) -> dict:
        """Debug only: the weight-law side of the last reduction of the handle (sknnr_debug_last_weight_law): the law's
        code (0 none), rows, k, and whether the law kernel ran for it."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_weight_law(self.handle, out))
        return dict(zip(self.WEIGHT_LAW_FIELDS, (int(v) for v in out)))

    # ---- nodata rows (include/sknnr_hip.h, "nodata rows") -----------------------------------
    def kneighbors_masked_host(self, q, opts: QueryOpts, nodata, fill_index=-1, return_distance=True):
        """``(dist, idx, n_valid)`` of the rows ``q`` with the rows that hold a nodata value masked on the device: they
        get ``fill_index`` / NaN, the others what the unmasked call gives for ``q[valid]``."""
        q = _c_rows(q, opts)
        nodata = _c_f64(nodata)
        nq, k = q.shape[0], opts.n_neighbors
        idx = np.empty((nq, k), dtype=np.int64)
        dist = np.empty((nq, k), dtype=np.float64) if return_distance else None
        nv = c_int64(0)
        check(load().sknnr_kneighbors_masked(self.handle, _host_ptr(q), nq, byref(opts), _host_ptr(nodata),
                                             int(fill_index), _host_ptr(dist), _host_ptr(idx), MEM_HOST, None, byref(nv)))
        return dist, idx, int(nv.value)

    def predict_masked_host(self, q, opts: QueryOpts, nodata, fill_index=-1, return_neighbors=False):
        q = _c_rows(q, opts)
        nodata = _c_f64(nodata)
        nq, k = q.shape[0], opts.n_neighbors
        pred = np.empty((nq, self.t), dtype=np.float64)
        dist = idx = None
        if return_neighbors:
            dist = np.empty((nq, k), dtype=np.float64)
            idx = np.empty((nq, k), dtype=np.int64)
        nv = c_int64(0)
        check(load().sknnr_predict_masked(self.handle, _host_ptr(q), nq, byref(opts), _host_ptr(nodata), int(fill_index),
                                          _host_ptr(pred), _host_ptr(dist), _host_ptr(idx), MEM_HOST, None, byref(nv)))
        return (pred, dist, idx, int(nv.value)) if return_neighbors else (pred, int(nv.value))

    def kneighbors_masked_device(self, q_ptr, nq, opts: QueryOpts, nodata, fill_index, dist_ptr, idx_ptr, stream=0) -> int:
        """Device pointers in and out (``nodata`` stays a host array); returns the valid rows.  Synchronises ``stream``
        once, for the 8-byte read of that count."""
        nodata = _c_f64(nodata)
        nv = c_int64(0)
        check(load().sknnr_kneighbors_masked(self.handle, c_void_p(q_ptr or None), nq, byref(opts), _host_ptr(nodata),
                                             int(fill_index), c_void_p(dist_ptr or None), c_void_p(idx_ptr), MEM_DEVICE,
                                             c_void_p(stream or None), byref(nv)))
        return int(nv.value)

    def predict_masked_device(self, q_ptr, nq, opts: QueryOpts, nodata, fill_index, pred_ptr, dist_ptr=0, idx_ptr=0,
                              stream=0) -> int:
        nodata = _c_f64(nodata)
        nv = c_int64(0)
        check(load().sknnr_predict_masked(self.handle, c_void_p(q_ptr or None), nq, byref(opts), _host_ptr(nodata),
                                          int(fill_index), c_void_p(pred_ptr), c_void_p(dist_ptr or None),
                                          c_void_p(idx_ptr or None), MEM_DEVICE, c_void_p(stream or None), byref(nv)))
        return int(nv.value)

    MASK_FIELDS = ("ran", "rows", "valid_rows", "path", "mask_blocks", "row_bytes", "valid_total", "reserved")

    def debug_last_mask(self) -> dict:
        """Debug only: the nodata front end of the last call's last tile (sknnr_debug_last_mask): whether the mask ran,
        the tile's rows and valid rows, the path (1: every row valid, searched in place; 2: every row masked, the fill
        alone; 0: compacted and expanded), workgroups of the mask kernel, bytes of a row, and the valid rows of the whole
        call or of the stream so far."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_mask(self.handle, out))
        return dict(zip(self.MASK_FIELDS, (int(v) for v in out)))

    NARROW_FIELDS = ("ran", "rows", "idx_dtype", "dist_dtype", "pred_dtype", "d2h_bytes", "wide_mask", "reserved")

    def debug_last_narrow(self) -> dict:
        """Debug only: the output side of the last tile of the host pipeline (sknnr_debug_last_narrow): whether a
        conversion kernel ran, the tile's rows, the sknnr_dtype of indices / distances / predictions (0: int64 / float64),
        the bytes its device-to-host copies moved, which outputs took the 4-elements-per-lane path (bit 0 indices,
        1 distances, 2 predictions), and, under the field's old name ``reserved``, whether its indices were crosswalked to dataframe ids on the device."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_narrow(self.handle, out))
        return dict(zip(self.NARROW_FIELDS, (int(v) for v in out)))

    # ---- device-pointer entry points (ints from tensor.data_ptr()) ------------------------
    def debug_last_planes(self) -> dict:
        """Debug only: the last tile of the host pipeline (sknnr_debug_last_planes): whether its rows arrived as planes
        and were packed on the device, its shape, and whether (and how many) result planes were written there."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_planes(self.handle, out))
        keys = ("planes_in", "rows", "cols", "elem_bytes", "planes_out", "out_planes", "chunk_cols")
        return {key: int(out[i]) for i, key in enumerate(keys)}

    def kneighbors_device(self, q_ptr, nq, opts: QueryOpts, dist_ptr, idx_ptr, stream=0):
        check(load().sknnr_kneighbors(self.handle, c_void_p(q_ptr or None), nq, byref(opts),
                                      c_void_p(dist_ptr or None), c_void_p(idx_ptr), MEM_DEVICE,
                                      c_void_p(stream or None)))

    def predict_device(self, q_ptr, nq, opts: QueryOpts, pred_ptr, dist_ptr=0, idx_ptr=0, stream=0):
        check(load().sknnr_predict(self.handle, c_void_p(q_ptr or None), nq, byref(opts),
                                   c_void_p(pred_ptr), c_void_p(dist_ptr or None),
                                   c_void_p(idx_ptr or None), MEM_DEVICE, c_void_p(stream or None)))

    def predict_from_neighbors_device(self, dist_ptr, idx_ptr, w_ptr, nq, k, weight_mode, pred_ptr,
                                      stream=0):
        check(load().sknnr_predict_from_neighbors(
            self.handle, c_void_p(dist_ptr or None), c_void_p(idx_ptr), c_void_p(w_ptr or None), nq, k,
            int(weight_mode), c_void_p(pred_ptr), MEM_DEVICE, c_void_p(stream or None)))

    def hamming_distances_host(self, q, rows=None):
        """Full weighted-Hamming distance rows ``(len(rows), n_ref)`` of the query rows ``q[rows]`` (``q`` None: of the
        index's own rows), computed on the device in the reference's float64 arithmetic (sknnr_hamming_distances)."""
        q = _c_f64(q)
        nq = self.n_ref if q is None else q.shape[0]
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        n_rows = nq if rows is None else rows.size
        out = np.empty((n_rows, self.n_ref), dtype=np.float64)
        check(load().sknnr_hamming_distances(self.handle, _host_ptr(q), nq, _host_ptr(rows), n_rows, _host_ptr(out),
                                             MEM_HOST, None))
        return out

    # ---- reference-sharded search (include/sknnr_hip.h) -------------------------------------------
    def shard_candidates_host(self, q, opts: QueryOpts, index_offset=0):
        q = _c_f64(q)
        nq, k = q.shape[0], opts.n_neighbors
        val = np.empty((nq, k), dtype=np.float64)
        idx = np.empty((nq, k), dtype=np.int64)
        check(load().sknnr_shard_candidates(self.handle, _host_ptr(q), nq, byref(opts), int(index_offset),
                                            _host_ptr(val), _host_ptr(idx), MEM_HOST, None))
        return val, idx

    def shard_candidates_device(self, q_ptr, nq, opts: QueryOpts, index_offset, val_ptr, idx_ptr, stream=0):
        check(load().sknnr_shard_candidates(self.handle, c_void_p(q_ptr), nq, byref(opts), int(index_offset),
                                            c_void_p(val_ptr), c_void_p(idx_ptr), MEM_DEVICE, c_void_p(stream or None)))

    def merge_shards_host(self, q, opts: QueryOpts, shard_val, shard_idx, nq=None, return_distance=True):
        q = _c_f64(q)
        shard_val = _c_f64(shard_val)
        shard_idx = np.ascontiguousarray(shard_idx, dtype=np.int64)
        n_shards = shard_val.shape[0]
        if q is not None:
            nq = q.shape[0]
        k = opts.n_neighbors
        idx = np.empty((nq, k), dtype=np.int64)
        dist = np.empty((nq, k), dtype=np.float64) if return_distance else None
        check(load().sknnr_merge_shards(self.handle, _host_ptr(q), nq, byref(opts), n_shards, _host_ptr(shard_val),
                                        _host_ptr(shard_idx), _host_ptr(dist), _host_ptr(idx), MEM_HOST, None))
        return dist, idx

    def merge_shards_device(self, q_ptr, nq, opts: QueryOpts, n_shards, val_ptr, sidx_ptr, dist_ptr, idx_ptr, stream=0):
        check(load().sknnr_merge_shards(self.handle, c_void_p(q_ptr or None), nq, byref(opts), n_shards, c_void_p(val_ptr),
                                        c_void_p(sidx_ptr), c_void_p(dist_ptr or None), c_void_p(idx_ptr), MEM_DEVICE,
                                        c_void_p(stream or None)))

    # ---- diagnostics ------------------------------------------------------------------------
    def debug_coarse_matrix(self, q):
        q = _c_f64(q)
        nq = q.shape[0]
        out = np.empty((nq, self.n_ref), dtype=np.float32)
        qn = np.empty(nq, dtype=np.float64)
        s, eps = c_double(), c_double()
        check(load().sknnr_debug_coarse_matrix(self.handle, _host_ptr(q), nq, _host_ptr(out),
                                               _host_ptr(qn), byref(s), byref(eps)))
        return out, qn, s.value, eps.value

    PREFILTER_FIELDS = ("generation", "ks", "m_list", "rank_extra", "bulk_waves", "bulk_rows", "thin_rows", "cell_depth")

    def debug_last_prefilter(self) -> dict:
        """The Euclidean pre-filter launches of the last call's last device chunk (sknnr_debug_last_prefilter):
        generation (0: none, 1: coarse_kernel, 2: coarse2_kernel), K-steps, list length, rank beyond the list, waves of the
        bulk launch, rows of the bulk and of the 4-wave thin launch, cell depth of the query order (0: plain order)."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_prefilter(self.handle, out))
        return dict(zip(self.PREFILTER_FIELDS, (int(v) for v in out)))

    FINALIZE_FIELDS = ("lanes_per_query", "record", "truncated_rows", "reserved")

    def debug_last_finalize(self) -> dict:
        """Debug only: the finaliser of the last call's last device chunk (sknnr_debug_last_finalize): lanes per query
        (8: finalize_record_kernel, 16 / 32 / 64: finalize_kernel, 0: none), whether merged candidate records were used, and
        the rows their truncation rule handed to the exact scan over the call."""
        out = (c_int64 * 4)()
        check(load().sknnr_debug_last_finalize(self.handle, out))
        return dict(zip(self.FINALIZE_FIELDS, (int(v) for v in out)))

    HAMMING_FIELDS = ("ran", "kk", "compacts", "seed_rows", "band", "tree_pairs", "chunks", "handed_to_scan")

    def debug_last_hamming(self) -> dict:
        """Debug only: the integer Hamming pre-filter of the last call (sknnr_debug_last_hamming): whether it ran, kk,
        compaction on, rows of the seeding pass, band, tree pairs, device chunks, and the rows it handed to the exact scan
        over the call (all zero when it did not run).  Under the forest map: the last forest chunk."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_hamming(self.handle, out))
        return dict(zip(self.HAMMING_FIELDS, (int(v) for v in out)))

    SCAN_FIELDS = ("formula_plus_1", "chunked", "kk", "workgroups", "lds_bytes", "rows", "slices", "replayed_rows")

    def debug_last_scan(self) -> dict:
        """Debug only: the float64 exact scan of the last call (sknnr_debug_last_scan): formula + 1 (0: no scan ran), the
        column-chunked instantiation, kk, workgroups and dynamic LDS bytes of the first scan launch, rows offered (the
        call's, or the fail list's device count), slices per pass (1: not sliced; the shard count after a shard merge), and
        the rows the merge filed for the sequential replay."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_scan(self.handle, out))
        return dict(zip(self.SCAN_FIELDS, (int(v) for v in out)))

    RESCUE_FIELDS = ("launched", "ks", "offered", "not_rescuable", "overflowed", "rescued", "handed_on", "rescued_total")

    def debug_last_rescue(self) -> dict:
        """Debug only: the rescue re-sweep of the last call (sknnr_debug_last_rescue): whether it was launched, K-steps, the
        rows the finalisers listed (offered), those without a threshold, those with more than 16 rows under their bound,
        the rows rescued and the rows handed on to the exact scan; and the rows rescued since the last reset_stats()."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_rescue(self.handle, out))
        return dict(zip(self.RESCUE_FIELDS, (int(v) for v in out)))

    def debug_hamming_candidates(self, n: int):
        """Debug only: ``(cnt, ids)`` the integer Hamming pre-filter wrote for the first ``n`` rows of the last call's last
        device chunk (sknnr_debug_hamming_candidates); ``ids`` is ``(n, 192)``, row i's candidates in ``ids[i, :cnt[i]]``."""
        cnt = np.empty(n, dtype=np.int32)
        ids = np.empty((n, 192), dtype=np.int32)
        check(load().sknnr_debug_hamming_candidates(self.handle, _host_ptr(cnt), _host_ptr(ids), int(n)))
        return cnt, ids

    def debug_coarse_candidates(self, n: int):
        """Debug only: ``(val, pos, perm)`` the first-generation Euclidean pre-filter wrote for the first ``n`` rows of the last call's last
        device chunk (sknnr_debug_coarse_candidates): ``(n, 2, M)`` float32 ranking values and int32 image positions as
        stored (lane half 0's list first; -1: sentinel or unused slot), and the first-generation position -> row table."""
        m = self.debug_last_prefilter()["m_list"]
        val = np.empty((n, 2, m), dtype=np.float32)
        pos = np.empty((n, 2, m), dtype=np.int32)
        perm = np.empty(self.n_ref, dtype=np.int32)
        check(load().sknnr_debug_coarse_candidates(self.handle, int(n), _host_ptr(val), _host_ptr(pos), _host_ptr(perm)))
        return val, pos, perm

    PREP_FIELDS = ("kernel", "rows_per_block", "x_dtype", "nq", "nq_pad", "xt_written", "cells_by", "affine_bits")

    def debug_last_prep(self) -> dict:
        """Debug only: the query preparation launch of the last call's last device chunk (sknnr_debug_last_prep): kernel
        (0: none, 1: prep_queries_direct_kernel, 2: prep_queries_kernel), rows per block, element type, live and padded
        rows, whether the transformed rows were written, who named the cells (0: not bucketed, 1: the preparation kernel,
        2: cell_assign_kernel) and the parts of the affine map in use (1 center | 2 scale | 4 proj)."""
        out = (c_int64 * 8)()
        check(load().sknnr_debug_last_prep(self.handle, out))
        return dict(zip(self.PREP_FIELDS, (int(v) for v in out)))

    def debug_query_prep(self, n: int, want=("qimg", "qnc", "xt", "cell", "perm", "qnc_pos")) -> dict:
        """Debug only: what the preparation and bucketing kernels wrote for the first ``n`` rows (positions) of the last
        call's last device chunk (sknnr_debug_query_prep), the buffers named in ``want``: ``qimg`` (n, 64 ks) uint8,
        ``qnc`` (n), ``xt`` (min(n, live rows), d), ``cell`` (n) uint8, ``perm`` (n) int32, ``qnc_pos`` (n)."""
        n = int(n)
        ks = (self.d + 15) // 16
        nq = self.debug_last_prep()["nq"]
        out = {}
        if "qimg" in want:
            out["qimg"] = np.empty((n, 64 * ks), dtype=np.uint8)
        if "qnc" in want:
            out["qnc"] = np.empty(n, dtype=np.float64)
        if "xt" in want:
            out["xt"] = np.empty((min(n, nq), self.d), dtype=np.float64)
        if "cell" in want:
            out["cell"] = np.empty(n, dtype=np.uint8)
        if "perm" in want:
            out["perm"] = np.empty(n, dtype=np.int32)
        if "qnc_pos" in want:
            out["qnc_pos"] = np.empty(n, dtype=np.float64)
        check(load().sknnr_debug_query_prep(self.handle, n, *(_host_ptr(out.get(name)) for name in
                                                              ("qimg", "qnc", "xt", "cell", "perm", "qnc_pos"))))
        return out

    def debug_image_constants(self) -> dict:
        """Debug only: the host-built constants of the preparation and bucketing kernels (sknnr_debug_image_constants):
        ``mu`` (16 ks), ``s``, ``cell_depth``, and with a cell tree ``axes`` (depth, d), ``centre`` (d), ``thr`` (2^depth - 1)
        float32 (without one: empty arrays)."""
        ks = (self.d + 15) // 16
        mu = np.empty(16 * ks, dtype=np.float64)
        s, depth = c_double(), c_int32()
        check(load().sknnr_debug_image_constants(self.handle, _host_ptr(mu), byref(s), byref(depth), None, None, None))
        axes = np.empty((depth.value, self.d), dtype=np.float32)
        centre = np.empty(self.d if depth.value else 0, dtype=np.float32)
        thr = np.empty((1 << depth.value) - 1, dtype=np.float32)
        check(load().sknnr_debug_image_constants(self.handle, None, None, None, _host_ptr(axes), _host_ptr(centre),
                                                 _host_ptr(thr)))
        return dict(mu=mu, s=s.value, cell_depth=int(depth.value), axes=axes, centre=centre, thr=thr)


class QueryStream:
    """Owner of one ``sknnr_stream*``: host tiles in, host results out, the PCIe pipeline kept full
    across pushes (see include/sknnr_hip.h).  Output arrays handed to :meth:`push` are filled at the
    latest when :meth:`flush` / :meth:`close` returns; the object keeps them alive until then."""

    def __init__(self, index: Index, opts: QueryOpts, want_dist=True, want_pred=False):
        self._index = index
        self._h = c_void_p()
        self._keep = []
        self.k = opts.n_neighbors
        self._opts = opts
        self.want_dist, self.want_pred = bool(want_dist), bool(want_pred)
        # element types of the results (set_output narrows them)
        self.idx_dtype, self.dist_dtype, self.pred_dtype = np.dtype(np.int64), np.dtype(np.float64), np.dtype(np.float64)
        self._typed = False
        self.pred_cols = index.t  # columns of the prediction lane (set_plan widens it)
        self._tally = False
        self._zonal = None  # (n_zones, elements of hist per zone) once set_zonal was called
        self._domain = False
        self._domain_out = None  # the code plane named for the next push (next_domain_out)
        self._idx_by_default = True  # a push that predicts nothing delivers the indices even unasked
        self._begin(index, opts)

    def _begin(self, index, opts):
        check(load().sknnr_stream_begin(index.handle, byref(opts), int(self.want_dist), int(self.want_pred),
                                        byref(self._h)))

    def configure(self, *, nodata=None, fill_index=-1, output=None, statistic=None, id_table=None, fill_id=-1, plan=None,
                  tally=False, zonal=None, domain=None, bootstrap=None):
        """Every ``set_*`` a fresh stream was asked for (the keywords of :meth:`Index.open_stream`), in the one order they
        work in, for a search stream and a replay alike (a replay has no ``nodata``).  Returns the stream; a refusal
        closes it."""
        try:
            if plan is not None:  # (first: it sets the width set_output's scale / offset must have)
                self.set_plan(plan)
            if bootstrap is not None:  # (likewise)
                self.set_bootstrap(*bootstrap)
            if nodata is not None:
                self.set_nodata(nodata, fill_index)
            if output:
                self.set_output(**output)
            if statistic is not None:
                self.set_statistics(statistic)
            if id_table is not None:
                self.set_id_table(id_table, fill_id)
            if tally:
                self.set_tally()
            if zonal is not None:  # (behind the plan: n_classes holds one value per plane)
                self.set_zonal(*zonal)
            if domain is not None:
                self.set_domain(*domain)
        except Exception:
            self.close()
            raise
        return self

    def _push(self, native, tile, nq, planes, out_idx, out_dist, out_pred, need_idx):
        """Push one tile of ``nq`` pixels through ``native`` (a row push, or with ``planes`` a band-first one): the missing
        outputs are allocated, the given ones validated -- ``(nq, cols)`` rows, or ``(cols, nq)`` planes that share one
        stride -- and all of them kept alive while the tile may be in the pipeline."""
        outs, strides = [], set()  # (strides in ELEMENTS of each output's own type: the outputs share the pixel axis, not the byte count)
        for a, dt, cols, wanted in ((out_idx, self.idx_dtype, self.k, need_idx or (self._idx_by_default and not self.want_pred)),
                                    (out_dist, self.dist_dtype, self.k, self.want_dist),
                                    (out_pred, self.pred_dtype, self.pred_cols, self.want_pred)):
            if a is None and wanted:
                a = np.empty((cols, nq) if planes else (nq, cols), dtype=dt)
            if a is not None and planes:
                if a.dtype != dt or a.shape != (cols, nq) or (nq > 1 and a.strides[1] != dt.itemsize):
                    raise ValueError(f"output arrays must be ({cols}, {nq}) {np.dtype(dt)} with contiguous planes")
                if cols > 1:  # (a single plane has no stride to speak of)
                    strides.add(a.strides[0] / dt.itemsize)
            elif a is not None and (a.dtype != dt or not a.flags.c_contiguous or a.shape != (nq, cols)):
                raise ValueError(f"output arrays must be C-contiguous ({nq}, {cols}) {np.dtype(dt)}")
            outs.append(a)
        if len(strides) > 1 or any(st != int(st) or st < nq for st in strides):
            raise ValueError("output arrays must share one stride between planes, of at least the tile's pixels")
        out_idx, out_dist, out_pred = outs
        stride = (int(strides.pop()) if strides else nq,) if planes else ()
        check(native(self._h, tile, nq, _host_ptr(out_dist), _host_ptr(out_idx), _host_ptr(out_pred), *stride))
        if self._domain_out is not None:  # (the library consumed it with this push)
            outs.append(self._domain_out)
            self._domain_out = None
        self._keep.append(outs)
        if len(self._keep) > 8:
            del self._keep[:-8]  # older tiles have left the pipeline (four slots: at most the last four pushes are pending)
        return out_idx, out_dist, out_pred

    def push(self, q, out_idx=None, out_dist=None, out_pred=None, need_idx=True):
        """Answer the rows of ``q``; returns the (idx, dist, pred) arrays that will hold the results
        (the ones passed in, or fresh ones; ``need_idx=False`` with predictions skips the indices)."""
        q = _c_rows(q, self._opts)
        native = load().sknnr_stream_push_typed if self._typed else load().sknnr_stream_push
        return self._push(native, _host_ptr(q), q.shape[0], False, out_idx, out_dist, out_pred, need_idx)

    def push_planes(self, bands, out_idx=None, out_dist=None, out_pred=None, need_idx=True):
        """Answer a band-first tile (sknnr_stream_push_planes): ``bands`` is a sequence of 1-D C-contiguous arrays of one
        length ``n`` and of the stream's element type, one per input column.  Returns the band-first (idx, dist, pred)
        arrays that will hold the results: ``(k, n)`` / ``(t, n)``, fresh ones, or the ones passed in -- those may be
        column windows ``a[:, r0:r0 + n]`` of a C-contiguous ``(k or t, N)`` array."""
        cols = self._index.d_in if self._opts.apply_affine else self._index.d
        want = next(dt for dt, code in DTYPE_CODES.items() if code == self._opts.query_dtype)
        bands = list(bands)
        if len(bands) != cols:
            raise ValueError(f"a band-first tile needs {cols} bands, got {len(bands)}")
        nq = bands[0].shape[0]
        for b in bands:
            if b.ndim != 1 or b.shape[0] != nq or b.dtype != want or not b.flags.c_contiguous:
                raise ValueError(f"every band must be a C-contiguous ({nq},) {want} array")
        ptrs = (c_void_p * cols)(*[b.ctypes.data for b in bands])
        native = load().sknnr_stream_push_planes_typed if self._typed else load().sknnr_stream_push_planes
        return self._push(native, ptrs, nq, True, out_idx, out_dist, out_pred, need_idx)

    def set_nodata(self, nodata, fill_index=-1):
        """Mask every pushed tile on the device (sknnr_stream_set_nodata; only before the first push)."""
        nodata = _c_f64(nodata).reshape(-1)
        cols = self._index.d_in if self._opts.apply_affine else self._index.d
        if nodata.size != cols:
            raise ValueError(f"nodata must hold one value per input column ({cols}), got {nodata.size}")
        check(load().sknnr_stream_set_nodata(self._h, _host_ptr(nodata), int(fill_index)))

    def set_statistics(self, stat):
        """One statistic code per target (sknnr_stream_set_statistics; only before the first push): the stream's
        predictions become those summaries of the neighbours."""
        stat = _c_stat(stat)
        check(load().sknnr_stream_set_statistics(self._h, _host_ptr(stat), int(stat.size)))

    def set_plan(self, plan):
        """An output plan ``(cols, codes, params)`` (sknnr_stream_set_plan; only before the first push, before
        :meth:`set_output`, and not together with :meth:`set_statistics`): the stream's predictions become its ``n_out``
        planes -- pushes take and return ``(nq, n_out)`` rows or ``(n_out, nq)`` planes."""
        cols, codes, params = _c_plan(plan)
        check(load().sknnr_stream_set_plan(self._h, _host_ptr(cols), _host_ptr(codes), _host_ptr(params), int(cols.size)))
        self.pred_cols = int(cols.size)

    def set_bootstrap(self, k, plan):
        """The bootstrap of the handle's table (:meth:`Index.set_bootstrap`) as the stream's reduction stage
        (sknnr_stream_set_bootstrap; only before the first push, before :meth:`set_output`, and not together with
        statistics, plans, the usage tally, zonal statistics or a domain): ``k`` copies per replicate out of the
        stream's ``self.k`` candidates, ``plan`` = ``(cols, codes)``; the predictions become its ``n_out`` planes."""
        cols, codes = _c_boot_plan(plan)
        check(load().sknnr_stream_set_bootstrap(self._h, int(k), _host_ptr(cols), _host_ptr(codes), int(cols.size)))
        self.pred_cols = int(cols.size)

    def bootstrap(self):
        """Flush, then the int64 pair (pixels reduced, valid replicates over them) of everything pushed so far
        (sknnr_stream_get_bootstrap)."""
        out = (c_int64 * 2)()
        check(load().sknnr_stream_get_bootstrap(self._h, out))
        self._keep.clear()
        return np.array([out[0], out[1]], dtype=np.int64)

    def set_output(self, index_dtype=None, distance_dtype=None, pred_dtype=None, scale=None, offset=None, fill=None):
        """The element types in which the results leave the device (sknnr_stream_set_output; only before the first
        push): ``index_dtype`` int32, ``distance_dtype`` float32, ``pred_dtype`` float32 / int16 / uint16 / uint8 / int32;
        None (or the wide type) leaves an output as it is.  ``scale`` / ``offset``: float64 ``(t,)`` each, both or
        neither -- the stored prediction is ``rint(pred * scale + offset)`` (no ``rint`` for float32), clamped to the
        type's range; ``fill``: what a NaN prediction becomes.  Pushes then take and return arrays of those types."""
        def code(dt, wide):
            dt = np.dtype(wide if dt is None else dt)
            if dt == np.dtype(wide):
                return dt, 0
            if not DTYPE_CODES.get(dt):
                raise ValueError(f"{dt} is no narrow output type of the library")
            return dt, DTYPE_CODES[dt]
        idt, ic = code(index_dtype, np.int64)
        ddt, dc = code(distance_dtype, np.float64)
        pdt, pc = code(pred_dtype, np.float64)
        if (scale is None) != (offset is None):
            raise ValueError("scale and offset come together")
        t = self.pred_cols
        if scale is not None:
            scale, offset = _c_f64(scale).reshape(-1), _c_f64(offset).reshape(-1)
            if scale.size != t or offset.size != t:
                raise ValueError(f"scale and offset must hold one value per target ({t})")
        check(load().sknnr_stream_set_output(self._h, ic, dc, pc, _host_ptr(scale), _host_ptr(offset),
                                             int(fill is not None), float(0.0 if fill is None else fill)))
        self.idx_dtype, self.dist_dtype, self.pred_dtype = idt, ddt, pdt
        self._typed = bool(ic or dc or pc)

    def set_id_table(self, table, fill_id=-1):
        """Dataframe ids on the device (sknnr_stream_set_id_table; only before the first push): ``table`` holds one
        int64 id per reference row, and the index output of every tile leaves as ``table[idx]``, negative indices (the
        ``fill_index`` of a nodata mask) as ``fill_id`` -- in the stream's index type, whose range they must fit."""
        table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1)
        check(load().sknnr_stream_set_id_table(self._h, _host_ptr(table), int(table.size), int(fill_id)))

    def set_tally(self):
        """Tally every tile's neighbours on the device (sknnr_stream_set_tally; only before the first push): per
        reference row and rank the rows it served, and its largest distance -- over valid rows only under a nodata
        mask.  What the pushes deliver is unchanged; :meth:`tally` reads the accumulators."""
        check(load().sknnr_stream_set_tally(self._h))
        self._tally = True

    def tally(self):
        """Flush, then ``(counts, max_dist)`` of everything pushed so far (sknnr_stream_get_tally): ``(n_ref, k)`` int64
        and ``(n_ref,)`` float64, 0.0 where a row was never used.  The accumulators keep running."""
        counts = np.empty((self._index.n_ref, self.k), dtype=np.int64)
        max_dist = np.empty(self._index.n_ref, dtype=np.float64)
        check(load().sknnr_stream_get_tally(self._h, _host_ptr(counts), _host_ptr(max_dist)))
        self._keep.clear()
        return counts, max_dist

    def set_zonal(self, n_zones, n_classes=None):
        """Tally every tile's predictions by zone on the device (sknnr_stream_set_zonal; only before the first push, after
        :meth:`set_plan`): over the stored values of the stream's integer ``pred_dtype``.  ``n_classes``: one class count
        per column of the prediction lane (0: numeric), or None.  Every push then needs :meth:`next_zones` first; what
        the pushes deliver is unchanged; :meth:`zonal` reads the accumulators."""
        n_classes, per_zone = _zonal_classes(n_classes, self.pred_cols)
        check(load().sknnr_stream_set_zonal(self._h, int(n_zones), _host_ptr(n_classes)))
        self._zonal = (int(n_zones), per_zone)

    def next_zones(self, zones):
        """The zone codes of the next push (sknnr_stream_next_zones): int32, one per pixel; the array is free on return."""
        zones = np.ascontiguousarray(zones, dtype=np.int32).reshape(-1)
        check(load().sknnr_stream_next_zones(self._h, _host_ptr(zones), int(zones.size)))

    def zonal(self):
        """Flush, then ``(acc, hist)`` of everything pushed so far (sknnr_stream_get_zonal): ``(n_zones, c, 6)`` int64 and
        the flat class blocks (None when no column has classes).  The accumulators keep running."""
        if self._zonal is None:
            raise ValueError("the stream has no zones: set_zonal was not called")
        n_zones, per_zone = self._zonal
        acc = np.empty((n_zones, self.pred_cols, ZONAL_FIELDS), dtype=np.int64)
        hist = np.empty(n_zones * per_zone, dtype=np.int64) if per_zone else None
        check(load().sknnr_stream_get_zonal(self._h, _host_ptr(acc), _host_ptr(hist)))
        self._keep.clear()
        return acc, hist

    def set_domain(self, table, rank=1, threshold=None, mask_beyond=False):
        """Code every tile's distances against the sorted ``table`` on the device (sknnr_stream_set_domain; only before the
        first push): per pixel the percentile of its ``rank``-th neighbour distance, tallied into 103 counters.
        ``mask_beyond`` (with predictions and a ``threshold``): the predictions of pixels beyond the threshold become NaN
        before they are converted or enter zonal tables.  :meth:`next_domain_out` names where a push's codes go;
        :meth:`domain` reads the accumulators."""
        table, m, has_thr, thr = _domain_args(table, threshold)
        check(load().sknnr_stream_set_domain(self._h, _host_ptr(table), m, int(rank), has_thr, thr, int(bool(mask_beyond))))
        self._domain = True

    def next_domain_out(self, out):
        """Where the next push's code plane goes (sknnr_stream_next_domain_out): a C-contiguous uint8 array with one
        element per pixel of that push, filled when the push's own outputs are; kept alive until then."""
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
            raise ValueError("the code plane must be a C-contiguous uint8 (n,) array")
        check(load().sknnr_stream_next_domain_out(self._h, _host_ptr(out), int(out.size)))
        self._domain_out = out if out.size else None

    def domain(self):
        """Flush, then the 103 int64 accumulators of everything pushed so far (sknnr_stream_get_domain): the histogram
        of codes 0 .. 100, the beyond pixels, the nodata pixels.  The accumulators keep running."""
        if not self._domain:
            raise ValueError("the stream has no domain: set_domain was not called")
        acc = np.empty(DOMAIN_ACC, dtype=np.int64)
        check(load().sknnr_stream_get_domain(self._h, _host_ptr(acc)))
        self._keep.clear()
        return acc

    def valid_rows(self) -> int:
        """Valid (unmasked) rows submitted so far; without a nodata mask, the rows pushed."""
        n = c_int64(0)
        check(load().sknnr_stream_valid_rows(self._h, byref(n)))
        return int(n.value)

    def flush(self):
        check(load().sknnr_stream_flush(self._h))
        self._keep.clear()

    def close(self) -> int:
        """Flush and free; returns the number of rows pushed."""
        if not self._h:
            return 0
        n = c_int64(0)
        h, self._h = self._h, c_void_p()
        code = load().sknnr_stream_end(h, byref(n))
        self._keep.clear()
        check(code)
        return int(n.value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.close()
        else:  # do not mask the original error
            try:
                self.close()
            except HipBackendError:
                pass

    def __del__(self):
        try:
            if self._h:
                load().sknnr_stream_end(self._h, None)
                self._h = c_void_p()
        except Exception:
            pass


class TargetIndex(Index):
    """Owner of an attribute-only ``sknnr_index*`` (sknnr_index_create_targets): a target table and nothing else.  The
    from-neighbours entries and replay streams accept it; whatever searches refuses it."""

    def __init__(self, y, device: int = 0):
        y2 = _c_f64(y)
        if y2.ndim == 1:
            y2 = y2.reshape(-1, 1)
        if y2.ndim != 2:
            raise ValueError("y must be 1-D or 2-D")
        self.n_ref, self.t = y2.shape
        self.d = self.d_in = 0
        self.device = device
        self._h = c_void_p()
        check(load().sknnr_index_create_targets(_host_ptr(y2), self.n_ref, self.t, device, byref(self._h)))


# stored neighbour types of a replay stream: numpy dtype -> the sknnr_replay_begin code
REPLAY_NO_DIST = -1
REPLAY_IDX_CODES = {np.dtype(np.int64): 0, np.dtype(np.int32): DTYPE_CODES[np.dtype(np.int32)]}
REPLAY_DIST_CODES = {np.dtype(np.float64): 0, np.dtype(np.float32): DTYPE_CODES[np.dtype(np.float32)]}


def replay_instance(idx_dtype, dist_dtype, planes: bool) -> int:
    """The decode instantiation ``Index.debug_last_replay()["instance"]`` names (sknnr_amd/csrc/replay.hip.h)."""
    dk = 0 if dist_dtype is None else (1 if np.dtype(dist_dtype) == np.float32 else 2)
    return (6 if np.dtype(idx_dtype) == np.int64 else 0) + 2 * dk + int(bool(planes))


class ReplayStream(QueryStream):
    """A stream whose tiles are stored neighbours (sknnr_replay_begin): every setter and getter of
    :class:`QueryStream` but :meth:`set_nodata` works on it unchanged."""

    def __init__(self, index, k, ks, weight_mode=0, weight_law=0, idx_dtype=np.int64, dist_dtype=None, fill_index=-1,
                 ids=False, want_dist=False, want_pred=True):
        self.ks = int(ks)
        self.store_idx = np.dtype(idx_dtype)
        self.store_dist = None if dist_dtype is None else np.dtype(dist_dtype)
        if self.store_idx not in REPLAY_IDX_CODES:
            raise ValueError(f"stored indices must be int32 or int64, got {self.store_idx}")
        if self.store_dist is not None and self.store_dist not in REPLAY_DIST_CODES:
            raise ValueError(f"stored distances must be float32 or float64, got {self.store_dist}")
        self._replay = (int(fill_index), bool(ids))
        opts = Index.make_opts(int(k))
        opts.weight_mode, opts.weight_law = int(weight_mode), int(weight_law)
        super().__init__(index, opts, want_dist=want_dist, want_pred=want_pred)
        self._idx_by_default = False

    def _begin(self, index, opts):
        fill_index, ids = self._replay
        dc = REPLAY_NO_DIST if self.store_dist is None else REPLAY_DIST_CODES[self.store_dist]
        check(load().sknnr_replay_begin(index.handle, opts.n_neighbors, self.ks, opts.weight_mode, opts.weight_law,
                                        REPLAY_IDX_CODES[self.store_idx], dc, fill_index, int(ids), int(self.want_dist),
                                        int(self.want_pred), byref(self._h)))

    def _stored(self, idx, dist, shape):
        """The tile's arrays as the push reads them: of the stream's stored types, C-contiguous, ``shape``."""
        if (dist is None) != (self.store_dist is None):
            raise ValueError("a tile carries distances exactly when the stream was opened with stored distances")
        out = []
        for a, dt in ((idx, self.store_idx), (dist, self.store_dist)):
            if a is None:
                out.append(None)
                continue
            a = np.asarray(a)
            if a.dtype != dt or a.shape != shape:
                raise ValueError(f"a stored tile must be {shape} {dt}, got {a.shape} {a.dtype}")
            out.append(np.ascontiguousarray(a))
        return out

    def push(self, idx, dist=None, out_idx=None, out_dist=None, out_pred=None, need_idx=False):
        """Replay the ``(n, ks)`` row tile ``idx`` (and ``dist``); returns the (idx, dist, pred) result arrays."""
        idx = np.asarray(idx)
        if idx.ndim != 2 or idx.shape[1] != self.ks:
            raise ValueError(f"a stored row tile must be (n, {self.ks}), got {idx.shape}")
        idx, dist = self._stored(idx, dist, idx.shape)
        lib = load()

        def native(h, tile, nq, od, oi, op):
            return lib.sknnr_replay_push(h, _host_ptr(tile[0]), _host_ptr(tile[1]), nq, od, oi, op)
        return self._push(native, (idx, dist), idx.shape[0], False, out_idx, out_dist, out_pred, need_idx)

    def push_planes(self, idx, dist=None, out_idx=None, out_dist=None, out_pred=None, need_idx=False):
        """Replay the band-first ``(ks, n)`` tile ``idx`` (and ``dist``); returns band-first result arrays."""
        idx = np.asarray(idx)
        if idx.ndim != 2 or idx.shape[0] != self.ks:
            raise ValueError(f"a stored band-first tile must be ({self.ks}, n), got {idx.shape}")
        idx, dist = self._stored(idx, dist, idx.shape)
        nq = idx.shape[1]
        lib = load()

        def native(h, tile, nq, od, oi, op, stride):
            return lib.sknnr_replay_push_planes(h, _host_ptr(tile[0]), _host_ptr(tile[1]), nq, nq, od, oi, op, stride)
        return self._push(native, (idx, dist), nq, True, out_idx, out_dist, out_pred, need_idx)

    def set_nodata(self, nodata, fill_index=-1):
        check(load().sknnr_stream_set_nodata(self._h, _host_ptr(_c_f64(nodata).reshape(-1)), int(fill_index)))

    def counts(self) -> dict:
        """Flush, then the pixels, masked and unknown pixels of the stream so far, and the first push that held unknown
        values (-1: none) (sknnr_replay_get_counts)."""
        out = (c_int64 * 4)()
        check(load().sknnr_replay_get_counts(self._h, out))
        self._keep.clear()
        return dict(zip(("pixels", "masked", "unknown", "first_unknown"), map(int, out)))


def affine_transform_host(x, center=None, scale=None, proj=None, device: int = 0) -> np.ndarray:
    """``((x - center) / scale) @ proj`` on the GPU (float64 fma chains), host in / host out."""
    x = _c_f64(x)
    center, scale, proj = _c_f64(center), _c_f64(scale), _c_f64(proj)
    n, d_in = x.shape
    d = d_in if proj is None else proj.shape[1]
    out = np.empty((n, d), dtype=np.float64)
    check(load().sknnr_affine_transform(_host_ptr(x), n, d_in, _host_ptr(center), _host_ptr(scale),
                                        _host_ptr(proj), d, _host_ptr(out), device))
    return out


def crosswalk_host(table, idx, device: int = 0):
    table = np.ascontiguousarray(table, dtype=np.int64)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    out = np.empty(idx.shape, dtype=np.int64)
    check(load().sknnr_crosswalk(_host_ptr(table), table.size, _host_ptr(idx), idx.size,
                                 _host_ptr(out), device, MEM_HOST, None))
    return out


def crosswalk_device(table_ptr, n_table, idx_ptr, n, out_ptr, device=0, stream=0):
    check(load().sknnr_crosswalk(c_void_p(table_ptr), n_table, c_void_p(idx_ptr), n, c_void_p(out_ptr),
                                 device, MEM_DEVICE, c_void_p(stream or None)))


def debug_weight_law_host(law: int, p0: float, p1: float, dist, device: int = 0) -> np.ndarray:
    """Debug only: the law kernel alone (sknnr_debug_weight_law) on a host array of distances of any shape; float64
    weights of that shape."""
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    out = np.empty_like(dist)
    check(load().sknnr_debug_weight_law(int(law), float(p0), float(p1), _host_ptr(dist), dist.size, _host_ptr(out),
                                        MEM_HOST, device))
    return out


def debug_weight_law_device(law: int, p0: float, p1: float, dist_ptr, n, out_ptr, device: int = 0) -> None:
    """The same on device pointers (default stream; returns when ``out`` is written)."""
    check(load().sknnr_debug_weight_law(int(law), float(p0), float(p1), c_void_p(dist_ptr or None), int(n),
                                        c_void_p(out_ptr or None), MEM_DEVICE, device))


def mask_rows_host(q, nodata, device: int = 0):
    """``(valid, n_valid)``: uint8 ``(nq,)`` with 1 for every row of ``q`` none of whose columns equals its nodata value
    (a NaN nodata value: is NaN), computed on the device (sknnr_mask_rows).  ``q`` keeps its dtype when the library reads
    it (:data:`DTYPE_CODES`), else it is converted to float64."""
    q = np.asarray(q)
    code = dtype_code(q.dtype)
    q = np.ascontiguousarray(q) if code is not None else np.ascontiguousarray(q, dtype=np.float64)
    nodata = _c_f64(nodata).reshape(-1)
    nq, d_in = q.shape
    if nodata.size != d_in:
        raise ValueError(f"nodata must hold {d_in} values, got {nodata.size}")
    valid = np.empty(nq, dtype=np.uint8)
    nv = c_int64(0)
    check(load().sknnr_mask_rows(_host_ptr(q), nq, d_in, code or 0, _host_ptr(nodata), device, MEM_HOST, None,
                                 _host_ptr(valid), byref(nv)))
    return valid, int(nv.value)


def mask_rows_device(q_ptr, nq, d_in, query_dtype, nodata, valid_ptr, device=0, stream=0) -> int:
    nodata = _c_f64(nodata).reshape(-1)
    nv = c_int64(0)
    check(load().sknnr_mask_rows(c_void_p(q_ptr), nq, d_in, int(query_dtype), _host_ptr(nodata), device, MEM_DEVICE,
                                 c_void_p(stream or None), c_void_p(valid_ptr), byref(nv)))
    return int(nv.value)


def debug_mask_compact(q_ptr, nq, d_in, query_dtype, nodata, packed_ptr, device=0, stream=0) -> dict:
    """Debug only: mask, scan and compaction alone on device pointers (sknnr_debug_mask_compact).  ``valid`` uint8
    ``(nq,)``, ``blk_off`` int32 per block of 256 rows, ``rank`` int32 ``(nq,)``, ``unit`` (bytes per copy) and
    ``n_valid``; the packed rows are written at ``packed_ptr``."""
    nodata = _c_f64(nodata).reshape(-1)
    if nodata.size != d_in:
        raise ValueError(f"nodata must hold {d_in} values, got {nodata.size}")
    valid = np.empty(nq, dtype=np.uint8)
    blk_off = np.empty((nq + 255) // 256, dtype=np.int32)
    rank = np.empty(nq, dtype=np.int32)
    unit, nv = c_int32(0), c_int64(0)
    check(load().sknnr_debug_mask_compact(c_void_p(q_ptr or None), nq, d_in, int(query_dtype), _host_ptr(nodata), device,
                                          c_void_p(stream or None), _host_ptr(valid), _host_ptr(blk_off), _host_ptr(rank),
                                          c_void_p(packed_ptr or None), byref(unit), byref(nv)))
    return {"valid": valid, "blk_off": blk_off, "rank": rank, "unit": int(unit.value), "n_valid": int(nv.value)}


def debug_expand_rows(nq, k, t, valid_ptr, rank_ptr, c_idx_ptr, c_dist_ptr, c_pred_ptr, idx_ptr, dist_ptr, pred_ptr,
                      fill_index=-1, stream=0) -> None:
    """Debug only: the expansion alone on device pointers (sknnr_debug_expand_rows); 0 / None is a null pointer."""
    ptrs = [c_void_p(p or None) for p in (valid_ptr, rank_ptr, c_idx_ptr, c_dist_ptr, c_pred_ptr, idx_ptr, dist_ptr,
                                          pred_ptr)]
    check(load().sknnr_debug_expand_rows(nq, k, t, *ptrs, int(fill_index), c_void_p(stream or None)))


def planes_to_rows_device(src_ptr, n, c, elem_bytes, src_stride, dst_ptr, device=0, stream=0) -> None:
    """``c`` planes of ``n`` elements of ``elem_bytes``, ``src_stride`` elements apart, to packed ``(n, c)`` rows, on
    device pointers (sknnr_planes_to_rows); enqueued on ``stream``."""
    check(load().sknnr_planes_to_rows(c_void_p(src_ptr or None), n, c, elem_bytes, src_stride, c_void_p(dst_ptr or None),
                                      device, c_void_p(stream or None)))


def rows_to_planes_device(src_ptr, n, c, dst_ptr, dst_stride, device=0, stream=0) -> None:
    """Packed ``(n, c)`` rows of 8-byte elements to ``c`` planes ``dst_stride`` elements apart, on device pointers
    (sknnr_rows_to_planes); enqueued on ``stream``."""
    check(load().sknnr_rows_to_planes(c_void_p(src_ptr or None), n, c, c_void_p(dst_ptr or None), dst_stride, device,
                                      c_void_p(stream or None)))


NARROW_VALUE, NARROW_INDEX = 0, 1


def narrow_device(src_ptr, kind, n, c, dst_ptr, dst_dtype, dst_stride=0, scale_ptr=0, offset_ptr=0, fill=None, device=0,
                  stream=0) -> bool:
    """A packed ``(n, c)`` float64 (``NARROW_VALUE``) or int64 (``NARROW_INDEX``) tile to ``dst_dtype`` (a numpy dtype or
    a sknnr_dtype code), packed rows (``dst_stride`` 0) or ``c`` planes ``dst_stride`` elements apart, on device pointers
    (sknnr_narrow); enqueued on ``stream``.  Returns whether the launch took the 4-elements-per-lane path."""
    code = dst_dtype if isinstance(dst_dtype, int) else DTYPE_CODES.get(np.dtype(dst_dtype), -1)
    wide = c_int32(0)
    check(load().sknnr_narrow(c_void_p(src_ptr or None), int(kind), n, c, c_void_p(dst_ptr or None), code, dst_stride,
                              c_void_p(scale_ptr or None), c_void_p(offset_ptr or None), int(fill is not None),
                              float(0.0 if fill is None else fill), device, c_void_p(stream or None), byref(wide)))
    return bool(wide.value)


def narrow_ids_device(src_ptr, n, c, table_ptr, n_table, dst_ptr, dst_dtype, dst_stride=0, fill_id=None, device=0,
                      stream=0) -> bool:
    """A packed ``(n, c)`` int64 index tile to the ids ``table[idx]`` (``fill_id`` for negatives; None: they pass through),
    as int64 or int32, packed rows (``dst_stride`` 0) or ``c`` planes ``dst_stride`` elements apart, on device pointers
    (sknnr_narrow_ids); enqueued on ``stream``.  Returns whether the launch took the 4-elements-per-lane path."""
    code = dst_dtype if isinstance(dst_dtype, int) else {np.dtype(np.int64): 0}.get(
        np.dtype(dst_dtype), DTYPE_CODES.get(np.dtype(dst_dtype), -1))
    wide = c_int32(0)
    check(load().sknnr_narrow_ids(c_void_p(src_ptr or None), n, c, c_void_p(table_ptr or None), n_table,
                                  int(fill_id is not None), int(0 if fill_id is None else fill_id),
                                  c_void_p(dst_ptr or None), code, dst_stride, device, c_void_p(stream or None),
                                  byref(wide)))
    return bool(wide.value)
