"""Which float64 exact-scan launches a call makes, restated from the host code (no GPU needed).

tests/test_scan_instances_gpu.py asserts that ``Index.debug_last_scan()`` reports exactly what ``expected_scan`` predicts
and that the slice merge hands exactly ``expected_replays`` rows to the sequential replay.  When the scan's dispatch changes
in the library, these restatements stop matching and the instance tests fail loudly instead of quietly testing another
launch.  Sources, all in sknnr_amd/csrc:

- ``scan_qpw``, ``scan_nq``, ``scan_layout`` / ``scan_block_bytes``, ``scan_slices``, ``kScanWaves``, ``kScanRefs``,
  ``kScanColChunk``, ``kScanSliceMaxKK``, ``kScanMaxSlices`` and the slice bounds of ``exact_scan_kernel``: exact.hip.h
- ``kScanGridWg``, ``kScanMaxKK``, the 150 KiB refusal and the chunked rule of ``launch_scan``, the grid of
  ``launch_scan_formula``, the replay launch of ``merge_shards_formula``: sknnr_hip.hip
- the merge's uniqueness rule (``scan_merge_kernel``) is not restated here: ``oracle.merge_shards`` states it for shards,
  and a slice is a shard (``expected_replays``)
"""

from __future__ import annotations

import numpy as np

EXPANDED, DIRECT, HAMMING = 0, 1, 2
FORMULA_NAMES = {EXPANDED: "expanded", DIRECT: "direct", HAMMING: "hamming"}

SCAN_WAVES = 4              # kScanWaves
SCAN_REFS = 512             # kScanRefs = 2 * kScanWaves * 64: reference rows per step
COL_CHUNK = 1024            # kScanColChunk: query columns held in LDS at a time
SLICE_MAX_KK = 32           # kScanSliceMaxKK: more neighbours (+ self) than this are never sliced
MAX_SLICES = 32             # kScanMaxSlices
GRID_WG = 1024              # kScanGridWg = 256 * 4
MAX_KK = 192                # kScanMaxKK
LDS_LIMIT = 150 * 1024      # launch_scan / merge_shards_formula refuse more dynamic LDS than this
MAX_SHARDS = 64             # sknnr_merge_shards
REFUSAL = "does not fit the exact scan kernel"

RECORD_FIELDS = ("formula_plus_1", "chunked", "kk", "workgroups", "lds_bytes", "rows", "slices", "replayed_rows")


def scan_qpw(formula: int) -> int:
    return 3 if formula == EXPANDED else 2


def scan_nq(formula: int) -> int:
    return SCAN_WAVES * scan_qpw(formula)


def scan_layout(d: int, kk: int, nq: int) -> dict:
    """xs[NQ][dpad] | qn[NQ] | hv[NQ][KK] | hi[NQ][kkp] | stack[NQ][stk] | (16-byte aligned) d2[NQ][kScanRefs]"""
    dpad = (min(d, COL_CHUNK) + 1) & ~1
    kkp = kk + (kk & 1)
    stk = (2 * kk + 4 + 1) & ~1
    out = dict(dpad=dpad, kkp=kkp, stk=stk)
    b = 0
    for name, size in (("xs", 8 * nq * dpad), ("qn", 8 * nq), ("hv", 8 * nq * kk), ("hi", 4 * nq * kkp), ("stack", 4 * nq * stk)):
        out[name] = b
        b += size
    b = (b + 15) & ~15
    out["d2"] = b
    out["total"] = b + 8 * nq * SCAN_REFS
    return out


def scan_block_bytes(d: int, kk: int, formula: int) -> int:
    return scan_layout(d, kk, scan_nq(formula))["total"]


def fits(d: int, kk: int, formula: int) -> bool:
    return scan_block_bytes(d, kk, formula) <= LDS_LIMIT


def chunked(d: int) -> bool:
    return d > COL_CHUNK


def n_steps(n_ref: int) -> int:
    return (n_ref + SCAN_REFS - 1) // SCAN_REFS


def scan_slices(n_items: int, nq_pass: int, n_ref: int, kk: int, grid_wg: int = GRID_WG) -> int:
    passes = (n_items + nq_pass - 1) // nq_pass
    if passes <= 0 or kk > SLICE_MAX_KK:
        return 1
    sl = min(grid_wg // passes, MAX_SLICES, n_steps(n_ref))
    return 1 if sl < 2 else sl


def may_slice(formula: int, n_ref: int, kk: int) -> bool:
    """launch_scan_formula provides the slice buffers (and launches the whole grid) when one pass could be sliced."""
    return kk <= SLICE_MAX_KK and scan_slices(1, scan_nq(formula), n_ref, kk) > 1


def scan_grid(formula: int, n_ref: int, kk: int, max_items: int) -> int:
    """Workgroups of the first exact_scan_kernel launch of launch_scan_formula (max_items: the call's rows, also when the
    scan serves a fail list)."""
    if may_slice(formula, n_ref, kk):
        return GRID_WG
    passes = (max_items + scan_nq(formula) - 1) // scan_nq(formula)
    return max(1, min(passes, GRID_WG))


def slice_bounds(n_ref: int, S: int) -> list[tuple[int, int]]:
    """Reference rows [begin, end) of each of the S slices of a pass: whole steps of 512 rows, the last one cut at n_ref."""
    steps = n_steps(n_ref)
    return [(min(s * steps // S * SCAN_REFS, n_ref), min((s + 1) * steps // S * SCAN_REFS, n_ref)) for s in range(S)]


def largest_kk_that_fits(d: int, formula: int) -> int:
    """The largest kk <= kScanMaxKK whose workgroup image passes the 150 KiB check at this width (0: none)."""
    best = 0
    for kk in range(1, MAX_KK + 1):
        if fits(d, kk, formula):
            best = kk
    return best


def lds_boundary(d: int, formula: int) -> tuple[int, int | None]:
    """(largest accepted kk, smallest refused kk or None when kScanMaxKK itself fits).  scan_block_bytes grows with kk, so
    the two are neighbours."""
    ok = largest_kk_that_fits(d, formula)
    assert all(fits(d, kk, formula) for kk in range(1, ok + 1))
    return ok, (None if ok == MAX_KK else ok + 1)


def expected_scan(formula: int, n_ref: int, d: int, kk: int, nq: int, listed: int | None = None, replays: int = 0,
                  shards: int | None = None) -> dict:
    """What debug_last_scan() reports after one call of ``nq`` rows searching ``kk`` neighbours (k + 1 for X=None) on an
    index of ``n_ref`` x ``d`` rows that the exact scan serves: every row, or the ``listed`` rows of the fail list (the
    device's count: the caller reads it from the record).  ``replays``: rows the slice merge hands on (``expected_replays``).
    ``shards``: the call is sknnr_merge_shards over that many shards -- the only scan launch is the replay."""
    assert fits(d, kk, formula), "the call is refused: no record"
    f_nq = scan_nq(formula)
    rows = nq if listed is None else listed
    rec = dict(formula_plus_1=formula + 1, chunked=int(chunked(d)), kk=kk, lds_bytes=scan_block_bytes(d, kk, formula), rows=rows)
    if shards is not None:
        rec.update(workgroups=max(1, min((nq + f_nq - 1) // f_nq, GRID_WG)), slices=shards, replayed_rows=replays)
    else:
        S = scan_slices(rows, f_nq, n_ref, kk) if may_slice(formula, n_ref, kk) else 1
        assert S > 1 or replays == 0
        rec.update(workgroups=scan_grid(formula, n_ref, kk, nq), slices=S, replayed_rows=replays)
    return {name: rec[name] for name in RECORD_FIELDS}


def no_scan() -> dict:
    return dict.fromkeys(RECORD_FIELDS, 0)


# ---------------------------------------------------------------------------------------------------------------------
# slices as shards
# ---------------------------------------------------------------------------------------------------------------------
def slice_candidates(fit_X, Xq, kk: int, formula: int, bounds, w=None):
    """(S, nq, kk) values and indices: each slice's kk smallest (squared distance | Hamming distance, index), as
    oracle.shard_candidates gives them with index_offset = the slice start.  A slice of fewer than kk rows leaves the other
    slots unfilled: +inf, index -1 (the device keeps DBL_MAX there and the merge skips it)."""
    from oracle import oracle as O

    nq = len(Xq)
    val = np.full((len(bounds), nq, kk), np.inf)
    idx = np.full((len(bounds), nq, kk), -1, dtype=np.int64)
    for s, (a, b) in enumerate(bounds):
        m = min(kk, b - a)
        if m <= 0:
            continue
        if formula == HAMMING:
            v, i = O.argkmin_hamming(Xq, fit_X[a:b], w, m)  # ascending by (distance, index) already
            i = i + a
        else:
            v, i = O.shard_candidates(fit_X[a:b], Xq, m, FORMULA_NAMES[formula], index_offset=a)
        val[s, :, :m], idx[s, :, :m] = v, i
    return val, idx


def merge_slices(fit_X, X, k: int, formula: int, bounds, deterministic=True, decimals=10, row_offset=0, nq=None, w=None,
                 lists=None):
    """The device's slice merge on the CPU: (dist, idx, rows handed to the sequential replay) of a call whose passes are
    split at ``bounds`` (``X`` None: the X=None path on rows [row_offset, row_offset + nq) of the index).  Expanded and
    direct: oracle.merge_shards.  Hamming: the union of the slices' lists by (distance, index) is the answer, no row is
    handed on (scan_merge_kernel applies the uniqueness rule to the expanded formula alone).  ``lists``: the result of
    ``slice_candidates`` for these rows and bounds, when the caller has it already."""
    from oracle import oracle as O

    fit_X = np.ascontiguousarray(fit_X, dtype=np.float64)
    self_rows = X is None
    kk = k + (1 if self_rows else 0)
    Xq = fit_X[row_offset:row_offset + nq] if self_rows else np.ascontiguousarray(X, dtype=np.float64)
    sv, si = lists if lists is not None else slice_candidates(fit_X, Xq, kk, formula, bounds, w)
    if formula != HAMMING:
        return O.merge_shards(fit_X, None if self_rows else Xq, sv, si, k, FORMULA_NAMES[formula], deterministic, decimals, row_offset)
    v = np.moveaxis(sv, 0, 1).reshape(len(Xq), -1)
    i = np.moveaxis(si, 0, 1).reshape(len(Xq), -1)
    order = np.lexsort((i, v), axis=1)[:, :kk]
    dist, idx = np.take_along_axis(v, order, 1), np.take_along_axis(i, order, 1)
    if self_rows:
        dist, idx = O.drop_self(dist, idx, row_offset)
    if deterministic:
        dist, idx = O.deterministic_reorder(dist, idx, decimals, row_offset)
    return dist, idx, 0


def expected_replays(fit_X, X, k: int, formula: int, S: int, **kw) -> int:
    """Rows scan_merge_kernel must file for the sequential replay when a call's passes are split into S slices (0 when
    S = 1: nothing is merged).  The first two results of the merge must equal oracle.kneighbors: the caller checks that."""
    if S <= 1:
        return 0
    return merge_slices(fit_X, X, k, formula, slice_bounds(len(fit_X), S), **kw)[2]
