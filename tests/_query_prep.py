"""What the query preparation and bucketing kernels write, restated on the host (no GPU needed).

tests/test_query_prep_gpu.py compares every buffer these launches fill with the arrays built here, bit for bit, and the
launch record ``Index.debug_last_prep()`` with ``expected_prep``; tests/test_query_prep_cpu.py checks this module itself
against exact rational arithmetic.  Sources, all in sknnr_amd/csrc:

- dispatch: ``launch_prep`` and ``bucket_chunk`` (sknnr_hip.hip)
- transformed rows, image, query norm: ``prep_queries_direct_kernel``, ``prep_queries_kernel`` (exact.hip.h); the rows are
  ``oracle.affine`` of the input widened exactly to float64 (one k-ordered fma chain per output; without ``proj``: subtract,
  then divide)
- image layout: ``qimg_index`` (coarse.hip.h): [row][hi | lo][K-step][K half] pieces of 16 bytes
- cells: ``cell_of`` / ``cell_assign_kernel`` (bucket.hip.h) through ``oracle.cell_assign`` (C ``fmaf``)
- the counting sort (``cell_count_kernel``, ``cell_scatter_kernel``) leaves the order inside a cell open: ``check_bucketing``
  states everything it does promise

The constants ``mu``, ``s`` and the cell tree come from ``Index.debug_image_constants()``: the index build sums ``mu`` in long
double, which numpy does not reproduce.
"""

from __future__ import annotations

import numpy as np

import _prefilter_dispatch as P

ROW_QUANTUM = P.ROW_QUANTUM
IMAGE_LIMIT = 32768.0        # kImageLimit: |b| at or above it has no image, qnc = +inf
LDS_LIMIT = 150 * 1024       # launch_prep: bytes of the LDS kernel's row tile
KERNEL_DIRECT, KERNEL_LDS = 1, 2
CELLS_NONE, CELLS_BY_PREP, CELLS_BY_ASSIGN = 0, 1, 2
UNSUPPORTED_MESSAGE = "d_in = {d_in} is too wide for the query preparation kernel (max 299)"


def padded_rows(nq: int) -> int:
    return (nq + ROW_QUANTUM - 1) // ROW_QUANTUM * ROW_QUANTUM


def lds_rows_per_block(d_in: int) -> int | None:
    """Rows per block of prep_queries_kernel for rows of ``d_in`` columns (row stride d_in | 1 doubles), None: refused."""
    for bt in (256, 128, 64):
        if bt * (d_in | 1) * 8 <= LDS_LIMIT:
            return bt
    return None


def expected_prep(d: int, nq: int, *, d_in: int | None = None, center=False, scale=False, proj=False, x_dtype: int = 0,
                  prep_lds: bool = False, bucketed: bool = False) -> dict | None:
    """What debug_last_prep() reports after one Euclidean call of ``nq`` rows (one device chunk, kk <= 31, d <= 128).
    ``d_in``: columns of the rows when the call applies the index's affine map (``center`` / ``scale`` / ``proj``: its parts),
    None without one.  ``prep_lds``: SKNNR_PREP_LDS is set.  ``bucketed``: the call's pre-filter runs in the cell order
    (``_prefilter_dispatch.expected_launch(...)["cell_depth"] > 0``).  None: the library refuses the call."""
    ks = P.ks_of(d)
    assert 1 <= ks <= 8
    affine = d_in is not None
    width = d_in if affine else d
    if ks <= 4 and not prep_lds:
        kernel, rows = KERNEL_DIRECT, 256
    else:
        kernel, rows = KERNEL_LDS, lds_rows_per_block(width)
        if rows is None:
            return None
    cells = CELLS_NONE if not bucketed else (CELLS_BY_PREP if kernel == KERNEL_DIRECT else CELLS_BY_ASSIGN)
    bits = (1 if center else 0) | (2 if scale else 0) | (4 if proj else 0) if affine else 0
    return dict(kernel=kernel, rows_per_block=rows, x_dtype=x_dtype, nq=nq, nq_pad=padded_rows(nq),
                xt_written=int(affine or x_dtype != 0), cells_by=cells, affine_bits=bits)


def qimg_index(row: int, part: int, ks: int, step: int, kh: int) -> int:
    """Index of a 16-byte piece of the image (coarse.hip.h, qimg_index): part 0 = hi, 1 = lo; K half kh of K-step step."""
    return ((row * 2 + part) * ks + step) * 2 + kh


def widen(x) -> np.ndarray:
    """The rows as float64: exact for every element type the kernels take (float32, int16, uint16, uint8, int32)."""
    x = np.asarray(x)
    assert x.dtype in (np.float64, np.float32, np.int16, np.uint16, np.uint8, np.int32)
    return np.ascontiguousarray(x, dtype=np.float64)


def transformed_rows(x, center=None, scale=None, proj=None) -> np.ndarray:
    from oracle import oracle

    xw = widen(x)
    if center is None and scale is None and proj is None:
        return xw
    return oracle.affine(xw, center, scale, proj)


def scaled_rows(xt, mu, s, nq_pad: int) -> np.ndarray:
    """b = s (xt - mu) in float64, (nq_pad, 16 ks): zero beyond column d and on the padding rows."""
    nq, d = xt.shape
    b = np.zeros((nq_pad, len(mu)), dtype=np.float64)
    b[:nq, :d] = s * (xt - mu[:d])
    return b


def split_f16(b):
    """hi = f16(f32(b)), lo = f16(f32(b - f64(hi))): the kernel's two roundings each."""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = b.astype(np.float32).astype(np.float16)
        lo = (b - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
    return hi, lo


def image_bytes(b) -> np.ndarray:
    """The image rows as the kernels store them: (rows, 64 ks) uint8."""
    rows, dp = b.shape
    ks = dp // 16
    hi, lo = split_f16(b)
    pieces = np.zeros((rows * 4 * ks, 8), dtype=np.uint16)
    row = np.arange(rows)
    for part, h in enumerate((hi.view(np.uint16), lo.view(np.uint16))):
        for step in range(ks):
            for kh in range(2):
                k0 = (2 * step + kh) * 8
                pieces[qimg_index(row, part, ks, step, kh)] = h[:, k0:k0 + 8]
    return pieces.reshape(rows, 4 * ks * 8).view(np.uint8)


def query_norms(b) -> np.ndarray:
    """qnc: the fma chain of b * b over all 16 ks columns; +inf when any !(|b| < 32768)."""
    from oracle import oracle

    with np.errstate(over="ignore", invalid="ignore"):
        qn = oracle.row_norms(b)
        overflow = ~(np.abs(b) < IMAGE_LIMIT)
    qn[overflow.any(axis=1)] = np.inf
    return qn


def cells(xt, consts, nq_pad: int) -> np.ndarray:
    """qcell after the counting sort: the live rows' cells, the last cell on the padding rows."""
    from oracle import oracle

    depth = consts["cell_depth"]
    out = np.full(nq_pad, (1 << depth) - 1, dtype=np.uint8)
    out[:len(xt)] = oracle.cell_assign(xt, consts["axes"], consts["centre"], consts["thr"])
    return out


def restate(x, consts, *, center=None, scale=None, proj=None, bucketed=False) -> dict:
    """Every buffer one call's preparation fills for the rows ``x`` (as handed to the call): ``xt`` (nq, d), ``qimg``
    (nq_pad, 64 ks) uint8, ``qnc`` (nq_pad), and for a bucketed call ``cell`` (nq_pad)."""
    xt = transformed_rows(x, center, scale, proj)
    nq_pad = padded_rows(len(xt))
    b = scaled_rows(xt, consts["mu"], consts["s"], nq_pad)
    out = dict(xt=xt, qimg=image_bytes(b), qnc=query_norms(b))
    if bucketed:
        out["cell"] = cells(xt, consts, nq_pad)
    return out


def check_bucketing(perm, cell, nq: int, depth: int, qnc=None, qnc_pos=None) -> None:
    """Everything the counting sort promises about ``perm`` (position -> row) given the final ``cell`` array."""
    n_pad = len(perm)
    perm = np.asarray(perm, dtype=np.int64)
    assert len(cell) == n_pad
    np.testing.assert_array_equal(np.sort(perm), np.arange(n_pad), err_msg="perm is not a permutation of [0, nq_pad)")
    np.testing.assert_array_equal(perm[nq:], np.arange(nq, n_pad), err_msg="padding positions must map to themselves")
    by_pos = cell[perm[:nq]].astype(np.int64)
    assert (np.diff(by_pos) >= 0).all(), "cells are not non-decreasing along the positions"
    assert (cell[nq:] == (1 << depth) - 1).all(), "padding rows must sit in the last cell"
    if qnc_pos is not None:
        np.testing.assert_array_equal(qnc_pos, qnc[perm], err_msg="qnc_pos[p] != qnc[perm[p]]")
