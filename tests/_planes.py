"""Host restatement of the band-first transpositions (sknnr_amd/csrc/planes.hip.h), in numpy.

Both directions work on element views of a flat buffer, with the plane side's stride in ELEMENTS, exactly as the C ABI
states them (sknnr_planes_to_rows / sknnr_rows_to_planes); on such views each is one line.  The kernels move raw bytes,
so the restatement is applied to unsigned integer views of the element size and compared byte for byte.

The host makes no choice of a wider access unit for these kernels (every global access is one element wide); what it
does choose is the column chunk a workgroup handles, 128 bytes of a row, restated here as :func:`chunk_cols` and checked
against a hand-written table, because the tests pick their column counts around it.
"""

from __future__ import annotations

import numpy as np

BLOCK_ROWS = 256     # pixels per workgroup (kPlanesRows)
CHUNK_BYTES = 128    # bytes of a row per workgroup (kPlanesChunkBytes)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def planes_to_rows(src, n, c, stride):
    """``src``: 1-D element array holding ``c`` planes of ``n`` elements, plane ``j`` at ``j * stride``.  Returns the
    packed ``(n, c)`` rows."""
    return np.ascontiguousarray(np.lib.stride_tricks.as_strided(src, (c, n), (stride * src.itemsize, src.itemsize)).T)


def rows_to_planes(rows, dst, stride):
    """``rows``: ``(n, c)``; writes plane ``j`` at ``dst[j * stride : j * stride + n]`` of the 1-D element array ``dst``
    and leaves every other element alone."""
    n, c = rows.shape
    np.lib.stride_tricks.as_strided(dst, (c, n), (stride * dst.itemsize, dst.itemsize))[...] = rows.T


def chunk_cols(elem_bytes):
    """Columns one workgroup handles (planes_chunk_cols)."""
    return CHUNK_BYTES // elem_bytes


# written out by hand: element bytes -> columns per chunk.  (This pins the helper above; the kernel's own chunk is read
# back through sknnr_debug_last_planes and compared with the helper in tests/test_raster_layout_gpu.py.)
CHUNK_TABLE = {1: 128, 2: 64, 4: 32, 8: 16}
