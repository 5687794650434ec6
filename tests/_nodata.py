"""What the nodata kernels write, restated on the host with numpy (no GPU needed).

tests/test_nodata_gpu.py compares ``sknnr_mask_rows`` with ``row_mask`` bit for bit and uses ``compact`` / ``expand`` to
state what a masked call must return; tests/test_nodata_kernels_gpu.py compares everything each kernel writes, run alone,
with this module; tests/test_nodata_cpu.py checks this module itself against plain boolean indexing.
Source: sknnr_amd/csrc/mask.hip.h.

- ``row_mask``: ``row_mask_kernel`` -- a row is masked when any column, widened exactly to float64, equals its nodata
  value; a NaN nodata value matches NaN.  Per block of ``BLOCK_ROWS`` rows one count of valid rows (``block_counts``).
- ``exclusive_scan``: ``mask_scan_kernel`` -- block offsets and the tile's valid count.
- ``ranks`` / ``compact``: ``row_compact_kernel`` -- rank of a row = its block's offset + the valid rows in front of it
  inside the block; valid rows are copied, as raw bytes and in order, to position rank.
- ``compact_unit``: ``launch::compact_unit`` (k_mask.hip) -- the bytes per copy of the compaction.
- ``expand``: ``row_expand_kernel`` -- a valid row takes row rank[row] of the packed results, a masked row the fills.
"""

from __future__ import annotations

import numpy as np

BLOCK_ROWS = 256  # kMaskRows
PATH_COMPACTED, PATH_IN_PLACE, PATH_ALL_MASKED = 0, 1, 2


def widen(x) -> np.ndarray:
    """The rows as the kernel compares them: float64, exact for every element type the library reads."""
    return np.asarray(x).astype(np.float64)


def row_mask(x, nodata) -> np.ndarray:
    """uint8 (nq,): 1 = valid.  ``nodata``: float64 (d_in,)."""
    v = widen(x)
    nd = np.asarray(nodata, dtype=np.float64).reshape(1, -1)
    assert nd.shape[1] == v.shape[1]
    hit = (v == nd) | (np.isnan(nd) & np.isnan(v))
    return (~hit.any(axis=1)).astype(np.uint8)


def mask_blocks(nq: int) -> int:
    return (nq + BLOCK_ROWS - 1) // BLOCK_ROWS


def block_counts(valid) -> np.ndarray:
    valid = np.asarray(valid, dtype=np.int64)
    pad = np.zeros(mask_blocks(valid.size) * BLOCK_ROWS, dtype=np.int64)
    pad[:valid.size] = valid
    return pad.reshape(-1, BLOCK_ROWS).sum(axis=1)


def exclusive_scan(counts):
    """(offsets, total) of the block counts."""
    counts = np.asarray(counts, dtype=np.int64)
    inc = np.cumsum(counts)
    return inc - counts, int(inc[-1]) if counts.size else 0


def ranks(valid) -> np.ndarray:
    """int64 (nq,): valid rows in front of each row, put together the kernel's way (block offset + rows in front inside
    the block)."""
    valid = np.asarray(valid, dtype=np.int64)
    offsets, _ = exclusive_scan(block_counts(valid))
    out = np.empty(valid.size, dtype=np.int64)
    for b in range(mask_blocks(valid.size)):
        blk = valid[b * BLOCK_ROWS:(b + 1) * BLOCK_ROWS]
        out[b * BLOCK_ROWS:b * BLOCK_ROWS + blk.size] = offsets[b] + np.cumsum(blk) - blk
    return out


def compact(x, valid) -> np.ndarray:
    """The packed rows: row r of ``x`` lands, byte for byte, at position ranks(valid)[r] when it is valid."""
    x = np.ascontiguousarray(x)
    valid = np.asarray(valid, dtype=bool)
    rk = ranks(valid)
    raw = x.view(np.uint8).reshape(x.shape[0], -1)
    out = np.zeros((int(valid.sum()), raw.shape[1]), dtype=np.uint8)
    out[rk[valid]] = raw[valid]
    return out.view(x.dtype).reshape(-1, x.shape[1])


def compact_unit(x_addr: int, out_addr: int, row_bytes: int) -> int:
    """Bytes per copy of the compaction: the largest power of two up to 16 that divides the row size and both base
    addresses -- the lowest set bit of their OR with 16."""
    bits = int(x_addr) | int(out_addr) | int(row_bytes) | 16
    return bits & -bits


def expand(valid, packed, fill) -> np.ndarray:
    """Full-layout rows from the packed results ``(n_valid, cols)``: masked rows hold ``fill``."""
    valid = np.asarray(valid, dtype=bool)
    packed = np.asarray(packed)
    rk = ranks(valid)
    out = np.full((valid.size,) + packed.shape[1:], fill, dtype=packed.dtype)
    out[valid] = packed[rk[valid]]
    return out


def expected_path(valid) -> int:
    n, nv = len(valid), int(np.sum(valid))
    return PATH_IN_PLACE if nv == n else (PATH_ALL_MASKED if nv == 0 else PATH_COMPACTED)


MASK_KINDS = ("none", "all", "first", "last", "alternating", "block_run", "random30")


def make_mask(kind: str, nq: int, seed: int = 0) -> np.ndarray:
    """bool (nq,): True = the row is to be MASKED."""
    m = np.zeros(nq, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "block_run":  # a run covering exactly one block of the kernels (the second one where there is one)
        start = BLOCK_ROWS if nq >= 2 * BLOCK_ROWS else 0
        m[start:start + BLOCK_ROWS] = True
    elif kind == "random30":
        m = np.random.default_rng(seed).random(nq) < 0.3
    elif kind != "none":
        raise ValueError(kind)
    return m


def blob_mask(nq: int, fraction: float, seed: int = 0, mean_len: int = 2000) -> np.ndarray:
    """bool (nq,): about ``fraction`` of the rows masked in contiguous runs (cloud / water blobs of a raster)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(nq, dtype=bool)
    if fraction >= 1.0:
        m[:] = True
        return m
    target = int(fraction * nq)
    while m.sum() < target:
        a = int(rng.integers(0, nq))
        m[a:a + int(rng.integers(1, 2 * mean_len))] = True
    return m
