"""numpy restatement of the typed-output conversions (sknnr_amd/csrc/narrow.hip.h; include/sknnr_hip.h, "typed outputs")
and of the host's choice between the two access widths.  Shared by test_narrow_cpu.py, test_narrow_kernels_gpu.py and
test_typed_outputs_gpu.py."""

from __future__ import annotations

import numpy as np

VALUE, INDEX = 0, 1
VALUE_DTYPES = tuple(np.dtype(t) for t in (np.float32, np.int16, np.uint16, np.uint8, np.int32))


def narrow_values(v, dtype, scale=None, offset=None, fill=None):
    """float64 ``v`` of shape ``(..., c)`` to ``dtype``.  ``x = v * scale + offset`` (two float64 roundings; ``x = v``
    without them); integers: NaN first -> ``fill`` (0 without one), else ``rint``, clamp, cast; float32: NaN -> ``fill``
    when one is given, else ``astype``."""
    dt = np.dtype(dtype)
    x = np.asarray(v, dtype=np.float64)
    if scale is not None:
        x = x * np.asarray(scale, dtype=np.float64)  # (rounded to float64 here ...)
        x = x + np.asarray(offset, dtype=np.float64)  # (... and here: no fma)
    if dt.kind == "f":
        with np.errstate(over="ignore"):
            out = x.astype(dt)
        if fill is not None:
            out = np.where(np.isnan(x), dt.type(fill), out)
        return out
    info = np.iinfo(dt)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(x), info.min, info.max)
        return np.where(np.isnan(x), 0 if fill is None else fill, r).astype(dt)


def narrow_indices(idx, dtype=np.int32):
    return np.asarray(idx, dtype=np.int64).astype(dtype)


def narrow(src, kind, dtype, scale=None, offset=None, fill=None):
    return narrow_indices(src, dtype) if kind == INDEX else narrow_values(src, dtype, scale, offset, fill)


def to_planes(rows, out, stride):
    """Packed ``(n, c)`` rows into ``out`` (1-D, the destination's elements): plane j at ``j * stride``; the gaps between
    planes are left as they are."""
    n, c = rows.shape
    for j in range(c):
        out[j * stride:j * stride + n] = rows[:, j]


def wide_ok(src_addr, dst_addr, dst_bytes, n, c, stride):
    """The host's choice of the 4-elements-per-lane path (narrow_wide_ok): every 4-element store aligned to its own size.
    Packed (stride 0): the source 16-byte aligned for the two loads, one full group of 4.  Planes: every plane base
    aligned, i.e. the stride a multiple of 4 elements (workgroups start at multiples of 256 pixels)."""
    if dst_addr % (4 * dst_bytes):
        return False
    if stride == 0:
        return src_addr % 16 == 0 and n * c >= 4
    return stride % 4 == 0 and n >= 4


# (v, scale, offset, two roundings, one rounding): v * scale is inexact in float64 and the offset cancels it, so the
# product's rounding error is the whole result and a fused multiply-add, which rounds once, ends elsewhere
FMA_CASES = [
    (2.0**26 + 1, 2.0**27 + 1, -(2.0**53 + 2.0**27 + 2.0**26), 0.0, 1.0),       # the product is a tie, rounded to even
    (2.0**26 + 3, 2.0**27 + 1, -(2.0**53 + 3 * 2.0**27 + 2.0**26), 4.0, 3.0),   # the tie rounds up
    (0.1, 3.0, -0.30000000000000004, 0.0, -2.7755575615628914e-17),             # shows in float32 only
    (1 / 3, 3.0, -1.0, 0.0, -5.551115123125783e-17),
]
