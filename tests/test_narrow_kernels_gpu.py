"""The conversion kernels of the typed outputs (sknnr_amd/csrc/narrow.hip.h), run alone through the handle-free entry
point ``sknnr_narrow`` on torch device buffers and compared with the numpy restatement (tests/_narrow.py) by
``assert_array_equal`` over the WHOLE destination buffer: every output byte, the 64 guard bytes in front of and behind
it, the gaps between output planes and the slack behind the guard.  The scheme is that of test_planes_kernels_gpu.py.

Every case also checks the access width the host chose (``*out_wide``) against the restated choice
(``_narrow.wide_ok``), and runs at destinations 0, 1, 2 and 3 elements behind a 16-byte boundary: the first takes the
4-elements-per-lane path wherever the stride and the count allow it, the others are bases at which that path's stores
would be misaligned, and the element path is forced there.  The source of packed cases is moved 8 bytes off its 16-byte
boundary in every second case, which forces the element path at an aligned destination.

Source values encode (pixel, column), within the destination type's range so that the clamp keeps them apart: uint8
``(p * c + j) mod 251``, the 16-bit types ``mod 65521`` (int16 shifted down by 32700), int32 / float32 ``p * c + j + 1``,
each plus 0.25 for the integer types (so that ``rint`` has work to do); indices ``(j + 1) << 20 | (p + 1)``.  Cases
with scale / offset divide the source by a per-column power of two and add a per-column integer back.

Groups:

* ``test_shapes_and_alignment``: n of {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513, 1000} x c of {1, 2, 3, 5, 7, 15,
  16, 17, 33, 35} x strides {0 (packed), n, n + 1, n + 13}, each at the four destination offsets; the six conversions
  (values to float32 / int16 / uint16 / uint8 / int32, indices to int32) and scale / offset rotate over the cases.
* ``test_special_values``: per type, half-way values on even and odd neighbours, both range ends and +-1 and +-0.5
  around them, +-inf, NaN with and without a fill, -0.0, +-1e300; float32: overflow to inf, the largest float32 and the
  tie above it, subnormal results, the tie below the smallest subnormal, ties to even both ways; indices 0, 2^31 - 1,
  -1, -2^31.  Packed and as planes, both access widths.
* ``test_two_roundings_on_the_device``: the scale / offset cases of ``_narrow.FMA_CASES``, in which an fma would differ.

Measured on an MI355X: the 535 cases of this module take 4.9 s, of which 3.4 s are the first case's device set-up; no
other case takes more than 0.1 s.

Scratch mutations of narrow.hip.h (never committed; every buffer of this module carries slack for 256 more rows, so each
keeps every access inside its buffer) and the cases that fail under them, of 535:

=====================================================================  ======  ==========================================
mutation                                                               failed  where
=====================================================================  ======  ==========================================
the NaN test moved behind the clamp (the clamp written with                 8  test_special_values, the four integer
fmin / fmax, which turn NaN into a range end)                                  types, with and without a fill
fma(v, scale, offset) for the two roundings                                 3  test_two_roundings_on_the_device, all types
round() -- half away from zero -- for rint()                                8  test_special_values, the four integer types
the wide path chosen without looking at the addresses                     219  every case with a shifted destination or
                                                                               source -- on the access-width assertion
the tail block's row bound replaced by the block size (rows = 256)        374  360 of the 390 plane cases of
                                                                               test_shapes_and_alignment (all but n = 256),
                                                                               11 special-value and 3 two-rounding cases
=====================================================================  ======  ==========================================

Two of these need a remark.  The kernel's clamp is a pair of compare-selects, through which a NaN passes unchanged, so
moving the NaN test alone changes nothing; the order matters as soon as the clamp is written with fmin / fmax, and that is
the mutation that was run.  Under the forced wide path every output byte was still right: the MI355X serves 4-, 8- and
16-byte global accesses at any element-aligned address, so the data comparison cannot see a misaligned base.  What pins
the host's choice is the comparison of ``*out_wide`` with the restated choice, which failed in all 219 cases; the
comparison of the bytes comes first in ``run_narrow`` so that a run shows which of the two broke.
"""

from __future__ import annotations

import numpy as np
import pytest

import _narrow as NR

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
NS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513, 1000)
CS = (1, 2, 3, 5, 7, 15, 16, 17, 33, 35)
STRIDES = ("packed", 0, 1, 13)  # packed rows, or planes n + pad apart
SHIFTS = (0, 1, 2, 3)           # destination elements behind a 16-byte boundary
# (kind, destination type)
CONVERSIONS = [(NR.VALUE, np.float32), (NR.VALUE, np.int16), (NR.VALUE, np.uint16), (NR.VALUE, np.uint8),
               (NR.VALUE, np.int32), (NR.INDEX, np.int32)]
BLOCK_ROWS = 256


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


def encoded(n, c, kind, dtype):
    """(n, c) float64 / int64 rows whose converted values name (pixel, column)."""
    p = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(c, dtype=np.int64)[None, :]
    if kind == NR.INDEX:
        return ((j + 1) << 20) | (p + 1)
    dt = np.dtype(dtype)
    if dt == np.uint8:
        v = (p * c + j) % 251
    elif dt == np.uint16:
        v = (p * c + j) % 65521
    elif dt == np.int16:
        v = (p * c + j) % 65521 - 32700
    else:
        v = p * c + j + 1
    return v.astype(np.float64) + (0.25 if dt.kind != "f" else 0.0)


def to_device(host_bytes):
    import torch

    t = torch.from_numpy(host_bytes).cuda()
    assert t.data_ptr() % 16 == 0, "the allocator's bases are 16-byte aligned"
    return t


def run_narrow(N, rows, kind, dtype, stride, shift, src_off8=0, scale=None, offset=None, fill=None, what=""):
    """``rows``: (n, c) float64 / int64.  ``stride``: 0 for packed rows, else the elements between planes.  The
    destination starts ``shift`` elements behind a 16-byte boundary, the source ``src_off8`` bytes behind one.  Compares
    the whole destination buffer with the restatement; returns whether the wide path ran."""
    import torch

    n, c = rows.shape
    dt = np.dtype(dtype)
    esz = dt.itemsize
    rows = np.ascontiguousarray(rows)
    slack = BLOCK_ROWS * (c + 1) * 8
    s_off = GUARD + src_off8
    src = np.full(s_off + rows.nbytes + slack, 0xEE, dtype=np.uint8)
    src[s_off:s_off + rows.nbytes] = rows.view(np.uint8).reshape(-1)
    d_off = GUARD + shift * esz
    extent = (n * c if stride == 0 else (c - 1) * stride + n) * esz
    want = np.full(d_off + extent + GUARD + slack, PATTERN, dtype=np.uint8)
    d_src, d_out = to_device(src), to_device(want.copy())
    conv = NR.narrow(rows, kind, dt, scale, offset, fill)
    assert conv.dtype == dt and conv.shape == (n, c)
    if stride == 0:
        want[d_off:d_off + extent] = conv.view(np.uint8).reshape(-1)
    else:
        NR.to_planes(conv, want[d_off:d_off + extent].view(dt), stride)
    d_scale = d_offset = None
    if scale is not None:
        d_scale = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float64)).cuda()
        d_offset = torch.from_numpy(np.ascontiguousarray(offset, dtype=np.float64)).cuda()
    src_ptr, dst_ptr = d_src.data_ptr() + s_off, d_out.data_ptr() + d_off
    wide = N.narrow_device(src_ptr, kind, n, c, dst_ptr, dt, stride,
                           d_scale.data_ptr() if scale is not None else 0,
                           d_offset.data_ptr() if scale is not None else 0, fill,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    msg = f"narrow kind={kind} {dt} n={n} c={c} stride={stride} shift={shift} src+{src_off8} wide={wide} {what}"
    np.testing.assert_array_equal(d_out.cpu().numpy(), want, err_msg=msg)
    assert wide == NR.wide_ok(src_ptr, dst_ptr, esz, n, c, stride), "access width: " + msg
    return wide


def shape_cases():
    cases = []
    for i, n in enumerate(NS):
        for k, c in enumerate(CS):
            for s, stride in enumerate(STRIDES):
                cases.append((n, c, stride, (i + k + s) % len(CONVERSIONS), (k // 2 + i) % 2 == 1, (i // 2 + k) % 2 == 1))
    return cases


def test_the_rotation_covers_every_conversion_in_every_form():
    seen = {(conv, stride, scaled, shifted) for _, _, stride, conv, scaled, shifted in shape_cases()}
    assert len(seen) == len(CONVERSIONS) * len(STRIDES) * 2 * 2


@pytest.mark.parametrize("n, c, stride, conv, scaled, src_shifted", shape_cases())
def test_shapes_and_alignment(N, n, c, stride, conv, scaled, src_shifted):
    kind, dtype = CONVERSIONS[conv]
    rows = encoded(n, c, kind, dtype)
    scale = offset = None
    if scaled and kind == NR.VALUE:
        scale = np.array([(0.5, 2.0, 4.0)[j % 3] for j in range(c)])
        offset = np.array([float(j % 3) for j in range(c)])
        rows = rows / scale  # (exact: powers of two)
    st = 0 if stride == "packed" else n + stride
    ran = set()
    for shift in SHIFTS:
        off8 = 8 if (src_shifted and st == 0) else 0
        ran.add(run_narrow(N, rows, kind, dtype, st, shift, off8, scale, offset, fill=None if kind == NR.INDEX else 3))
    esz = np.dtype(dtype).itemsize
    # shift 0 is 16-byte aligned: wide wherever the source, the stride and the count allow it; shifts 1 .. 3 are element
    # bases that are no multiple of 4 elements (uint8: of 4 bytes), where only the element path is right
    can = (st == 0 and not src_shifted and n * c >= 4) or (st != 0 and st % 4 == 0 and n >= 4)
    assert ran == ({True, False} if can else {False}), (ran, can, esz)


def special_values(kind, dtype):
    if kind == NR.INDEX:
        return np.array([0, 2**31 - 1, -1, -2**31, 1, 12345], dtype=np.int64)
    dt = np.dtype(dtype)
    common = [np.inf, -np.inf, np.nan, -0.0, 0.0, 1e300, -1e300]
    if dt.kind == "f":
        fmax = float(np.finfo(np.float32).max)
        half_ulp = 2.0**(127 - 24)
        return np.array(common + [1e39, -1e39, fmax, -fmax, fmax + half_ulp, np.nextafter(fmax + half_ulp, 0.0),
                                  1e-40, -1e-40, 2.0**-149, 2.0**-150, np.nextafter(2.0**-150, 1.0), 2.0**-126,
                                  1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24, np.nextafter(1.0 + 2.0**-24, 2.0), 0.1, -1 / 3])
    lo, hi = float(np.iinfo(dt).min), float(np.iinfo(dt).max)
    ends = [e + d for e in (lo, hi) for d in (0.0, 1.0, -1.0, 0.5, -0.5, 0.49999, -0.49999)]
    halves = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 100.5, 101.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0),
              np.nextafter(1.5, 1.0), np.nextafter(2.5, 3.0)]
    return np.array(common + ends + halves)


@pytest.mark.parametrize("conv, with_fill", [(i, f) for i, (kind, _) in enumerate(CONVERSIONS) for f in (False, True)
                                             if not (f and kind == NR.INDEX)])  # (indices take no fill)
def test_special_values(N, conv, with_fill):
    kind, dtype = CONVERSIONS[conv]
    sp = special_values(kind, dtype)
    fill = None
    if with_fill:
        fill = -9999.0 if np.dtype(dtype) in (np.float32, np.int16, np.int32) else 7.0
    for n, c in ((300, 5), (257, 17)):
        rows = sp[(np.arange(n)[:, None] * 3 + np.arange(c)[None, :] * 5) % sp.size]
        for st in (0, n + 3, n + 1):  # (300 + 3 and 257 + 3 are odd / even mixes: 303 no, 260 yes -- both widths occur)
            for shift in (0, 1):
                run_narrow(N, rows, kind, dtype, st, shift, fill=fill, what=f"special fill={fill}")
        assert run_narrow(N, rows, kind, dtype, 0, 0, fill=fill) is True
        assert run_narrow(N, rows, kind, dtype, (n + 3) // 4 * 4, 0, fill=fill) is True


@pytest.mark.parametrize("dtype", [np.int32, np.int16, np.float32])
def test_two_roundings_on_the_device(N, dtype):
    v = np.array([[c[0] for c in NR.FMA_CASES]] * 9)  # (9, 4): one column per case, both widths below
    scale = np.array([c[1] for c in NR.FMA_CASES])
    offset = np.array([c[2] for c in NR.FMA_CASES])
    two = np.array([c[3] for c in NR.FMA_CASES])
    np.testing.assert_array_equal(NR.narrow_values(v, dtype, scale, offset)[0], NR.narrow_values(two, dtype))
    for st in (0, 12, 9):
        for shift in (0, 1):
            run_narrow(N, v, NR.VALUE, dtype, st, shift, scale=scale, offset=offset, what="fma cases")
