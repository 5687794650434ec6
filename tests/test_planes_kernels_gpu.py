"""The two kernels of the band-first layout (sknnr_amd/csrc/planes.hip.h), each run alone through the handle-free entry
points ``sknnr_planes_to_rows`` / ``sknnr_rows_to_planes`` on torch device buffers and compared with the host
restatement (tests/_planes.py) by ``assert_array_equal`` over the WHOLE output buffer: every output byte, the 64 guard
bytes in front of and behind it, the gaps between output planes and the slack behind the guard.

Inputs: every element's bytes encode its (pixel, column), so a misplaced element cannot equal the right one -- uint8
``(p * c + j) mod 251``, uint16 ``mod 65521``, uint32 ``p * c + j + 1``, uint64 ``(j + 1) << 32 | (p + 1)``.  Source and
output start one element behind the allocator's 16-byte boundary plus the guard, so no 16-, 8- or 4-byte alignment holds
beyond the element's own; strides are ``n``, ``n + 1`` and ``n + 13`` in turn.

Groups (the column chunk of a workgroup is 128 bytes of a row: 128 / 64 / 32 / 16 columns of 1 / 2 / 4 / 8 bytes):

* ``test_planes_to_rows_every_n``: each n of {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4099} -- the tail block's
  row bound at one lane, one wave, one block, several blocks -- with c = 1, 7 and one below, at and one above the element
  size's chunk (127 / 128 / 129, 63 / 64 / 65, 31 / 32 / 33, 15 / 16 / 17), for every element size.
* ``test_planes_to_rows_every_c``: each c of {1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128, 129, 300, 700} --
  several chunks with a narrow last one -- with n = 65 and 513, for every element size.
* ``test_rows_to_planes_every_n`` / ``_every_c``: the reverse kernel (8-byte elements) over the same n and c.
* ``test_special_values_pass_bit_for_bit``: the six query dtypes with their range ends; the float types with NaNs with
  payloads (quiet, signalling, negative), -0.0, infinities, the largest, the smallest normal and a subnormal value.
* ``test_more_than_2_31_elements``: 33 planes of 2^26 + 5 uint8 pixels, n * c = 2.2e9: offsets that do not fit 32 bits.
  At that size the expected rows are torch's strided view of the source on the device, not the numpy restatement.
  (The reverse kernel computes its offsets with the same expressions; its case would need two 17 GiB buffers.)

Measured on an MI355X: the 493 cases of this module take 7 s, of which 3.2 s are the first case's device set-up; no other
case takes more than 0.15 s.

Scratch mutations of planes.hip.h (never committed; every buffer of this module carries slack for 256 more rows, so
each keeps every access inside its buffer; the 2^31 case, whose buffers carry no such slack, was left out of these runs)
and the cases that fail under them, of 492:

=====================================================================  ======  ==========================================
mutation                                                               failed  where
=====================================================================  ======  ==========================================
the tail block's row bound replaced by the block size (rows = 256)        467  every group; only n = 256 passes
the column chunk's edge off by one (a full chunk is chunk - 1 wide)       213  every c at or above the element's chunk
the stride replaced by n                                                  287  every case with stride n + 1 or n + 13
                                                                               and more than one column
the LDS padding removed (pitch = columns)                                   0  --
=====================================================================  ======  ==========================================

Removing the padding fails nothing, as it must: it is performance only.  The host chooses no wider access for these kernels
(every global access is one element wide, correct at any element-aligned address), so "the wide-access choice forced
on a misaligned base" has nothing to mutate.
"""

from __future__ import annotations

import numpy as np
import pytest

import _planes as PL

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
NS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4099)
CS = (1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128, 129, 300, 700)
PADS = (0, 1, 13)
ESZ = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


def encoded(n, c, esz):
    """(c, n) planes of unsigned elements whose bytes name (pixel, column)."""
    p = np.arange(n, dtype=np.uint64)[None, :]
    j = np.arange(c, dtype=np.uint64)[:, None]
    if esz == 1:
        v = (p * c + j) % 251
    elif esz == 2:
        v = (p * c + j) % 65521
    elif esz == 4:
        v = p * c + j + 1
    else:
        v = ((j + 1) << np.uint64(32)) | (p + 1)
    return v.astype(PL.UINT[esz])


def slack_bytes(c, esz):
    return PL.BLOCK_ROWS * (c + 1) * esz  # (256 more rows and 256 more elements of a plane stay inside the buffer)


def to_device(host_bytes):
    import torch

    t = torch.from_numpy(host_bytes).cuda()
    assert t.data_ptr() % 16 == 0, "the allocator's bases are 16-byte aligned"
    return t


def run_planes_to_rows(N, planes, pad, what=""):
    """``planes``: (c, n) array of any 1-, 2-, 4- or 8-byte dtype.  Runs the kernel with stride n + pad and compares the
    whole output buffer with the restatement."""
    import torch

    c, n = planes.shape
    esz = planes.dtype.itemsize
    stride = n + pad
    src_el = np.full(c * stride, 0xEE, dtype=PL.UINT[esz])
    src_el.reshape(c, stride)[:, :n] = planes.view(PL.UINT[esz])
    off = GUARD + esz  # one element behind a 16-byte boundary
    src = np.full(off + src_el.nbytes + slack_bytes(c, esz), 0xEE, dtype=np.uint8)
    src[off:off + src_el.nbytes] = src_el.view(np.uint8)
    want = np.full(off + n * c * esz + GUARD + slack_bytes(c, esz), PATTERN, dtype=np.uint8)
    d_src, d_out = to_device(src), to_device(want.copy())
    want[off:off + n * c * esz] = PL.planes_to_rows(src_el, n, c, stride).view(np.uint8).reshape(-1)
    N.planes_to_rows_device(d_src.data_ptr() + off, n, c, esz, stride, d_out.data_ptr() + off,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), want, err_msg=f"planes_to_rows n={n} c={c} esz={esz} stride={stride} {what}")


def run_rows_to_planes(N, rows, pad, what=""):
    """``rows``: (n, c) array of an 8-byte dtype.  Runs the kernel with stride n + pad and compares the whole output
    buffer -- planes, the gaps between them, guards and slack -- with the restatement."""
    import torch

    n, c = rows.shape
    stride = n + pad
    off = GUARD + 8
    extent = ((c - 1) * stride + n) * 8
    src = np.full(off + rows.nbytes + slack_bytes(c, 8), 0xEE, dtype=np.uint8)
    src[off:off + rows.nbytes] = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
    want = np.full(off + extent + GUARD + slack_bytes(c, 8), PATTERN, dtype=np.uint8)
    d_src, d_out = to_device(src), to_device(want.copy())
    PL.rows_to_planes(np.ascontiguousarray(rows).view(np.uint64), want[off:off + extent].view(np.uint64), stride)
    N.rows_to_planes_device(d_src.data_ptr() + off, n, c, d_out.data_ptr() + off, stride,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), want, err_msg=f"rows_to_planes n={n} c={c} stride={stride} {what}")


def every_n_cases():
    return [(esz, n, c, PADS[(i + k) % 3]) for esz in ESZ for i, n in enumerate(NS)
            for k, c in enumerate((1, 7, PL.chunk_cols(esz) - 1, PL.chunk_cols(esz), PL.chunk_cols(esz) + 1))]


def every_c_cases():
    return [(esz, n, c, PADS[(i + k) % 3]) for esz in ESZ for i, c in enumerate(CS) for k, n in enumerate((65, 513))]


@pytest.mark.parametrize("esz, n, c, pad", every_n_cases())
def test_planes_to_rows_every_n(N, esz, n, c, pad):
    run_planes_to_rows(N, encoded(n, c, esz), pad)


@pytest.mark.parametrize("esz, n, c, pad", every_c_cases())
def test_planes_to_rows_every_c(N, esz, n, c, pad):
    run_planes_to_rows(N, encoded(n, c, esz), pad)


@pytest.mark.parametrize("n, c, pad", [(n, c, PADS[(i + k) % 3]) for i, n in enumerate(NS) for k, c in enumerate((1, 3, 15, 16, 17))])
def test_rows_to_planes_every_n(N, n, c, pad):
    run_rows_to_planes(N, np.ascontiguousarray(encoded(n, c, 8).T), pad)


@pytest.mark.parametrize("n, c, pad", [(n, c, PADS[(i + k) % 3]) for i, c in enumerate(CS) for k, n in enumerate((65, 513))])
def test_rows_to_planes_every_c(N, n, c, pad):
    run_rows_to_planes(N, np.ascontiguousarray(encoded(n, c, 8).T), pad)


def special_values(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1], dtype=dtype)
    if dtype.itemsize == 4:  # quiet with a payload, negative quiet, signalling, negative signalling with every payload bit
        pay = np.array([0x7FC1235A, 0xFFC00007, 0x7F800001, 0xFFBFFFFF], dtype=np.uint32).view(dtype)
    else:
        pay = np.array([0x7FF8123456789ABC, 0xFFF8000000000007, 0x7FF0000000000001, 0xFFF7FFFFFFFFFFFF],
                       dtype=np.uint64).view(dtype)
    assert np.isnan(pay).all()
    fi = np.finfo(dtype)
    rest = np.array([-0.0, 0.0, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal],
                    dtype=dtype)
    return np.concatenate([pay, rest])


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16, np.uint16, np.uint8, np.int32])
@pytest.mark.parametrize("n, c", [(300, 5), (257, PL.CHUNK_BYTES // 2 + 1)])
def test_special_values_pass_bit_for_bit(N, dtype, n, c):
    sp = special_values(dtype)
    planes = sp[(np.arange(n)[None, :] * 3 + np.arange(c)[:, None] * 5) % sp.size]
    run_planes_to_rows(N, np.ascontiguousarray(planes), 1, what=str(np.dtype(dtype)))
    if np.dtype(dtype).itemsize == 8:  # float64 distances and predictions travel back through the reverse kernel
        run_rows_to_planes(N, np.ascontiguousarray(planes.T), 13, what=str(np.dtype(dtype)))


def test_more_than_2_31_elements(N):
    import torch

    n, c = (1 << 26) + 5, 33
    stride = n + 1
    assert n * c > 2**31
    src = torch.randint(0, 256, (GUARD + 1 + c * stride,), dtype=torch.uint8, device="cuda")
    out = torch.full((GUARD + 1 + n * c + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    off = GUARD + 1
    N.planes_to_rows_device(src.data_ptr() + off, n, c, 1, stride, out.data_ptr() + off,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = src[off:].view(c, stride)[:, :n].T
    assert torch.equal(out[off:off + n * c].view(n, c), want)
    assert bool((out[:off] == PATTERN).all()) and bool((out[off + n * c:] == PATTERN).all())
