"""The id lookup inside the index conversion (sknnr_amd/csrc/narrow.hip.h, "indices, id table"), run alone through the
handle-free entry point ``sknnr_narrow_ids`` on torch device buffers and compared with the numpy restatement
(tests/_id_table.py) by ``assert_array_equal`` over the WHOLE destination buffer: every output byte, the 64 guard bytes
in front of and behind it, the gaps between output planes where the stride exceeds n, and the slack behind the guard.
The scheme is that of test_narrow_kernels_gpu.py.

Cases: n of {0, 1, 3, 4, 5, 255, 256, 257, 1000} x c of {1, 5, 16, 17} (16 is the plane kernel's column chunk) x
destination int64 / int32 x packed rows, planes n apart and planes n + 3 apart.  Every case runs at three placements --
source and destination on a 32-byte boundary (the wide path wherever the stride and the count allow it), the source one
element behind it (packed: 16-byte loads impossible), the destination one element behind it (4-element stores misaligned)
-- each with a fill and without one, and asserts that ``*out_wide`` is what ``narrow_wide_ok`` (``_narrow.wide_ok``, with
8 bytes per int64 element) predicts.

Inputs: a table of 1000 random int64 -- for int64 destinations over the whole int64 range, so negatives and values
beyond 2^31 occur; for int32 destinations over the int32 range, both ends included -- stored with 64 entries of slack
on either side; source entries uniform over the table, index 0 and the last index planted, about a fifth of them -1.
With a fill the restatement gives those ``fill``; without one a negative passes through, i.e. the restatement with
``fill=-1``.

``test_invalid_calls_leave_the_destination_alone``: every SKNNR_ERR_INVALID case on device pointers, after which the
destination buffer still holds its pattern.

Scratch mutations of ``narrow_one`` (never committed; the slack round the table keeps every access of each inside its
buffer) and the cases of ``test_lookup`` that fail under them, of 216:

=====================================================================  ======  ==========================================
mutation                                                               failed  where
=====================================================================  ======  ==========================================
``v <= 0`` for ``v < 0`` (index 0 takes the fill)                          186  every case but the 24 of n = 0 and 6 of n = 1,
                                                                               c = 1 (whose few entries hold no index 0)
``has_fill`` ignored (a negative always becomes ``fill_id``)                168  every case whose source holds a -1 (the runs
                                                                               without a fill); none at n = 0, and the small
                                                                               n * c without one
the lookup left out of the wide packed kernel's tail group                  26  packed cases with n * c >= 4 and no multiple
                                                                               of 4 (n of 1, 3, 5, 255, 257 x c of 1, 5, 17),
                                                                               both destination types
the table read before the sign is tested (``table[-1]`` loaded, then         0  nowhere: the value is discarded, so the data
discarded)                                                                     cannot see it; what the order buys is that no
                                                                               address in front of the table is ever read
=====================================================================  ======  ==========================================

Measured on an MI355X: the 218 cases of this module take 4.4 s, of which 3.5 s are the first case's device set-up.
"""

from __future__ import annotations

import numpy as np
import pytest

import _id_table as IT
import _narrow as NR

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
NS = (0, 1, 3, 4, 5, 255, 256, 257, 1000)
CS = (1, 5, 16, 17)
DTYPES = (np.int64, np.int32)
STRIDES = ("packed", 0, 3)  # packed rows, or planes n + pad apart
# (source, destination) elements behind a 32-byte boundary
PLACEMENTS = ((0, 0), (1, 0), (0, 1))
N_TABLE = 1000
TABLE_SLACK = 64
BLOCK_ROWS = 256
FILLS = {np.dtype(np.int64): -(2**40) - 7, np.dtype(np.int32): -2**31}


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def tables(N):
    """Per destination type: the host table and its device copy (with slack), computed once and never written."""
    import torch

    rng = np.random.default_rng(20261019)
    out = {}
    for dt in DTYPES:
        info = np.iinfo(dt)
        t = rng.integers(info.min, info.max, size=N_TABLE, dtype=np.int64, endpoint=True)
        t[:4] = (info.max, info.min, -1, 0)
        buf = np.full(N_TABLE + 2 * TABLE_SLACK, 0x5A5A5A5A, dtype=np.int64)
        buf[TABLE_SLACK:TABLE_SLACK + N_TABLE] = t
        dev = torch.from_numpy(buf).cuda()
        t.setflags(write=False)
        out[np.dtype(dt)] = (t, dev, dev.data_ptr() + TABLE_SLACK * 8)
    assert (out[np.dtype(np.int64)][0] > 2**31).any() and (out[np.dtype(np.int64)][0] < -2**31).any()
    return out


def source_rows(n, c):
    rng = np.random.default_rng(n * 131 + c)
    rows = rng.integers(0, N_TABLE, size=(n, c), dtype=np.int64)
    rows[rng.random((n, c)) < 0.2] = -1
    if n * c >= 3:
        rows.reshape(-1)[[0, -1]] = (0, N_TABLE - 1)
    return rows


def to_device(host_bytes):
    import torch

    t = torch.from_numpy(host_bytes).cuda()
    assert t.data_ptr() % 32 == 0, "the allocator's bases are 32-byte aligned"
    return t


def run_ids(N, tables, rows, dtype, stride, src_shift, dst_shift, fill):
    """``rows``: (n, c) int64 indices.  ``stride``: 0 for packed rows, else the elements between planes.  Compares the
    whole destination buffer with the restatement, then the access width with the restated choice; returns it."""
    import torch

    n, c = rows.shape
    dt = np.dtype(dtype)
    esz = dt.itemsize
    table, _, table_ptr = tables[dt]
    rows = np.ascontiguousarray(rows)
    slack = BLOCK_ROWS * (c + 1) * 8
    s_off = GUARD + 8 * src_shift
    src = np.full(s_off + rows.nbytes + slack, 0xEE, dtype=np.uint8)
    src[s_off:s_off + rows.nbytes] = rows.view(np.uint8).reshape(-1)
    d_off = GUARD + dst_shift * esz
    extent = (n * c if stride == 0 else ((c - 1) * stride + n if n else 0)) * esz
    want = np.full(d_off + extent + GUARD + slack, PATTERN, dtype=np.uint8)
    d_src, d_out = to_device(src), to_device(want.copy())
    conv = IT.lookup(rows, table, -1 if fill is None else fill, dt)
    assert conv.dtype == dt and conv.shape == (n, c)
    if stride == 0:
        want[d_off:d_off + extent] = conv.view(np.uint8).reshape(-1)
    elif n:
        NR.to_planes(conv, want[d_off:d_off + extent].view(dt), stride)
    src_ptr, dst_ptr = d_src.data_ptr() + s_off, d_out.data_ptr() + d_off
    wide = N.narrow_ids_device(src_ptr, n, c, table_ptr, N_TABLE, dst_ptr, dt, stride, fill_id=fill,
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    msg = f"ids {dt} n={n} c={c} stride={stride} src+{src_shift} dst+{dst_shift} fill={fill} wide={wide}"
    np.testing.assert_array_equal(d_out.cpu().numpy(), want, err_msg=msg)
    assert wide == (n > 0 and NR.wide_ok(src_ptr, dst_ptr, esz, n, c, stride)), "access width: " + msg
    return wide


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_lookup(N, tables, n, c, dtype, stride):
    rows = source_rows(n, c)
    assert n * c < 40 or ((rows < 0).mean() > 0.1 and (rows >= 0).mean() > 0.6)
    st = 0 if stride == "packed" else n + stride
    ran = {}
    for src_shift, dst_shift in PLACEMENTS:
        for fill in (FILLS[np.dtype(dtype)], None):
            ran[(src_shift, dst_shift, fill is None)] = run_ids(N, tables, rows, dtype, st, src_shift, dst_shift, fill)
    # the aligned placement is wide wherever the stride and the count allow it; a shifted destination never is; a
    # shifted source forbids it for packed rows only (the plane form reads its source element by element)
    can = (st == 0 and n * c >= 4) or (st != 0 and st % 4 == 0 and n >= 4)
    for (src_shift, dst_shift, _), wide in ran.items():
        assert wide == (can and dst_shift == 0 and (src_shift == 0 or st != 0)), (ran, can)


def test_both_widths_occur_for_both_types_and_forms():
    """The table of cases above does reach the wide and the element kernels of every instantiation."""
    for esz in (8, 4):
        for form in STRIDES:
            seen = set()
            for n in NS:
                st = 0 if form == "packed" else n + form
                for s, d in PLACEMENTS:
                    if n:
                        seen.add(NR.wide_ok(64 + 8 * s, 64 + esz * d, esz, n, 5, st))
            assert seen == {True, False}, (esz, form)


def test_invalid_calls_leave_the_destination_alone(N, tables):
    import ctypes

    import torch

    lib = N.load()
    table, _, table_ptr = tables[np.dtype(np.int64)]
    rows = source_rows(8, 4)
    d_src = to_device(rows.view(np.uint8).reshape(-1).copy())
    host = np.full(8 * 4 * 8 + 2 * GUARD, PATTERN, dtype=np.uint8)
    d_out = to_device(host.copy())
    wide = ctypes.c_int32(7)
    vp = ctypes.c_void_p

    def call(src=d_src.data_ptr(), n=8, c=4, tab=table_ptr, n_table=N_TABLE, dst=d_out.data_ptr() + GUARD, dtype=0, stride=0):
        return lib.sknnr_narrow_ids(vp(src or None), n, c, vp(tab or None), n_table, 1, -1, vp(dst or None), dtype, stride,
                                    0, None, ctypes.byref(wide))

    inv = N.ERR_INVALID
    assert call(tab=0) == inv and call(n_table=0) == inv and call(n_table=-1) == inv
    for dtype in (1, 2, 3, 4, 6, -1):
        assert call(dtype=dtype) == inv
    assert call(n=-1) == inv and call(c=0) == inv and call(c=65537) == inv and call(stride=7) == inv
    assert call(src=0) == inv and call(dst=0) == inv
    assert wide.value == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), host)
    assert call() == 0  # (the same arguments, unbroken, do write)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    np.testing.assert_array_equal(got[GUARD:-GUARD].view(np.int64).reshape(8, 4), IT.lookup(rows, table, -1))
    assert (got[:GUARD] == PATTERN).all() and (got[-GUARD:] == PATTERN).all()
