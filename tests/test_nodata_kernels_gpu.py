"""The four kernels of the nodata front end (sknnr_amd/csrc/mask.hip.h), each run alone through the debug entry points
``sknnr_debug_mask_compact`` and ``sknnr_debug_expand_rows`` and compared with the host restatement (tests/_nodata.py)
by ``assert_array_equal``: every valid flag, every block offset, every rank, the unit of the copy, every packed byte and
every expanded element, and the bytes around them that must be left alone.  No row is exempted.

tests/test_nodata_gpu.py sees these kernels only through the answers of a whole masked search on allocator-aligned
buffers; here the test chooses the addresses (views into larger device buffers), the element types and their range
ends, the row widths around the staging limits of the nodata values (256 lanes, 512 LDS entries), more than one block
per lane of the scan, and k / t / absent outputs of the expansion.

Measured on an MI355X: the 388 cases of this module take 6.3 s, of which 3.4 s are the first case's device set-up; the
slowest single case takes 0.12 s.

Scratch mutations of mask.hip.h (never committed; each keeps every access inside its buffer -- the packed buffer has one
spare row for that) and the cases of this module that fail under them, of 388:

=========================================================  ======  ====================================================
mutation                                                   failed  where
=========================================================  ======  ====================================================
compaction: the lane mask made inclusive                      291  210 compaction, 48 widths, 27 range ends, 6 scan
compaction: wave 0's count left out of ``base``               201  120 compaction, 48 widths, 27 range ends, 6 scan
mask: the NaN clause removed                                   16  14 widths (float32 / float64), 2 range ends (NaN)
mask: the comparison made in float32                            8  range ends: the five int32 cases, float32 0.1
                                                                   against the double 0.1, float64 0.1, beside 2^53
expansion: ``fill_index`` replaced by 0                        91  84 k / t / nq, 4 absent outputs, 3 without ``valid``
=========================================================  ======  ====================================================
"""

from __future__ import annotations

import numpy as np
import pytest

import _nodata as ND

pytestmark = pytest.mark.gpu

GUARD = 64  # untouched bytes asked for in front of and behind the packed rows (a multiple of 16: alignment is the offset's)
PATTERN = 0xA5
NQS = (1, 63, 64, 65, 256, 257, 1025)


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


def run_mask_compact(N, x, nodata, src_off=0, out_off=0, want_unit=None, what=""):
    """Mask, scan and compaction of ``x`` on the device, the rows placed ``src_off`` bytes and the packed rows ``out_off``
    bytes behind a 16-byte boundary; everything that comes back is compared with the restatement.  Returns ``valid``."""
    import torch

    x = np.ascontiguousarray(x)
    nq, d_in = x.shape
    row_bytes = d_in * x.dtype.itemsize
    assert src_off % x.dtype.itemsize == 0 and out_off % x.dtype.itemsize == 0
    raw = x.view(np.uint8).reshape(-1)
    src = torch.zeros(src_off + raw.size, dtype=torch.uint8, device="cuda")
    src[src_off:] = torch.from_numpy(raw).cuda()
    # (one spare row: a rank that is one too large must show as a wrong byte, not leave the buffer)
    out = torch.full((GUARD + out_off + (nq + 1) * row_bytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0, "the allocator's bases are 16-byte aligned"
    q_ptr, packed_ptr = src.data_ptr() + src_off, out.data_ptr() + GUARD + out_off
    got = N.debug_mask_compact(q_ptr, nq, d_in, N.dtype_code(x.dtype), nodata, packed_ptr,
                               stream=torch.cuda.current_stream().cuda_stream)
    want = ND.row_mask(x, nodata)
    np.testing.assert_array_equal(got["valid"], want, err_msg=f"valid {what}")
    assert got["n_valid"] == int(want.sum()), what
    counts = ND.block_counts(want)
    offsets, total = ND.exclusive_scan(counts)
    np.testing.assert_array_equal(got["blk_off"], offsets, err_msg=f"block offsets {what}")
    np.testing.assert_array_equal(np.diff(np.append(got["blk_off"], got["n_valid"])), counts, err_msg=f"block counts {what}")
    np.testing.assert_array_equal(got["rank"], ND.ranks(want), err_msg=f"ranks {what}")
    assert got["unit"] == ND.compact_unit(q_ptr, packed_ptr, row_bytes), what
    if want_unit is not None:
        assert got["unit"] == want_unit, what
    buf = out.cpu().numpy()
    n_packed = total * row_bytes
    lo = GUARD + out_off
    np.testing.assert_array_equal(buf[lo:lo + n_packed], ND.compact(x, want).view(np.uint8).reshape(-1),
                                  err_msg=f"packed bytes {what}")
    assert (buf[:lo] == PATTERN).all(), f"bytes in front of the packed rows were written {what}"
    assert (buf[lo + n_packed:] == PATTERN).all(), f"bytes behind the {total} packed rows were written {what}"
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the mask: element types at the ends of their range
# ---------------------------------------------------------------------------------------------------------------------
NAN = float("nan")
INF = float("inf")
F01 = np.float32(0.1)
# (name, dtype, rows, nodata, valid written out by hand)
RANGE_CASES = [
    ("uint8 0/255", np.uint8, [[0, 255], [255, 0], [1, 254], [0, 0], [255, 255]], [0, 255], [0, 1, 1, 0, 0]),
    ("uint8 255/0", np.uint8, [[0, 255], [255, 0], [1, 254], [0, 0], [255, 255]], [255, 0], [1, 0, 1, 0, 0]),
    ("uint8 out of range", np.uint8, [[0, 255], [255, 0], [1, 1]], [-1, 256], [1, 1, 1]),
    ("int16 low end", np.int16, [[-32768, 0], [32767, -32768], [32767, 32767], [-32767, 1]], [-32768, -32768], [0, 0, 1, 1]),
    ("int16 high end", np.int16, [[-32768, 0], [32767, -32768], [0, 32767], [32766, -1]], [32767, 32767], [1, 0, 0, 1]),
    ("int16 out of range", np.int16, [[-32768, 32767], [0, -1]], [32768, 65535], [1, 1]),
    ("uint16 65535", np.uint16, [[65535, 0], [0, 65535], [65534, 1], [32768, 32767]], [65535, 65535], [0, 0, 1, 1]),
    ("uint16 is not signed", np.uint16, [[65535, 0], [32768, 1], [32767, 2]], [-1, -1], [1, 1, 1]),
    ("uint16 32768", np.uint16, [[32768, 0], [0, 32768], [32767, 5]], [32768, -32768], [0, 1, 1]),
    ("int32 low end", np.int32, [[-2**31, 0], [2**31 - 1, -2**31], [-2**31 + 1, 5]], [-2**31, -2**31], [0, 0, 1]),
    ("int32 high end", np.int32, [[2**31 - 1, 0], [0, 2**31 - 1], [2**31 - 2, 5], [-2**31, -1]], [2**31 - 1, 2**31 - 1], [0, 0, 1, 1]),
    # float32 has 24 bits: 2^31 - 1 and 2^31 - 64 both round to 2^31, 16777217 to 16777216
    ("int32 beside 2^31", np.int32, [[2**31 - 1, 2**31 - 64], [-2**31, 0]], [2.0**31, 2.0**31], [1, 1]),
    ("int32 2^24 + 1 as data", np.int32, [[16777217, 1], [16777216, 2], [1, 16777217]], [16777216, 16777216], [1, 0, 1]),
    ("int32 2^24 + 1 as nodata", np.int32, [[16777216, 1], [16777217, 2], [1, 16777216], [16777218, 3]], [16777217, 16777217], [1, 0, 1, 1]),
    ("float32 0.1, nodata the double 0.1", np.float32, [[F01, 1], [2, F01]], [0.1, 0.1], [1, 1]),
    ("float32 0.1, nodata the widened float", np.float32, [[F01, 1], [2, F01], [3, 4]], [float(F01), float(F01)], [0, 0, 1]),
    ("float32 +0.0 masks -0.0", np.float32, [[-0.0, 1], [1, 0.0], [1, 1]], [0.0, 0.0], [0, 0, 1]),
    ("float32 -0.0 masks +0.0", np.float32, [[-0.0, 1], [1, 0.0], [1, 1]], [-0.0, -0.0], [0, 0, 1]),
    ("float32 +inf", np.float32, [[INF, 1], [-INF, 1], [NAN, 1], [3.4e38, INF], [1, 1]], [INF, INF], [0, 1, 1, 0, 1]),
    ("float32 NaN in column 0 only", np.float32, [[NAN, 1], [1, NAN], [NAN, NAN], [7, 1], [1, 7], [INF, 2]], [NAN, 7], [0, 1, 0, 1, 0, 1]),
    ("float32 range ends", np.float32, [[np.finfo(np.float32).max, 1], [np.finfo(np.float32).tiny, 1], [1e-45, 1], [0, 1]],
     [float(np.finfo(np.float32).max), 0.0], [0, 1, 1, 1]),
    ("float64 0.1", np.float64, [[0.1, 1], [float(F01), 1], [np.nextafter(0.1, 1), 0.1]], [0.1, 0.1], [0, 1, 0]),
    ("float64 +0.0 masks -0.0", np.float64, [[-0.0, 1], [1, 0.0], [1, 1]], [0.0, 0.0], [0, 0, 1]),
    ("float64 -0.0 masks +0.0", np.float64, [[-0.0, 1], [1, 0.0], [1, 1]], [-0.0, -0.0], [0, 0, 1]),
    ("float64 +inf", np.float64, [[INF, 1], [-INF, 1], [NAN, 1], [1.7e308, INF], [1, 1]], [INF, INF], [0, 1, 1, 0, 1]),
    ("float64 NaN in column 1 only", np.float64, [[NAN, 1], [1, NAN], [NAN, NAN], [7, 1], [1, 7], [2, -INF]], [7, NAN], [1, 0, 0, 0, 1, 1]),
    ("float64 beside 2^53", np.float64, [[2.0**53, 1], [2.0**53 + 2, 1], [2.0**53 - 1, 1]], [2.0**53, 0], [0, 1, 1]),
]


@pytest.mark.parametrize("case", RANGE_CASES, ids=[c[0] for c in RANGE_CASES])
def test_mask_at_the_ends_of_each_type(N, case):
    name, dtype, rows, nodata, by_hand = case
    if np.dtype(dtype).kind == "f":
        x = np.array(rows, dtype=np.float64).astype(dtype)
    else:
        x = np.array(rows, dtype=np.int64).astype(dtype)
        assert np.array_equal(x.astype(np.int64), np.array(rows, dtype=np.int64)), "the rows fit the type"
    nodata = np.array(nodata, dtype=np.float64)
    np.testing.assert_array_equal(ND.row_mask(x, nodata), by_hand, err_msg="the restatement against the table")
    valid = run_mask_compact(N, x, nodata, what=name)
    np.testing.assert_array_equal(valid, by_hand)
    # the same rows over three blocks (the last one partial), every row at several lanes
    reps = -(-700 // x.shape[0])
    tiled = np.tile(x, (reps, 1))[:700]
    np.testing.assert_array_equal(run_mask_compact(N, tiled, nodata, what=name + " tiled"), np.tile(by_hand, reps)[:700])


# ---------------------------------------------------------------------------------------------------------------------
# the mask: row widths around the staging of the nodata values, rows around the block size
# ---------------------------------------------------------------------------------------------------------------------
WIDE_DTYPES = (np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64)
_wide = {}


def wide_problem(dtype, d_in):
    """1000 rows without a single hit, and per-column nodata values that all differ from their neighbours'."""
    key = (np.dtype(dtype), d_in)
    if key not in _wide:
        rng = np.random.default_rng(d_in * 8 + np.dtype(dtype).itemsize)
        x = rng.integers(0, 100, size=(1000, d_in)).astype(dtype)  # data in [0, 100)
        nodata = (100 + (np.arange(d_in) * 7) % 150).astype(np.float64)  # nodata in [100, 250): fits uint8
        if np.dtype(dtype).kind == "f":
            nodata[2::5] = np.nan
        x.setflags(write=False)
        _wide[key] = (x, nodata)
    return _wide[key]


def put(x, r, c, nodata):
    """Make (r, c) a hit of column c's nodata value."""
    x[r, c] = nodata[c]  # (NaN stays NaN in a float array)


@pytest.mark.parametrize("dtype", WIDE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("d_in", [1, 255, 256, 257, 511, 512, 513, 700])
def test_mask_row_widths_and_block_edges(N, dtype, d_in):
    base, nodata = wide_problem(dtype, d_in)
    rng = np.random.default_rng(d_in)
    is_float = np.dtype(dtype).kind == "f"
    for nq in (1, 255, 256, 257, 1000):
        x = base[:nq].copy()
        hit = np.zeros(nq, dtype=bool)
        # decoys first: another column's nodata value (and NaN where NaN is not nodata) leaves a row valid
        if d_in > 1:
            for r in rng.integers(0, nq, size=min(nq, 40)):
                c = int(rng.integers(0, d_in))
                other = (c + 1) % d_in
                if not np.isnan(nodata[other]) and nodata[other] != nodata[c]:
                    x[r, c] = nodata[other]
                elif is_float and not np.isnan(nodata[c]):
                    x[r, c] = np.nan
        # the only hit of a row in the first column of each block's first row ...
        for r in range(0, nq, ND.BLOCK_ROWS):
            x[r] = base[r]
            put(x, r, 0, nodata)
            hit[r] = True
        # ... and in the last column of the last row (of a partial block unless nq is a multiple of 256)
        x[nq - 1] = base[nq - 1]
        put(x, nq - 1, d_in - 1, nodata)
        hit[nq - 1] = True
        # single hits at random places, one per row; beyond column 255 the nodata value comes from the second round of
        # the staging loop, beyond column 511 (d_in > 512) from global memory
        for r in rng.choice(nq, size=min(nq, 60), replace=False):
            if not hit[r]:
                x[r] = base[r]
                put(x, r, int(rng.integers(0, d_in)), nodata)
                hit[r] = True
        if d_in > 256 and nq > 20:
            for r, c in ((10, 256), (11, d_in - 1), (12, min(d_in - 1, 512)), (13, 255)):
                x[r] = base[r]
                put(x, r, c, nodata)
                hit[r] = True
        valid = run_mask_compact(N, x, nodata, what=f"d_in={d_in} nq={nq}")
        np.testing.assert_array_equal(valid, (~hit).astype(np.uint8), err_msg=f"the rows that were given a hit, nq={nq}")


# ---------------------------------------------------------------------------------------------------------------------
# the scan: one, two and four blocks per lane
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blob", "alternating"])
@pytest.mark.parametrize("nq", [262_144, 262_145, 786_509])
def test_scan_with_several_blocks_per_lane(N, nq, kind):
    masked = ND.blob_mask(nq, 0.3, seed=nq & 7, mean_len=500) if kind == "blob" else ND.make_mask("alternating", nq)
    x = (np.arange(nq) % 251).astype(np.uint8).reshape(-1, 1)
    x[masked] = 255
    assert ND.mask_blocks(nq) == {262_144: 1024, 262_145: 1025, 786_509: 3073}[nq]
    valid = run_mask_compact(N, x, np.array([255.0]), want_unit=1, what=f"{kind} nq={nq}")
    np.testing.assert_array_equal(valid, ~masked)


# ---------------------------------------------------------------------------------------------------------------------
# the compaction: every unit, by the row size and by the addresses
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = {np.dtype(np.uint8): 255, np.dtype(np.int16): -32768, np.dtype(np.uint16): 65535, np.dtype(np.int32): -2**31,
            np.dtype(np.float32): -9999.0, np.dtype(np.float64): -9999.0}
# (dtype, columns, source offset, output offset, unit written out by hand)
COMPACT_CASES = [
    # by the row size, on aligned bases
    (np.uint8, 1, 0, 0, 1), (np.uint8, 3, 0, 0, 1), (np.uint8, 7, 0, 0, 1),  # 1, 3, 7 bytes
    (np.int16, 7, 0, 0, 2), (np.uint16, 3, 0, 0, 2),                         # 14, 6
    (np.float32, 3, 0, 0, 4), (np.int32, 3, 0, 0, 4),                        # 12
    (np.float64, 3, 0, 0, 8), (np.float64, 7, 0, 0, 8),                      # 24, 56
    (np.float64, 2, 0, 0, 16), (np.float64, 6, 0, 0, 16), (np.float64, 256, 0, 0, 16),  # 16, 48, 2048
    # by a view into a larger buffer: the source alone, the output alone, both
    (np.float32, 4, 4, 0, 4), (np.float32, 4, 0, 4, 4), (np.float32, 4, 4, 4, 4),      # 16-byte rows, unit 4
    (np.float64, 2, 8, 0, 8), (np.float64, 2, 0, 8, 8), (np.float64, 6, 8, 8, 8),      # 16 / 48-byte rows, unit 8
    (np.int16, 8, 2, 0, 2), (np.int16, 8, 0, 6, 2), (np.uint16, 8, 10, 2, 2),          # 16-byte rows, unit 2
    (np.uint8, 4, 0, 1, 1), (np.uint8, 16, 1, 0, 1), (np.uint8, 8, 3, 1, 1),           # 4 / 16 / 8-byte rows, unit 1
    (np.uint8, 16, 2, 4, 2), (np.uint8, 16, 4, 8, 4), (np.uint8, 16, 8, 0, 8),         # 16-byte rows of bytes: 2, 4, 8
    (np.int32, 4, 4, 8, 4), (np.float32, 2, 0, 4, 4), (np.float64, 256, 8, 0, 8),      # 16 / 8 / 2048-byte rows
]


def compact_id(c):
    dtype, d, so, oo, unit = c
    return f"{np.dtype(dtype).name}x{d}+{so}+{oo}-unit{unit}"


def rows_with_mask(nq, d, dtype, masked, seed):
    """Rows of full-range values without the sentinel; the rows named by ``masked`` get it in one column."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = rng.standard_normal((nq, d)).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, size=(nq, d), endpoint=True).astype(dt)
        x[x == SENTINEL[dt]] = 1
    rows = np.flatnonzero(masked)
    x[rows, rng.integers(0, d, size=rows.size)] = SENTINEL[dt]
    return x


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("case", COMPACT_CASES, ids=compact_id)
def test_compaction_units(N, case, nq):
    dtype, d, src_off, out_off, unit = case
    nodata = np.full(d, float(SENTINEL[np.dtype(dtype)]))
    for kind in ND.MASK_KINDS:
        masked = ND.make_mask(kind, nq, seed=nq + d)
        x = rows_with_mask(nq, d, dtype, masked, seed=nq * 31 + d)
        valid = run_mask_compact(N, x, nodata, src_off, out_off, want_unit=unit, what=f"{kind} nq={nq}")
        np.testing.assert_array_equal(valid, ~masked)


# ---------------------------------------------------------------------------------------------------------------------
# the expansion
# ---------------------------------------------------------------------------------------------------------------------
FILL_PATTERN = 0x5A5A5A5A5A5A5A5A
TAIL = 8  # elements behind each output that must be left alone
SPECIAL_BITS = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000001234,
                         0xFFF4000000000001, 0x0000000000000001], dtype=np.uint64).view(np.int64)  # -0.0, +-inf, NaNs, denormal
SPECIAL_IDX = np.array([2**53 + 1, 2**62 + 3, -1, -2**63, 2**63 - 1, -(2**53) - 1, 0], dtype=np.int64)


def packed_results(n_valid, cols, seed, special):
    """int64 (n_valid, cols) of arbitrary bit patterns, the special ones spread through them."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-2**63, 2**63 - 1, size=(n_valid, cols), dtype=np.int64)
    flat = a.reshape(-1)
    if flat.size:
        where = rng.integers(0, flat.size, size=max(1, flat.size // 3))
        flat[where] = special[np.arange(where.size) % special.size]
    return a


def run_expand(N, valid, k, t, fill_index, absent=None, valid_null=False, seed=0):
    import torch

    nq = valid.size
    vb = valid.astype(bool)
    nv = int(vb.sum())
    rank = ND.ranks(valid).astype(np.int32)
    rank[~vb] = 0  # a masked row's rank must not be used
    packed = {"idx": packed_results(nv, k, seed, SPECIAL_IDX), "dist": packed_results(nv, k, seed + 1, SPECIAL_BITS),
              "pred": packed_results(nv, t, seed + 2, SPECIAL_BITS)}
    cols = {"idx": k, "dist": k, "pred": t}
    dev = {name: torch.from_numpy(np.ascontiguousarray(a)).cuda() for name, a in packed.items()}
    outs = {name: torch.full((nq * c + TAIL,), FILL_PATTERN, dtype=torch.int64, device="cuda")
            for name, c in cols.items() if name != absent}
    v_dev, r_dev = torch.from_numpy(valid.astype(np.uint8)).cuda(), torch.from_numpy(rank).cuda()

    def out_ptr(name):
        return outs[name].data_ptr() if name in outs else 0

    def packed_ptr(name):
        # (no valid row: the packed arrays are empty and never read, but a requested output needs a non-null one)
        return 0 if valid_null else (dev[name].data_ptr() if nv else v_dev.data_ptr())

    N.debug_expand_rows(nq, k, t, 0 if valid_null else v_dev.data_ptr(), 0 if valid_null else r_dev.data_ptr(),
                        packed_ptr("idx"), packed_ptr("dist"), packed_ptr("pred"), out_ptr("idx"), out_ptr("dist"),
                        out_ptr("pred"), fill_index, stream=torch.cuda.current_stream().cuda_stream)
    use = np.zeros(nq, dtype=bool) if valid_null else vb
    what = f"nq={nq} k={k} t={t} absent={absent} valid_null={valid_null}"
    for name, out in outs.items():
        c = cols[name]
        got = out.cpu().numpy()
        assert (got[nq * c:] == FILL_PATTERN).all(), f"{name}: elements behind the output were written, {what}"
        got = got[:nq * c].reshape(nq, c)
        want = ND.expand(use, packed[name] if use.any() else np.zeros((0, c), dtype=np.int64),
                         fill_index if name == "idx" else 0)
        np.testing.assert_array_equal(got[use], want[use], err_msg=f"{name}: valid rows, bit for bit, {what}")
        if name == "idx":
            np.testing.assert_array_equal(got, want, err_msg=f"idx {what}")
        else:
            assert np.isnan(got[~use].view(np.float64)).all(), f"{name}: a masked row is not NaN, {what}"


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("t", [1, 2, 7])
@pytest.mark.parametrize("k", [1, 3, 5, 31])
def test_expansion(N, k, t, nq):
    for i, kind in enumerate(ND.MASK_KINDS):
        valid = (~ND.make_mask(kind, nq, seed=nq + k)).astype(np.uint8)
        fill_index = (0, -1, -7)[(i + k + t) % 3]
        run_expand(N, valid, k, t, fill_index, seed=nq + i)
        run_expand(N, valid, k, t, fill_index, absent=("idx", "dist", "pred")[(i + nq) % 3], seed=nq + i)


@pytest.mark.parametrize("absent", ["idx", "dist", "pred"])
@pytest.mark.parametrize("fill_index", [0, -1, -7])
def test_expansion_each_output_absent_and_each_fill(N, absent, fill_index):
    for nq in (257, 1025):
        for kind in ("random30", "block_run", "all"):
            valid = (~ND.make_mask(kind, nq, seed=3)).astype(np.uint8)
            run_expand(N, valid, 3, 2, fill_index, absent=absent, seed=nq)


@pytest.mark.parametrize("nq", [1, 256, 1025])
def test_expansion_without_valid_fills_everything(N, nq):
    valid = (~ND.make_mask("random30", nq, seed=1)).astype(np.uint8)
    for fill_index in (0, -1, -7):
        run_expand(N, valid, 3, 2, fill_index, valid_null=True)
        run_expand(N, valid, 1, 1, fill_index, valid_null=True, absent="dist")


def test_expansion_refuses_a_missing_packed_array(N):
    import torch

    nq, k, t = 300, 3, 2
    valid = (~ND.make_mask("random30", nq, seed=2)).astype(np.uint8)
    nv = int(valid.sum())
    v = torch.from_numpy(valid).cuda()
    r = torch.from_numpy(ND.ranks(valid).astype(np.int32)).cuda()
    ci = torch.zeros((nv, k), dtype=torch.int64, device="cuda")
    cd = torch.zeros((nv, k), dtype=torch.float64, device="cuda")
    cp = torch.zeros((nv, t), dtype=torch.float64, device="cuda")
    oi = torch.full((nq, k), 77, dtype=torch.int64, device="cuda")
    od = torch.full((nq, k), 77.0, dtype=torch.float64, device="cuda")
    op = torch.full((nq, t), 77.0, dtype=torch.float64, device="cuda")
    full = [v.data_ptr(), r.data_ptr(), ci.data_ptr(), cd.data_ptr(), cp.data_ptr(), oi.data_ptr(), od.data_ptr(), op.data_ptr()]
    for missing in (1, 2, 3, 4):  # rank, c_idx, c_dist, c_pred
        args = list(full)
        args[missing] = 0
        with pytest.raises(N.HipBackendError) as err:
            N.debug_expand_rows(nq, k, t, *args, fill_index=-1)
        assert err.value.code == N.ERR_INVALID
        assert (oi == 77).all() and (od == 77.0).all() and (op == 77.0).all(), "a refused call wrote something"
    # ... but a packed array nobody asks for may be missing
    for missing, out in ((2, 5), (3, 6), (4, 7)):
        args = list(full)
        args[missing] = args[out] = 0
        N.debug_expand_rows(nq, k, t, *args, fill_index=-1)
    # no output at all: nothing to do
    N.debug_expand_rows(nq, k, t, *full[:5], 0, 0, 0, fill_index=-1)
