"""The zonal-statistics kernel (sknnr_amd/csrc/zonal.hip.h) through the C ABI (sknnr_zonal_from_values,
sknnr_debug_last_zonal) on crafted tiles, against the numpy model of the contract (tests/_zonal.py).  Everything is
``assert_array_equal``: every accumulator is an integer add, min or max over the stored values, so the device's result
is exact and two runs are the same bytes.

The shapes follow the kernel's geometry, read from the library (``_native.zonal_geometry``: pixels per workgroup, table
slots), never hard-coded: pixel counts around one workgroup's share, more distinct keys per workgroup than its table
holds, host memory, device memory and device memory 8 bytes past a 16-byte boundary.

Without the feature every test here fails: the entry points do not exist.

Measured on an MI355X: the 20 cases take 4.1 s, of which 3.3 s are the first case's device set-up; no other case takes
more than 0.1 s.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import _zonal as Z

pytestmark = pytest.mark.gpu

_INDEX = []
MEMS = ["host", "device", "device-misaligned"]


def index():
    """One handle for the module: it gives the record and the staging buffers only."""
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    if not _INDEX:
        _INDEX.append(_native.Index(np.random.default_rng(0).standard_normal((37, 2))))
    return _INDEX[0]


def teardown_module(module):
    for ix in _INDEX:
        ix.close()
    _INDEX.clear()


def per_zone(n_classes):
    return 0 if n_classes is None else int(np.sum(n_classes))


def zonal_device(ix, values, zones, dtype, scale, offset, n_zones, n_classes, acc=None, hist=None, misalign=False):
    """sknnr_zonal_from_values on device memory; fresh outputs start as garbage (77): accumulate = 0 must initialise them.
    ``misalign``: values and zones start 8 bytes past a 16-byte boundary."""
    import torch

    def on_device(a, dtype, skip):
        flat = torch.empty(a.size + skip, dtype=dtype, device="cuda")
        assert flat.data_ptr() % 16 == 0
        view = flat[skip:skip + a.size] if misalign else flat[:a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        return view

    n, c = values.shape
    accumulate = acc is not None
    tv = on_device(values, torch.float64, 1)
    tz = on_device(np.asarray(zones, dtype=np.int32), torch.int32, 2)
    ph = per_zone(n_classes)
    ta = torch.from_numpy(acc).cuda() if accumulate else torch.full((n_zones, c, 6), 77, dtype=torch.int64, device="cuda")
    th = None
    if ph:
        th = torch.from_numpy(hist).cuda() if accumulate else torch.full((n_zones * ph,), 77, dtype=torch.int64, device="cuda")
    ix.zonal_from_values_device(tv.data_ptr(), tz.data_ptr(), n, c, np.dtype(dtype), n_zones, ta.data_ptr(),
                                th.data_ptr() if ph else 0, scale=scale, offset=offset, n_classes=n_classes,
                                accumulate=accumulate, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ta.cpu().numpy(), th.cpu().numpy() if ph else None


def run(ix, mem, values, zones, dtype, scale, offset, n_zones, n_classes, acc=None, hist=None):
    if mem == "host":
        return ix.zonal_from_values_host(values, zones, dtype, n_zones, scale=scale, offset=offset, n_classes=n_classes,
                                         acc=acc, hist=hist)
    return zonal_device(ix, values, zones, dtype, scale, offset, n_zones, n_classes, acc, hist, misalign=mem != "device")


def check(ix, got, values, zones, dtype, scale, offset, n_zones, n_classes, acc=None, hist=None):
    """``got`` against the model, and the record against the entries."""
    want_a, want_h, n_nan, n_outside, n_other = Z.zonal(values, zones, dtype, scale, offset, n_zones, n_classes, acc, hist)
    np.testing.assert_array_equal(got[0], want_a)
    if want_h is None:
        assert got[1] is None
    else:
        np.testing.assert_array_equal(got[1], want_h)
    rec = ix.debug_last_zonal()
    n, c = values.shape
    assert rec["ran"] == (1 if n else 0) and rec["pixels"] == n and rec["c"] == c, rec
    assert (rec["nan"], rec["outside"], rec["other"]) == (n_nan, n_outside, n_other), rec
    assert rec["tallied"] == n * c - n_nan - n_outside * c, rec
    return rec


def random_tile(n, c, n_zones, seed, lo=-300.0, hi=300.0, run_length=400):
    """Zones in runs (a raster's coherence) with a few codes outside, values with NaN rows and single NaN entries."""
    rng = np.random.default_rng(seed)
    values = rng.uniform(lo, hi, size=(n, c))
    zones = np.repeat(rng.integers(-1, n_zones + 1, size=n // run_length + 1), run_length)[:n].astype(np.int32)
    values[rng.random(n) < 0.03] = np.nan
    values[rng.random((n, c)) < 0.02] = np.nan
    return values, zones


@pytest.mark.parametrize("mem", MEMS)
def test_hand_written_case(mem):
    """12 pixels x 2 planes x 3 zones, written out in tests/_zonal.py: rounding to even, the clamp, NaN entries and a
    nodata pixel, zone codes -1 and n_zones, class values -1 and 5 of 3 classes."""
    ix = index()
    args = (Z.HAND_VALUES, Z.HAND_ZONES, np.int16, Z.HAND_SCALE, Z.HAND_OFFSET, 3, Z.HAND_CLASSES)
    got = run(ix, mem, *args)
    np.testing.assert_array_equal(got[0], Z.HAND_ACC)
    np.testing.assert_array_equal(got[1].reshape(3, 3), Z.HAND_HIST)
    rec = check(ix, got, *args)
    assert (rec["nan"], rec["outside"], rec["other"]) == Z.HAND_COUNTERS


@pytest.mark.parametrize("c", [1, 3, 7])
def test_pixel_counts_around_a_workgroup(c):
    """n in {1, 63, 257, a workgroup's pixels - 1, + 0, + 1, 70,001}: one lane, less than a wave, more than a workgroup's
    threads, and the borders between workgroups, at widths that do and do not divide a workgroup's entries."""
    from sknnr_amd import _native

    ix = index()
    ppw = _native.zonal_geometry(c)["pixels_per_workgroup"]
    n_classes = None if c == 1 else np.array([0] * (c - 1) + [6], dtype=np.int32)
    scale, offset = np.linspace(0.5, 2.0, c), np.linspace(-3.0, 40.0, c)
    for i, n in enumerate((1, 63, 257, ppw - 1, ppw, ppw + 1, 70_001)):
        values, zones = random_tile(n, c, 11, 100 * c + i)
        if c > 1:
            values[:, c - 1] = np.where(np.isnan(values[:, c - 1]), np.nan, np.floor(np.abs(values[:, c - 1])) % 8 - 1)
            offset[c - 1], scale[c - 1] = 0.0, 1.0
        args = (values, zones, np.int16, scale, offset, 11, n_classes)
        mem = MEMS[i % 3]
        check(ix, run(ix, mem, *args), *args)


@pytest.mark.parametrize("dtype", Z.DTYPES)
@pytest.mark.parametrize("scaled", [False, True])
def test_every_type_at_and_beyond_its_clamp(dtype, scaled):
    """Values at, next to and far beyond the type's range, +-inf, halves that round to even, and for int32 magnitudes
    >= 2^30, so that the high limb of the sum of squares is in use."""
    ix = index()
    info = np.iinfo(dtype)
    edge = np.array([info.min, info.max], dtype=np.float64)
    special = np.concatenate([edge, edge - 1, edge + 1, edge - 0.5, edge + 0.5, edge * 3, [np.inf, -np.inf, 0.5, 1.5, 2.5, -0.5,
                              -1.5, np.nan, 0.0, -0.0], np.array([2.0**30, -2.0**30, 2.0**30 + 1, 1.7e9, -2.1e9, 2.0**31 - 1])])
    rng = np.random.default_rng(int(info.max) % 1000 + scaled)
    body = rng.uniform(float(info.min) * 1.2 - 10, float(info.max) * 1.2 + 10, size=20_000)
    col0 = np.concatenate([special, body])
    values = np.stack([col0, col0[::-1]], axis=1)
    zones = (np.arange(len(col0)) * 7 // len(col0)).astype(np.int32)
    scale, offset = (np.array([0.5, 2.0]), np.array([0.25, -7.0])) if scaled else (None, None)
    args = (values, zones, dtype, scale, offset, 7, None)
    got = run(ix, "device", *args)
    check(ix, got, *args)
    if dtype == np.int32:
        assert (got[0][..., Z.SQ_HI] > 0).all()
    else:
        assert not got[0][..., Z.SQ_HI].any()
    got_host = run(ix, "host", *args)
    assert got_host[0].tobytes() == got[0].tobytes()


def test_one_hot_zone():
    """70,001 pixels all in zone 4: c distinct keys.  The design's bound: a workgroup issues global atomics only at its
    flush -- at most six per slot in use (c slots) and one per class slot in use."""
    from sknnr_amd import _native

    ix = index()
    n, c = 70_001, 3
    geo = _native.zonal_geometry(c)
    ppw = geo["pixels_per_workgroup"]
    assert n % 64 and n % ppw
    rng = np.random.default_rng(8)
    values = rng.uniform(-100.0, 100.0, size=(n, c))
    values[:, 2] = rng.integers(0, 4, size=n)
    n_classes = np.array([0, 0, 4], dtype=np.int32)
    zones = np.full(n, 4, dtype=np.int32)
    args = (values, zones, np.int32, np.array([1e6, 10.0, 1.0]), np.zeros(3), 9, n_classes)
    got = run(ix, "device", *args)
    rec = check(ix, got, *args)
    assert (got[0][4, :, Z.COUNT] == n).all() and got[0][..., Z.COUNT].sum() == n * c
    if geo["slots"]:  # (the LDS-table form; the plain form has no table and five or six atomics per entry)
        workgroups = -(-n // ppw)
        assert 0 < rec["global_atomics"] <= workgroups * (6 * c + 4), rec
        assert rec["global_atomics"] * 100 < n * c


def test_table_overflow():
    """Every pixel of a workgroup in a zone of its own: more distinct keys than its table holds.  The entries that find
    no slot go to the global accumulators directly -- the record's atomics exceed what a flush of every slot can issue --
    and the result is still the model's."""
    from sknnr_amd import _native

    ix = index()
    c = 2
    geo = _native.zonal_geometry(c)
    ppw = geo["pixels_per_workgroup"]
    n = 3 * ppw + 17
    n_zones = 65_537
    assert n < n_zones
    zones = np.random.default_rng(5).permutation(n_zones)[:n].astype(np.int32)
    rng = np.random.default_rng(6)
    values = np.stack([rng.uniform(-3e4, 3e4, size=n), rng.integers(0, 3, size=n).astype(np.float64)], axis=1)
    n_classes = np.array([0, 3], dtype=np.int32)
    args = (values, zones, np.int16, None, None, n_zones, n_classes)
    got = run(ix, "device", *args)
    rec = check(ix, got, *args)
    # all keys distinct, int16 (no high limb): five atomics per entry and one per class value, whichever way they went
    assert rec["global_atomics"] == 5 * n * c + n, rec
    if geo["slots"]:
        assert ppw * c > geo["slots"], "the shape no longer overflows a workgroup's table"
        workgroups = -(-n // ppw)
        assert rec["global_atomics"] > workgroups * (6 * geo["slots"] + geo["hist_slots"]), rec


def test_accumulate_in_any_order_equals_one_call():
    """accumulate = 1 over three calls equals one call on the concatenation, in either order, on host and device memory;
    accumulate = 0 overwrites garbage; two identical runs give the same bytes."""
    ix = index()
    c, n_zones = 3, 13
    n_classes = np.array([0, 5, 0], dtype=np.int32)
    scale, offset = np.array([10.0, 1.0, 0.01]), np.array([0.0, 0.0, 100.0])
    parts = []
    for i, n in enumerate((5_001, 257, 12_345)):
        values, zones = random_tile(n, c, n_zones, 40 + i)
        values[:, 1] = np.where(np.isnan(values[:, 1]), np.nan, np.floor(np.abs(values[:, 1])) % 7 - 1)
        parts.append((values, zones))
    all_values, all_zones = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rest = (np.int16, scale, offset, n_zones, n_classes)
    whole = run(ix, "device", all_values, all_zones, *rest)  # (over garbage: zonal_device fills fresh outputs with 77)
    check(ix, whole, all_values, all_zones, *rest)
    again = run(ix, "device-misaligned", all_values, all_zones, *rest)
    assert whole[0].tobytes() == again[0].tobytes() and whole[1].tobytes() == again[1].tobytes()
    for mem, order in (("device", (0, 1, 2)), ("host", (2, 0, 1)), ("device-misaligned", (1, 2, 0))):
        acc, hist = Z.empty(n_zones, c, n_classes)
        for i in order:
            acc, hist = run(ix, mem, *parts[i], *rest, acc=acc, hist=hist)
        np.testing.assert_array_equal(acc, whole[0])
        np.testing.assert_array_equal(hist, whole[1])
    # accumulate = 0 on host arrays that hold garbage
    host = ix.zonal_from_values_host(all_values, all_zones, np.int16, n_zones, scale=scale, offset=offset, n_classes=n_classes)
    assert host[0].tobytes() == whole[0].tobytes() and host[1].tobytes() == whole[1].tobytes()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_no_pixels_initialises_the_outputs(mem):
    """n == 0 is allowed: accumulate = 0 still initialises the outputs, the sentinels included; accumulate = 1 leaves
    them; the record says that no kernel ran."""
    ix = index()
    none_v, none_z = np.zeros((0, 2)), np.zeros(0, dtype=np.int32)
    args = (none_v, none_z, np.uint8, None, None, 3, Z.HAND_CLASSES)
    acc, hist = run(ix, mem, *args)
    want_a, want_h = Z.empty(3, 2, Z.HAND_CLASSES)
    np.testing.assert_array_equal(acc, want_a)
    np.testing.assert_array_equal(hist, want_h)
    rec = ix.debug_last_zonal()
    assert rec["ran"] == 0 and rec["pixels"] == 0 and rec["tallied"] == 0, rec
    kept = run(ix, mem, *args, acc=Z.HAND_ACC.copy(), hist=Z.HAND_HIST.reshape(-1).copy())
    np.testing.assert_array_equal(kept[0], Z.HAND_ACC)
    np.testing.assert_array_equal(kept[1], Z.HAND_HIST.reshape(-1))


def test_refusals_by_arguments_alone():
    """n_zones * c >= 2^32 and n_zones * max(n_classes) >= 2^32 are SKNNR_ERR_UNSUPPORTED before anything is allocated or
    read; NULL pointers and a float type are SKNNR_ERR_INVALID before any launch."""
    from sknnr_amd import _native

    ix = index()
    lib = _native.load()
    word = (ctypes.c_int64 * 2)()
    p = ctypes.cast(word, ctypes.c_void_p)
    H = _native.MEM_HOST
    I16 = _native.DTYPE_CODES[np.dtype(np.int16)]
    call = lib.sknnr_zonal_from_values
    assert call(ix.handle, p, p, 0, 2, I16, None, None, 2**31, None, p, None, 0, H, None) == _native.ERR_UNSUPPORTED
    assert b"32-bit keys" in lib.sknnr_last_error()
    cls = (ctypes.c_int32 * 2)(0, 4)
    assert call(ix.handle, p, p, 0, 2, I16, None, None, 2**30, cls, p, p, 0, H, None) == _native.ERR_UNSUPPORTED
    assert b"n_classes[1]" in lib.sknnr_last_error()
    ok_cls = (ctypes.c_int32 * 2)(0, 3)
    for args in ((ix.handle, None, p, 1, 2, I16, None, None, 3, None, p, None, 0, H, None),    # values NULL
                 (ix.handle, p, None, 1, 2, I16, None, None, 3, None, p, None, 0, H, None),    # zones NULL
                 (ix.handle, p, p, 1, 2, I16, None, None, 3, None, None, None, 0, H, None),    # acc NULL
                 (ix.handle, p, p, 1, 2, I16, None, None, 3, ok_cls, p, None, 0, H, None),     # hist NULL with classes
                 (ix.handle, p, p, 1, 2, I16, p, None, 3, None, p, None, 0, H, None),          # scale without offset
                 (ix.handle, p, p, 1, 2, 1, None, None, 3, None, p, None, 0, H, None),         # float32
                 (ix.handle, p, p, 1, 2, 0, None, None, 3, None, p, None, 0, H, None),         # float64
                 (ix.handle, p, p, -1, 2, I16, None, None, 3, None, p, None, 0, H, None),      # n < 0
                 (ix.handle, p, p, 1, 0, I16, None, None, 3, None, p, None, 0, H, None),       # c < 1
                 (ix.handle, p, p, 1, 2, I16, None, None, 0, None, p, None, 0, H, None),       # n_zones < 1
                 (ix.handle, p, p, 1, 2, I16, None, None, 3, None, p, None, 0, 7, None)):      # memspace
        assert call(*args) == _native.ERR_INVALID, args
    assert word[0] == 0 and word[1] == 0  # (nothing was written)
