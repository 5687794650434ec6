"""The neighbour-usage kernel (sknnr_amd/csrc/tally.hip.h) through the C ABI (sknnr_tally_from_neighbors,
sknnr_debug_last_tally) on crafted arrays, against the numpy model of the contract (tests/_usage.py).  Everything is
``assert_array_equal``: counts are integer adds and the maximum is an integer max on bit patterns, so the device's
result is exact and two runs are the same bytes.

The shapes follow the kernel's geometry, read from ``_native`` (rows per workgroup) and from the debug record (table
slots), never hard-coded: a row count that is no multiple of 64 nor of a workgroup's rows, more distinct keys per
workgroup than its table holds, odd first and last entries of a workgroup's range (k = 17), 16-byte aligned and
misaligned arrays, host and device memory.

Without the feature every test here fails: the entry points do not exist.

Measured on an MI355X: the 15 cases take 3.6 s, of which 3.2 s are the first case's device set-up; no other case takes
more than 0.1 s.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import _usage as U

pytestmark = pytest.mark.gpu

_INDEX = {}


def index(n_ref):
    """One handle per reference-row count, made once per module (the rows themselves do not matter to a tally)."""
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    if n_ref not in _INDEX:
        rng = np.random.default_rng(n_ref)
        _INDEX[n_ref] = _native.Index(rng.standard_normal((n_ref, 2)))
    return _INDEX[n_ref]


def teardown_module(module):
    for ix in _INDEX.values():
        ix.close()
    _INDEX.clear()


def tally_device(ix, idx, dist, counts=None, max_dist=None, misalign=False):
    """sknnr_tally_from_neighbors on device memory; fresh outputs start as garbage (77 / -3.0): accumulate = 0 must zero
    them.  ``misalign``: idx and dist start 8 bytes past a 16-byte boundary (the one-entry-per-load path)."""
    import torch

    def on_device(a, dtype):
        flat = torch.empty(a.size + 2, dtype=dtype, device="cuda")
        assert flat.data_ptr() % 16 == 0
        view = flat[1:1 + a.size] if misalign else flat[:a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        return view

    n, k = idx.shape
    accumulate = counts is not None
    ti = on_device(idx, torch.int64)
    td = on_device(dist, torch.float64) if dist is not None else None
    tc = torch.from_numpy(counts).cuda() if accumulate else torch.full((ix.n_ref, k), 77, dtype=torch.int64, device="cuda")
    tm = None
    if dist is not None:
        tm = torch.from_numpy(max_dist).cuda() if accumulate else torch.full((ix.n_ref,), -3.0, dtype=torch.float64, device="cuda")
    ix.tally_from_neighbors_device(0 if td is None else td.data_ptr(), ti.data_ptr(), n, k, tc.data_ptr(),
                                   0 if tm is None else tm.data_ptr(), accumulate, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tc.cpu().numpy(), None if tm is None else tm.cpu().numpy()


def check(ix, idx, dist, got, counts=None, max_dist=None):
    """``got`` against the model, and the record against the entries."""
    want_c, want_m, skipped = U.tally(idx, dist, ix.n_ref, counts, max_dist)
    np.testing.assert_array_equal(got[0], want_c)
    if dist is None:
        assert got[1] is None
    else:
        np.testing.assert_array_equal(got[1], want_m)
        assert not np.signbit(got[1]).any()
    rec = ix.debug_last_tally()
    assert rec["ran"] == 1 and rec["rows"] == idx.shape[0] and rec["k"] == idx.shape[1], rec
    assert rec["skipped"] == skipped and rec["tallied"] == idx.size - skipped, rec
    return rec


@pytest.mark.parametrize("with_dist", [True, False])
@pytest.mark.parametrize("mem", ["host", "device", "device-misaligned"])
def test_hand_written_case(mem, with_dist):
    """n_ref = 7, k = 3, 10 rows: a fill row, entries == n_ref, far outside and negative, a repeated index, distances
    0.0, -0.0 and NaN; the expected arrays are written out in tests/_usage.py."""
    ix = index(U.HAND_N_REF)
    dist = U.HAND_DIST if with_dist else None
    if mem == "host":
        got = ix.tally_from_neighbors_host(dist, U.HAND_IDX)
    else:
        got = tally_device(ix, U.HAND_IDX, dist, misalign=mem != "device")
    np.testing.assert_array_equal(got[0], U.HAND_COUNTS)
    if with_dist:
        np.testing.assert_array_equal(got[1], U.HAND_MAX)
    rec = check(ix, U.HAND_IDX, dist, got)
    assert rec["skipped"] == U.HAND_SKIPPED


@pytest.mark.parametrize("k", [1, 5])
def test_one_hot_bin(k):
    """70,001 rows all naming reference row 4 at every rank: k distinct keys.  The design's bound: a workgroup issues
    global atomics only at its flush, one add and at most one max per slot in use -- k slots here."""
    from sknnr_amd import _native

    ix = index(U.HAND_N_REF)
    n = 70_001
    per_wg = _native.tally_rows_per_workgroup(k)
    assert n % 64 and n % per_wg
    idx = np.full((n, k), 4, dtype=np.int64)
    dist = np.full((n, k), 0.75)
    dist[n // 2, k - 1] = 3.5
    got = tally_device(ix, idx, dist)
    assert (got[0][4] == n).all() and got[0].sum() == n * k and got[1][4] == 3.5
    rec = check(ix, idx, dist, got)
    if rec["slots"]:  # (the LDS-table form; the plain form has no table and one or two atomics per entry)
        workgroups = -(-n // per_wg)
        assert rec["overflowed"] == 0 and 0 < rec["global_atomics"] <= 2 * k * workgroups, rec
        assert rec["global_atomics"] * 100 < n * k


def test_table_overflow():
    """Every workgroup sees more distinct keys than its table holds: the entries that find no slot go to the global
    accumulators directly, and the result is still the model's."""
    from sknnr_amd import _native

    n_ref, k = 65_537, 5
    ix = index(n_ref)
    per_wg = _native.tally_rows_per_workgroup(k)
    n = 3 * per_wg + 17
    perm = np.random.default_rng(5).permutation(n_ref).astype(np.int64)
    idx = perm[np.arange(n * k) % n_ref].reshape(n, k)  # (n * k < n_ref: every key of the call is distinct)
    assert n * k < n_ref
    dist = np.random.default_rng(6).random((n, k)) + 0.5
    got = tally_device(ix, idx, dist)
    rec = check(ix, idx, dist, got)
    if rec["slots"]:
        assert per_wg * k > rec["slots"], "the shape no longer overflows a workgroup's table"
        # at least what cannot fit, in each of the three full workgroups
        assert rec["overflowed"] >= 3 * (per_wg * k - rec["slots"]) > 0, rec
        assert rec["global_atomics"] == 2 * n * k, rec  # (all keys distinct, all distances > 0: an add and a max each)


def mixed_rows(n, n_ref, k, seed):
    """Runs of equal rows of random length 1 .. 5,000: coherent stretches and their borders."""
    rng = np.random.default_rng(seed)
    lengths = []
    while sum(lengths) < n:
        lengths.append(int(rng.integers(1, 5_001)))
    proto_i = rng.integers(0, n_ref, size=(len(lengths), k))
    proto_d = rng.random((len(lengths), k)) * 100.0
    rep = np.repeat(np.arange(len(lengths)), lengths)[:n]
    return proto_i[rep].astype(np.int64), proto_d[rep]


@pytest.fixture(scope="module")
def mixed():
    n_ref, k = 50_000, 5
    idx, dist = mixed_rows(200_000, n_ref, k, 21)
    return n_ref, idx, dist, U.tally(idx, dist, n_ref)


def test_mixed_law_twice_and_accumulated(mixed):
    n_ref, idx, dist, want = mixed
    ix = index(n_ref)
    first = tally_device(ix, idx, dist)
    check(ix, idx, dist, first)
    second = tally_device(ix, idx, dist, misalign=True)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    # accumulate = 1 on the first result: exactly double the counts, the same maxima; a stored NaN / negative reads as +0.0
    stored = first[1].copy()
    unused = np.flatnonzero(first[0].sum(1) == 0)
    assert unused.size > 1
    stored[unused[0]], stored[unused[1]] = np.nan, -2.0
    doubled = tally_device(ix, idx, dist, counts=first[0].copy(), max_dist=stored)
    np.testing.assert_array_equal(doubled[0], 2 * want[0])
    np.testing.assert_array_equal(doubled[1], want[1])
    host = ix.tally_from_neighbors_host(dist, idx, counts=first[0].copy(), max_dist=stored.copy())
    np.testing.assert_array_equal(host[0], 2 * want[0])
    np.testing.assert_array_equal(host[1], want[1])


@pytest.mark.parametrize("k, n", [(1, 20_011), (17, None), (192, 301)])
def test_width_extremes(k, n):
    """k = 1, k = 192 at n_ref = 300, and k = 17, where a workgroup's rows hold an odd number of entries: its range begins
    and ends on odd entries, which the 16-byte loads leave to single loads."""
    from sknnr_amd import _native

    ix = index(300)
    per_wg = _native.tally_rows_per_workgroup(k)
    if n is None:
        assert (per_wg * k) % 2 == 1
        n = 3 * per_wg + 5
    rng = np.random.default_rng(k)
    idx = rng.integers(-2, 302, size=(n, k)).astype(np.int64)  # (a few entries outside [0, 300))
    dist = rng.random((n, k))
    for misalign in (False, True):
        check(ix, idx, dist, tally_device(ix, idx, dist, misalign=misalign))
    check(ix, idx, None, tally_device(ix, idx, None))
    check(ix, idx, dist, ix.tally_from_neighbors_host(dist, idx))


def test_refusals_by_arguments_alone():
    """n_ref * k >= 2^32 is SKNNR_ERR_UNSUPPORTED before anything is allocated or read; dist and max_dist come together."""
    from sknnr_amd import _native

    ix = index(300)
    lib = _native.load()
    k_big = -(-2**32 // 300)
    assert 300 * k_big >= 2**32 > 300 * (k_big - 1)
    word = (ctypes.c_int64 * 1)()
    p = ctypes.cast(word, ctypes.c_void_p)
    rc = lib.sknnr_tally_from_neighbors(ix.handle, None, p, 0, k_big, p, None, 0, _native.MEM_HOST, None)
    assert rc == _native.ERR_UNSUPPORTED and b"32-bit keys" in lib.sknnr_last_error()
    assert lib.sknnr_tally_from_neighbors(ix.handle, p, p, 1, 1, p, None, 0, _native.MEM_HOST, None) == _native.ERR_INVALID
    assert b"come together" in lib.sknnr_last_error()
    assert lib.sknnr_tally_from_neighbors(ix.handle, None, p, 1, 0, p, None, 0, _native.MEM_HOST, None) == _native.ERR_INVALID
    assert lib.sknnr_tally_from_neighbors(ix.handle, None, p, 1, 1, None, None, 0, _native.MEM_HOST, None) == _native.ERR_INVALID
    assert lib.sknnr_tally_from_neighbors(None, None, p, 1, 1, p, None, 0, _native.MEM_HOST, None) == _native.ERR_INVALID
    assert lib.sknnr_stream_set_tally(None) == _native.ERR_INVALID
    assert lib.sknnr_stream_get_tally(None, p, None) == _native.ERR_INVALID


def test_no_rows_zeroes_the_outputs():
    """nq = 0 is allowed: accumulate = 0 still zeroes the outputs, accumulate = 1 leaves them (through the > 0 rule), and
    the record says that no kernel ran."""
    ix = index(U.HAND_N_REF)
    none_i, none_d = np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3))
    counts, mx = ix.tally_from_neighbors_host(none_d, none_i)
    assert not counts.any() and not mx.any() and counts.shape == (7, 3)
    rec = ix.debug_last_tally()
    assert rec["ran"] == 0 and rec["rows"] == 0 and rec["tallied"] == 0, rec
    kept = ix.tally_from_neighbors_host(none_d, none_i, counts=U.HAND_COUNTS.copy(), max_dist=np.array([1.5, -1, np.nan, 0, 2, 0, 0]))
    np.testing.assert_array_equal(kept[0], U.HAND_COUNTS)
    np.testing.assert_array_equal(kept[1], [1.5, 0, 0, 0, 2, 0, 0])
