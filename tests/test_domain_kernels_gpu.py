"""The distance-domain kernel (sknnr_amd/csrc/domain.hip.h) through the C ABI (sknnr_domain_from_neighbors,
sknnr_debug_last_domain) on crafted tables and scores, against the numpy model of the contract (tests/_domain.py).
Everything is ``assert_array_equal``: a code is a count of comparisons and an integer division, every accumulator an
integer add, so the device's result is exact and two runs are the same bytes.

The shapes follow the kernel's geometry, read from the library (``_native.domain_geometry``: pixels per workgroup P,
skeleton entries S), never hard-coded: pixel counts around one workgroup's share, table lengths around the skeleton's
capacity.  The scores are made to sit where a search can go wrong: on table entries (at least half of them; the tables
hold long runs of duplicates), one float64 step to either side of an entry, midpoints, 0.0, -0.0, +inf, NaN and values
above the maximum.

Without the feature every test here fails: the entry points do not exist.

Measured on an MI355X: the 28 cases take 4.1 s, of which 3.2 s are the first case's device set-up; no other case takes more
than 0.05 s.
"""

from __future__ import annotations

import numpy as np
import pytest

import _domain as D

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


def geometry():
    from sknnr_amd import _native

    g = _native.domain_geometry(1)
    return g["pixels_per_workgroup"], g["skeleton"]


def make_table(m, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "runs":      # integer-valued, long runs of duplicates
        return np.sort(rng.integers(1, max(2, m // 7 + 2), size=m).astype(np.float64))
    if kind == "equal":     # every entry the same
        return np.full(m, 3.25)
    if kind == "zeros":     # leading zeros (co-located plots), then distinct values
        t = np.sort(rng.gamma(2.0, 1.0, size=m))
        t[: (m + 1) // 2] = 0.0
        t[0] = -0.0
        return t
    raise AssertionError(kind)


def make_scores(n, k, rank, table, seed):
    """(n, k) distances whose column rank - 1 holds the crafted scores; the other columns hold garbage the kernel must
    not read as scores (NaN and huge values)."""
    rng = np.random.default_rng(seed)
    dist = np.where(rng.random((n, k)) < 0.5, np.nan, 1e300)
    if n == 0:
        return dist
    entries = table[rng.integers(0, table.size, size=n)]
    s = entries.copy()                                        # at least half stay table entries
    kind = rng.integers(0, 12, size=n)
    s[kind == 6] = np.nextafter(entries[kind == 6], np.inf)
    s[kind == 7] = np.nextafter(entries[kind == 7], -np.inf)
    other = table[rng.integers(0, table.size, size=n)]
    s[kind == 8] = ((entries + other) / 2)[kind == 8]          # midpoints
    s[kind == 9] = rng.choice([0.0, -0.0, np.inf, np.nan], size=int((kind == 9).sum()))
    s[kind == 10] = table[-1] * rng.uniform(1.0, 3.0, size=int((kind == 10).sum())) + 1e-9
    s[kind == 11] = rng.uniform(0.0, table[-1] + 1.0, size=int((kind == 11).sum()))
    specials = [0.0, -0.0, np.inf, np.nan, table[-1], np.nextafter(table[-1], np.inf), table[0], np.nextafter(table[0], -np.inf)]
    s[: min(n, len(specials))] = specials[: min(n, len(specials))]
    dist[:, rank - 1] = s
    return dist


def domain_device(ix, dist, table, rank, threshold, acc=None, want_codes=True, misalign=False):
    """sknnr_domain_from_neighbors on device memory; fresh outputs start as garbage (77): accumulate = 0 must zero acc.
    ``misalign``: dist starts 8 bytes past a 16-byte boundary and the code plane 1 byte past a 4-byte one."""
    import torch

    n, k = dist.shape
    flat = torch.empty(dist.size + 1, dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0
    td = flat[1:1 + dist.size] if misalign else flat[:dist.size]
    td.copy_(torch.from_numpy(np.ascontiguousarray(dist).reshape(-1)))
    plane = torch.full((n + 1,), 77, dtype=torch.uint8, device="cuda")
    tc = plane[1:] if misalign else plane[:n]
    accumulate = acc is not None
    ta = torch.from_numpy(acc).cuda() if accumulate else torch.full((103,), 77, dtype=torch.int64, device="cuda")
    ix.domain_from_neighbors_device(td.data_ptr(), n, k, table, rank, threshold, tc.data_ptr() if want_codes else 0,
                                    ta.data_ptr(), accumulate, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if misalign and want_codes:
        assert int(plane[0]) == 77  # (the byte in front of the plane is not the kernel's)
    return (tc.cpu().numpy() if want_codes else None), ta.cpu().numpy()


def run(ix, mem, dist, table, rank, threshold=None, acc=None, want_codes=True):
    if mem == "host":
        return ix.domain_from_neighbors_host(dist, table, rank, threshold, acc=None if acc is None else acc.copy(),
                                             want_codes=want_codes)
    return domain_device(ix, dist, table, rank, threshold, acc, want_codes, misalign=mem != "device")


def check(ix, got, dist, table, rank, threshold=None, into=None):
    """``got`` against the model, and the record against the pixels."""
    codes, acc = got
    if codes is not None:
        np.testing.assert_array_equal(codes, D.codes(dist, table, rank))
    np.testing.assert_array_equal(acc, D.acc(dist, table, rank, threshold, into))
    rec = ix.debug_last_domain()
    n, k = dist.shape
    assert rec["ran"] == (1 if n else 0) and rec["pixels"] == n and rec["k"] == k, rec
    assert rec["rank"] == rank and rec["m"] == table.size and rec["blanked"] == 0, rec
    assert rec["nodata"] == int(np.isnan(dist[:, rank - 1]).sum()), rec
    return rec


def pixel_counts():
    p, _ = geometry()
    return [0, 1, 63, 64, 65, p - 1, p, p + 1, 3 * p + 7]


def table_lengths():
    _, s = geometry()
    return [1, 2, 3, s - 1, s, s + 1, 2 * s + 1, 40_000]


@pytest.mark.parametrize("kind", ["runs", "equal", "zeros"])
def test_every_table_length_at_every_pixel_count(kind):
    """All 9 x 8 shapes of one kind of table, host memory (the staged path), k = 5 at rank 5."""
    ix = index()
    for j, m in enumerate(table_lengths()):
        table = make_table(m, kind, seed=m)
        for i, n in enumerate(pixel_counts()):
            dist = make_scores(n, 5, 5, table, seed=100 * j + i)
            check(ix, run(ix, "host", dist, table, 5), dist, table, 5)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k, rank", [(1, 1), (5, 1), (5, 5), (17, 1), (17, 17)])
def test_ranks_memory_spaces_and_alignment(mem, k, rank):
    ix = index()
    p, s = geometry()
    for m, n in ((2 * s + 1, 3 * p + 7), (3, p + 1), (40_000, 65)):
        table = make_table(m, "runs", seed=k + m)
        dist = make_scores(n, k, rank, table, seed=rank + n)
        rec = check(ix, run(ix, mem, dist, table, rank), dist, table, rank)
        # the LDS form issues at most one global add per counter and workgroup; the plain form (-DSKNNR_DOMAIN_PLAIN) one
        # per pixel and one more per beyond pixel: no build issues more than the larger of the two
        assert 0 < rec["global_atomics"] <= max(103 * -(-n // p), 2 * n), rec


@pytest.mark.parametrize("mem", MEMS)
def test_threshold_on_an_entry_and_one_step_above(mem):
    """A pixel is beyond when s > theta: a score equal to the threshold is not."""
    ix = index()
    p, s = geometry()
    table = make_table(s + 1, "runs", seed=5)
    dist = make_scores(2 * p + 3, 5, 1, table, seed=6)
    entry = float(table[table.size // 2])
    dist[::7, 0] = entry
    dist[1::7, 0] = np.nextafter(entry, np.inf)
    counts = []
    for theta in (entry, float(np.nextafter(entry, np.inf)), 0.0, float(table[-1])):
        got = run(ix, mem, dist, table, 1, threshold=theta)
        check(ix, got, dist, table, 1, threshold=theta)
        counts.append(int(got[1][D.BEYOND]))
    assert counts[0] > counts[1] > 0  # (the pixels one step above the entry separate the two thresholds)
    assert counts[0] - counts[1] == int((dist[:, 0] == np.nextafter(entry, np.inf)).sum())
    got = run(ix, mem, dist, table, 1)  # no threshold: nothing is beyond
    assert got[1][D.BEYOND] == 0


@pytest.mark.parametrize("mem", MEMS)
def test_no_code_plane_tallies_the_same(mem):
    ix = index()
    p, s = geometry()
    table = make_table(2 * s + 1, "zeros", seed=9)
    dist = make_scores(p + 1, 5, 5, table, seed=10)
    codes, acc = run(ix, mem, dist, table, 5, threshold=1.0, want_codes=False)
    assert codes is None
    check(ix, (None, acc), dist, table, 5, threshold=1.0)


@pytest.mark.parametrize("mem", MEMS)
def test_accumulate_over_uneven_cuts_equals_one_shot_and_runs_repeat(mem):
    ix = index()
    p, s = geometry()
    table = make_table(40_000, "runs", seed=11)
    n = 3 * p + 7
    dist = make_scores(n, 5, 1, table, seed=12)
    theta = float(np.median(table))
    one = run(ix, mem, dist, table, 1, threshold=theta)  # accumulate = 0 over garbage-filled acc (device) / np.empty (host)
    check(ix, one, dist, table, 1, threshold=theta)
    again = run(ix, mem, dist, table, 1, threshold=theta)
    assert one[0].tobytes() == again[0].tobytes() and one[1].tobytes() == again[1].tobytes()
    acc = np.zeros(103, dtype=np.int64)
    parts = []
    for a, b in ((0, 1), (1, p + 64), (p + 64, n)):
        codes, acc = run(ix, mem, dist[a:b], table, 1, threshold=theta, acc=acc)
        parts.append(codes)
    np.testing.assert_array_equal(np.concatenate(parts), one[0])
    np.testing.assert_array_equal(acc, one[1])
    # accumulate = 1 adds to whatever the caller holds
    base = np.arange(103, dtype=np.int64) * 1_000_003
    _, acc = run(ix, mem, dist, table, 1, threshold=theta, acc=base)
    np.testing.assert_array_equal(acc, base + one[1])


def test_bad_arguments_are_refused_with_a_live_handle():
    from sknnr_amd import _native

    ix = index()
    dist = np.ones((4, 3))
    for table, rank, thr in (([2.0, 1.0], 1, None), ([1.0, np.nan], 1, None), ([1.0], 0, None), ([1.0], 4, None),
                             ([1.0], 1, -1.0), ([], 1, None)):
        with pytest.raises(_native.HipBackendError) as err:
            ix.domain_from_neighbors_host(dist, np.asarray(table, dtype=np.float64), rank, thr)
        assert err.value.code == _native.ERR_INVALID
