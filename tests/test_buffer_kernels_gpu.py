"""The buffer instantiations of group_scan_kernel (groups.hip.h) and buffer_count_kernel (buffer.hip.h) through
``_native.Index``: every comparison is ``assert_array_equal`` against the contract's numpy model (tests/_buffer.py).

Shapes, the smallest at which the kernels can go wrong: 37 reference rows (less than one step of 512 columns), 700 (a
partial second step in which a thread's second column runs off the end), 1100 (a third step); d = 3 (below the 8-wide
unroll) and 13 (unroll plus tail); one column-chunked case (40 rows of 1,030 columns); k = 1 and 5; positions of 1, 2 and
3 columns; the buffer alone and together with groups of 1 to 7 rows.  8,200 rows of 3 columns are 1,025 passes on 1,024
workgroups.  One value matrix per (n, d, formula) is computed once and shared; nothing writes to it."""

from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import pytest

import _buffer
import _groups
from sknnr_amd import synth

pytestmark = pytest.mark.gpu

FORMULAS = {"expanded": 0, "direct": 1, "hamming": 2}
KS = (1, 5)
PLUS = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]
DIAG = [(1, 1), (1, -1), (-1, 1), (-1, -1)]


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


@lru_cache(maxsize=None)
def fit_rows(n, d):
    x = synth.make_features(n, d, seed=3)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def values(n, d, formula):
    full = _groups.value_rows(fit_rows(n, d), np.arange(n), formula)
    full.setflags(write=False)
    return full


@lru_cache(maxsize=None)
def hamming_problem(n, trees):
    ids, _ = synth.make_forest_ids(n, 1, trees)
    w = np.random.default_rng(11).uniform(0.05, 1.05, trees)
    full = _groups.value_rows(ids, np.arange(n), "hamming", w)
    for a in (ids, w, full):
        a.setflags(write=False)
    return ids, w, full


def codes_of(n):
    return _groups.random_sizes(n, 1, 7, seed=n)


@pytest.fixture(scope="module")
def indexes(N):
    """One handle per reference set, shared by the module's tests and closed behind them."""
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    yield get
    for ix in cache.values():
        ix.close()


def call(ix, k, formula, det=True, **kw):
    return ix.kneighbors_grouped(k, deterministic=det, decimals=10, formula=FORMULAS[formula], **kw)


def check_against_model(ix, full, coords, radius, codes, formula, ks=KS, hamming=False):
    """Masks on the handle, then the counts and the scan at every k, with and without the reorder."""
    n = full.shape[0]
    rows = np.arange(n)
    ix.set_groups(codes)
    ix.set_buffer(coords, radius)
    mask = _buffer.excluded_mask(coords, radius, rows, codes)
    np.testing.assert_array_equal(ix.buffer_counts(), mask.sum(axis=1))
    val, idx = _buffer.ranked_candidates(full, mask, max(ks))
    for k in ks:
        for det in (True, False):
            want_d, want_i = _groups.finish(val[:, :k], idx[:, :k], rows, hamming=hamming, deterministic=det)
            dist, got = call(ix, k, formula, det)
            np.testing.assert_array_equal(got, want_i, err_msg=f"k={k} det={det}")
            np.testing.assert_array_equal(dist, want_d, err_msg=f"k={k} det={det}")
            assert not np.take_along_axis(mask, got, axis=1).any()
    assert ix.debug_last_buffer()["mask"] == (2 if codes is None else 3)
    only_idx = call(ix, ks[-1], formula, False, return_distance=False)
    assert only_idx[0] is None
    np.testing.assert_array_equal(only_idx[1], got)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("formula", ["expanded", "direct"])
@pytest.mark.parametrize("d", [3, 13])
@pytest.mark.parametrize("n", [37, 700, 1100])
def test_euclidean_matches_the_model(N, indexes, n, d, formula, c):
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    coords, radius = _buffer.uniform_square(n, c, seed=n + c), _buffer.radius_for(n, c)
    for codes in (None, codes_of(n)):
        check_against_model(ix, values(n, d, formula), coords, radius, codes, formula)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("n,trees", [(37, 3), (700, 13), (1100, 13)])
def test_hamming_matches_the_model(N, indexes, n, trees, c):
    ids, w, full = hamming_problem(n, trees)

    def make():
        ix = N.Index(ids)
        ix.set_hamming_weights(w)
        return ix

    coords, radius = _buffer.uniform_square(n, c, seed=n + c), _buffer.radius_for(n, c)
    for codes in (None, codes_of(n)):
        check_against_model(indexes(("hamming", n, trees), make), full, coords, radius, codes, "hamming", hamming=True)


@pytest.mark.parametrize("formula", ["expanded", "direct", "hamming"])
def test_wide_rows_in_column_chunks(N, formula):
    """d = 1030: the second column chunk is six columns wide (tail loop only)."""
    n, d = 40, 1030
    if formula == "hamming":
        fit, _ = synth.make_forest_ids(n, 1, d, seed=4)
        w = np.random.default_rng(12).uniform(0.05, 1.05, d)
    else:
        fit, w = synth.make_features(n, d, seed=3), None
    full = _groups.value_rows(fit, np.arange(n), formula, w)
    coords, radius = _buffer.uniform_square(n, 2, seed=n), _buffer.radius_for(n, 2)
    ix = N.Index(fit)
    try:
        if w is not None:
            ix.set_hamming_weights(w)
        for codes in (None, codes_of(n)):
            check_against_model(ix, full, coords, radius, codes, formula, hamming=w is not None)
    finally:
        ix.close()


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_the_boundary_is_closed(N, indexes, formula):
    """Positions on the integer lattice, 25 to a line: squared distances are small integers, exact in float64.
    radius 1: the four neighbours at distance exactly 1 are excluded (<=).  radius sqrt(2), whose square rounds to just
    above 2: the diagonals go too.  One ulp below, whose square is just below 2: the diagonals stay."""
    n, d, width = 700, 13, 25
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    coords = _buffer.lattice(n, width)
    below = math.nextafter(math.sqrt(2.0), 0.0)
    assert math.sqrt(2.0) * math.sqrt(2.0) > 2.0 > below * below
    for radius, offsets in ((1.0, PLUS), (math.sqrt(2.0), PLUS + DIAG), (below, PLUS)):
        check_against_model(ix, values(n, d, formula), coords, radius, None, formula)
        want = _buffer.lattice_counts(n, width, offsets)
        np.testing.assert_array_equal(ix.buffer_counts(), want)
    # a reference set whose features ARE the positions: the nearest kept rows show which lattice offsets were left out
    pos_ix = N.Index(coords)
    try:
        inner = 12 * width + 12  # a row with all eight lattice neighbours
        for radius, nearest2 in ((1.0, 2.0), (math.sqrt(2.0), 4.0), (below, 2.0)):
            pos_ix.set_buffer(coords, radius)
            dist, idx = call(pos_ix, 4, formula)
            np.testing.assert_array_equal(dist[inner], np.full(4, math.sqrt(nearest2)))  # diagonals, or the rows two away
            want_d, want_i = _buffer.buffered_kneighbors(coords, coords, radius, 4, formula=formula)
            np.testing.assert_array_equal(idx, want_i)
            np.testing.assert_array_equal(dist, want_d)
    finally:
        pos_ix.close()


@pytest.mark.parametrize("formula", ["expanded", "direct"])
@pytest.mark.parametrize("n,d", [(37, 3), (700, 13), (1100, 3)])
def test_equivalences_with_the_grouped_call(N, indexes, n, d, formula):
    """Distinct positions at radius 0 are singleton groups; 1-column positions that ARE the codes, at radius 0 and 0.5,
    are those groups (co-located means same group, other groups are at least 1 away): bit for bit the grouped call."""
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    codes = codes_of(n)
    for grouped_codes, coords, radii in ((_groups.singletons(n), _buffer.uniform_square(n, 2, seed=n), (0.0,)),
                                         (codes, codes.astype(np.float64), (0.0, 0.5))):
        assert len(np.unique(coords, axis=0)) == len(np.unique(grouped_codes))
        ix.set_buffer(None)
        ix.set_groups(grouped_codes)
        want = {(k, det): call(ix, k, formula, det) for k in KS for det in (True, False)}
        assert ix.debug_last_buffer()["mask"] == 1
        ix.set_groups(None)
        for radius in radii:
            ix.set_buffer(coords, radius)
            for (k, det), (want_d, want_i) in want.items():
                dist, idx = call(ix, k, formula, det)
                np.testing.assert_array_equal(idx, want_i)
                np.testing.assert_array_equal(dist, want_d)
            assert ix.debug_last_buffer()["mask"] == 2
            np.testing.assert_array_equal(ix.buffer_counts(), np.bincount(grouped_codes)[grouped_codes])


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_a_cluster_that_covers_a_column_step(N, indexes, formula):
    """Rows 500 .. 1099 of 1,100 sit inside one radius: for each of them the second step (columns 512 .. 1023) and the
    third are masked whole, and 500 candidates remain."""
    n, d = 1100, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    coords, who = _buffer.cluster(n, 600, 0.05, seed=2, first=500)
    check_against_model(ix, values(n, d, formula), coords, 0.05, None, formula, ks=(5, 150))
    counts = ix.buffer_counts()
    assert (counts[who] == 600).all() and counts.max() == 600
    _, idx = call(ix, 150, formula)
    assert (idx[who] < 500).all()


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_windows_carry_the_global_row(N, indexes, formula):
    n, d = 700, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    coords, radius = _buffer.uniform_square(n, 2, seed=9), _buffer.radius_for(n, 2)
    for codes in (None, codes_of(n)):
        ix.set_groups(codes)
        ix.set_buffer(coords, radius)
        for decimals in (10, 0):  # (decimals = 0 ties many: the reorder's second key is |index - global row|)
            full_d, full_i = ix.kneighbors_grouped(5, deterministic=True, decimals=decimals, formula=FORMULAS[formula])
            dist, idx = ix.kneighbors_grouped(5, deterministic=True, decimals=decimals, formula=FORMULAS[formula],
                                              row_offset=300, n_rows=100)
            assert idx.shape == (100, 5)
            np.testing.assert_array_equal(idx, full_i[300:400])
            np.testing.assert_array_equal(dist, full_d[300:400])
            want_d, want_i = _buffer.buffered_from_values(values(n, d, formula)[300:400], np.arange(300, 400), coords, radius,
                                                          5, codes=codes, decimals=decimals)
            np.testing.assert_array_equal(idx, want_i)
            np.testing.assert_array_equal(dist, want_d)
    for bad in (dict(row_offset=650, n_rows=100), dict(row_offset=-1, n_rows=10)):
        with pytest.raises(N.HipBackendError, match="outside the 700 reference rows") as e:
            call(ix, 5, formula, **bad)
        assert e.value.code == N.ERR_INVALID


def test_counts_with_and_without_groups(N, indexes):
    """buffer_counts alone (no scan before it), under each mask and both; groups alone count their group sizes."""
    n, d = 1100, 3
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    codes = codes_of(n)
    sizes = np.bincount(codes)[codes]
    for c in (1, 2, 3):
        coords, radius = _buffer.uniform_square(n, c, seed=c), _buffer.radius_for(n, c, 9.0)
        ix.set_groups(None)
        ix.set_buffer(coords, radius)
        alone = ix.buffer_counts()
        np.testing.assert_array_equal(alone, _buffer.excluded_counts(coords, radius))
        ix.set_groups(codes)
        both = ix.buffer_counts()
        np.testing.assert_array_equal(both, _buffer.excluded_counts(coords, radius, codes))
        assert (both >= alone).all() and (both >= sizes).all() and (both > alone).any()
        assert alone.dtype == np.int64 and alone.shape == (n,)
    ix.set_buffer(None)
    np.testing.assert_array_equal(ix.buffer_counts(), sizes)
    ix.set_groups(None)
    with pytest.raises(N.HipBackendError, match="needs sknnr_index_set_buffer or sknnr_index_set_groups first") as e:
        ix.buffer_counts()
    assert e.value.code == N.ERR_INVALID


@pytest.mark.parametrize("with_groups", [False, True])
def test_the_refusal_boundary(N, indexes, with_groups):
    """k = n_ref - max(excluded) is served; one more is refused before the scan is launched."""
    n, d = 37, 3
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    codes = codes_of(n) if with_groups else None
    coords, radius = _buffer.uniform_square(n, 2, seed=5), _buffer.radius_for(n, 2)
    counts = _buffer.excluded_counts(coords, radius, codes)
    worst, row = int(counts.max()), int(np.argmax(counts))
    k = n - worst
    ix.set_groups(codes)
    ix.set_buffer(coords, radius)
    want_d, want_i = _buffer.buffered_from_values(values(n, d, "direct"), np.arange(n), coords, radius, k, codes=codes)
    dist, idx = call(ix, k, "direct")
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(dist, want_d)
    assert ix.debug_last_grouped()["k"] == k
    ix.kneighbors_host(fit_rows(n, d)[:4], ix.make_opts(2))  # (any other search call zeroes the records)
    before = ix.stats()
    with pytest.raises(N.HipBackendError, match=rf"Expected n_neighbors <= n_samples_fit - max\(excluded\), but n_neighbors = {k + 1}, "
                                                rf"n_samples_fit = {n}, max\(excluded\) = {worst} \(row {row}\)") as e:
        call(ix, k + 1, "direct")
    assert e.value.code == N.ERR_K_TOO_LARGE
    assert all(v == 0 for v in ix.debug_last_grouped().values())  # no scan
    assert all(v == 0 for v in ix.debug_last_buffer().values())
    assert ix.stats()["queries"] == before["queries"]


def test_masks_are_state_that_clears(N, indexes):
    n, d = 700, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    codes = codes_of(n)
    coords, radius = _buffer.uniform_square(n, 2, seed=3), _buffer.radius_for(n, 2)
    full = values(n, d, "expanded")
    rows = np.arange(n)
    groups_only = _groups.grouped_from_values(full, rows, codes, 5)
    buffer_only = _buffer.buffered_from_values(full, rows, coords, radius, 5)
    both = _buffer.buffered_from_values(full, rows, coords, radius, 5, codes=codes)
    assert (groups_only[1] != buffer_only[1]).any() and (both[1] != buffer_only[1]).any() and (both[1] != groups_only[1]).any()

    def same(got, want):
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], want[0])

    ix.set_groups(None)
    ix.set_buffer(coords, radius)
    same(call(ix, 5, "expanded"), buffer_only)
    ix.set_groups(codes)  # buffered, then both
    same(call(ix, 5, "expanded"), both)
    ix.set_buffer(None)  # buffer cleared: the groups-only result, by the groups-only instantiation
    same(call(ix, 5, "expanded"), groups_only)
    assert ix.debug_last_buffer()["mask"] == 1 and ix.debug_last_buffer()["c"] == 0
    ix.set_buffer(coords, radius)
    ix.set_groups(None)  # groups cleared: the buffer-only result
    same(call(ix, 5, "expanded"), buffer_only)
    ix.set_buffer(None)  # neither: today's refusal, today's text
    with pytest.raises(N.HipBackendError, match="needs sknnr_index_set_groups first") as e:
        call(ix, 5, "expanded")
    assert e.value.code == N.ERR_INVALID


def test_many_workgroups_and_a_grid_stride_pass(N):
    """8,200 rows: 1,025 passes on 1,024 workgroups.  The model answers a seeded sample of 200 rows."""
    n, d, k = 8_200, 3, 5
    fit = synth.make_features(n, d, seed=3)
    coords, radius = _buffer.uniform_square(n, 2, seed=1), _buffer.radius_for(n, 2)
    codes = _groups.random_sizes(n, 1, 6, seed=1)
    rows = np.sort(np.random.default_rng(2).choice(n, 200, replace=False))
    rows[-1] = n - 1  # (the row of the grid-stride pass)
    ix = N.Index(fit)
    try:
        for use_codes in (None, codes):
            ix.set_groups(use_codes)
            ix.set_buffer(coords, radius)
            np.testing.assert_array_equal(ix.buffer_counts(), _buffer.excluded_counts(coords, radius, use_codes))
            for formula in ("expanded", "direct"):
                dist, idx = call(ix, k, formula)
                assert ix.debug_last_grouped()["workgroups"] == 1024 and ix.debug_last_grouped()["rows"] == n
                want_d, want_i = _buffer.buffered_kneighbors(fit, coords, radius, k, codes=use_codes, formula=formula, rows=rows)
                np.testing.assert_array_equal(idx[rows], want_i)
                np.testing.assert_array_equal(dist[rows], want_d)
    finally:
        ix.close()


def test_set_buffer_refusals(N):
    ix = N.Index(fit_rows(37, 3))
    try:
        ok = _buffer.uniform_square(37, 2, seed=0)
        for bad, text in (((ok[:36], 1.0), r"one position per reference row \(37\), got 36"),
                          ((np.zeros((37, 4)), 1.0), "1 to 3 columns, got 4"),
                          ((ok, -1.0), "radius must be finite and >= 0"),
                          ((ok, float("nan")), "radius must be finite and >= 0"),
                          ((ok, float("inf")), "radius must be finite and >= 0")):
            with pytest.raises(N.HipBackendError, match=text) as e:
                ix.set_buffer(*bad)
            assert e.value.code == N.ERR_INVALID
        for v in (np.nan, np.inf):
            pos = ok.copy()
            pos[7, 1] = v
            with pytest.raises(N.HipBackendError, match="positions must be finite, got .* at row 7, column 1") as e:
                ix.set_buffer(pos, 1.0)
            assert e.value.code == N.ERR_INVALID
        with pytest.raises(N.HipBackendError, match="needs sknnr_index_set_groups first"):  # nothing was kept
            call(ix, 1, "direct")
    finally:
        ix.close()


def test_debug_record_and_counters(N, indexes):
    n, d = 700, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    coords, radius = _buffer.uniform_square(n, 3, seed=6), _buffer.radius_for(n, 3)
    codes = codes_of(n)
    ix.set_groups(codes)
    ix.set_buffer(coords, radius)
    counts = _buffer.excluded_counts(coords, radius, codes)
    before = ix.stats()
    call(ix, 5, "direct")
    rec = ix.debug_last_buffer()
    assert rec["mask"] == 3 and rec["c"] == 3
    assert rec["max_excluded"] == counts.max() and rec["min_excluded"] == counts.min()
    assert rec["argmax_row"] == int(np.argmax(counts)) and rec["reserved"] == 0
    # 3 blocks of 256 rows, each in two shares of the two 512-row tiles; a tile is three float64 columns and the codes
    assert rec["count_workgroups"] == 6 and rec["count_lds_bytes"] == 512 * (3 * 8 + 4)
    grouped = ix.debug_last_grouped()
    assert grouped["formula_plus_1"] == 2 and grouped["k"] == 5 and grouped["rows"] == n and grouped["slices"] == 1
    assert grouped["workgroups"] == (n + 7) // 8 and grouped["largest_group"] == np.bincount(codes).max()
    lds_both = grouped["lds_bytes"]
    after = ix.stats()
    assert after["queries"] - before["queries"] == n
    assert after["exact_only_queries"] - before["exact_only_queries"] == n
    ix.set_buffer(None)
    call(ix, 5, "direct")
    assert lds_both - ix.debug_last_grouped()["lds_bytes"] == 8 * 3 * 8  # the positions of a pass's eight queries
    rec = ix.debug_last_buffer()  # groups alone: nothing is counted by the search
    assert rec["mask"] == 1 and rec["c"] == 0 and rec["max_excluded"] == np.bincount(codes).max()
    assert rec["min_excluded"] == 0 and rec["count_workgroups"] == 0 and rec["count_lds_bytes"] == 0
    ix.kneighbors_host(fit_rows(n, d)[:10], ix.make_opts(5))
    assert all(v == 0 for v in ix.debug_last_buffer().values())
