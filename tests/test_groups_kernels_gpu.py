"""group_scan_kernel (groups.hip.h) through ``_native.Index``: every comparison is ``assert_array_equal`` on distances and
indices against the contract's numpy model (tests/_groups.py).

Shapes, the smallest at which the kernel can go wrong: 37 reference rows (less than a wave of columns), 700 (two column
steps of 512, the second partial; the last pass of 8 queries is partial), 1100 (three steps); d in 3 (tail loop only), 8
(unrolled loop only), 13 (both), 32; k in 1, 5, 9; the expanded and the direct formula on ``make_features`` rows, weighted
Hamming on ``make_forest_ids`` ids; deterministic ordering on and off.  Group laws: singletons, pairs, random sizes 1 to 7,
one group that covers a whole column step (rows 100 .. 699 of 700), a group in two pieces (the first and the last 5 rows).
One value matrix per (n, d, formula) is computed once and shared; nothing writes to it."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import _groups
from sknnr_amd import synth

pytestmark = pytest.mark.gpu

FORMULAS = {"expanded": 0, "direct": 1, "hamming": 2}
KS = (1, 5, 9)
TIE_FREE_SHAPES = [(700, 13, 5), (700, 32, 5), (37, 3, 1), (1100, 8, 9)]


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
def hamming_problem():
    ids, _ = synth.make_forest_ids(700, 1, 40)
    w = np.random.default_rng(11).uniform(0.05, 1.05, 40)
    full = _groups.value_rows(ids, np.arange(700), "hamming", w)
    for a in (ids, w, full):
        a.setflags(write=False)
    return ids, w, full


def laws(n):
    return {"singletons": _groups.singletons(n), "pairs": _groups.pairs(n), "random": _groups.random_sizes(n, 1, 7, seed=n),
            "two_piece": _groups.two_piece(n)}


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


def check_against_model(ix, full, codes, formula, ks=KS, hamming=False):
    n = full.shape[0]
    rows = np.arange(n)
    ix.set_groups(codes)
    val, idx = _groups.ranked_candidates(full, rows, codes, max(ks))
    for k in ks:
        for det in (True, False):
            want_d, want_i = _groups.finish(val[:, :k], idx[:, :k], rows, hamming=hamming, deterministic=det)
            dist, got = ix.kneighbors_grouped(k, deterministic=det, decimals=10, formula=FORMULAS[formula])
            np.testing.assert_array_equal(got, want_i, err_msg=f"k={k} det={det}")
            np.testing.assert_array_equal(dist, want_d, err_msg=f"k={k} det={det}")
            assert not (codes[got] == codes[:, None]).any()
    only_idx = ix.kneighbors_grouped(ks[-1], deterministic=False, decimals=10, formula=FORMULAS[formula],
                                     return_distance=False)
    assert only_idx[0] is None
    np.testing.assert_array_equal(only_idx[1], got)


@pytest.mark.parametrize("law", ["singletons", "pairs", "random", "two_piece"])
@pytest.mark.parametrize("formula", ["expanded", "direct"])
@pytest.mark.parametrize("d", [3, 8, 13, 32])
@pytest.mark.parametrize("n", [37, 700, 1100])
def test_euclidean_matches_the_model(N, indexes, n, d, formula, law):
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    check_against_model(ix, values(n, d, formula), laws(n)[law], formula)


@pytest.mark.parametrize("law", ["singletons", "pairs", "random", "two_piece"])
def test_hamming_matches_the_model(N, indexes, law):
    ids, w, full = hamming_problem()

    def make():
        ix = N.Index(ids)
        ix.set_hamming_weights(w)
        return ix

    check_against_model(indexes("hamming", make), full, laws(700)[law], "hamming", hamming=True)


@pytest.mark.parametrize("formula", ["expanded", "direct", "hamming"])
def test_wide_rows_in_column_chunks(N, formula):
    """d = 1025: the second column chunk is one column wide (tail loop only); the queries' columns pass through LDS
    chunk by chunk inside every step.  Hamming on 1,100 trees (a chunk of 76: unrolled loop and tail)."""
    n = 300
    if formula == "hamming":
        fit, _ = synth.make_forest_ids(n, 1, 1100, seed=4)
        w = np.random.default_rng(12).uniform(0.05, 1.05, 1100)
    else:
        fit, w = synth.make_features(n, 1025, seed=3), None
    full = _groups.value_rows(fit, np.arange(n), formula, w)
    ix = N.Index(fit)
    try:
        if w is not None:
            ix.set_hamming_weights(w)
        check_against_model(ix, full, _groups.random_sizes(n, 1, 7, seed=n), formula, ks=(5,), hamming=w is not None)
    finally:
        ix.close()


@pytest.mark.parametrize("formula", ["expanded", "direct"])
@pytest.mark.parametrize("n,d,k", TIE_FREE_SHAPES)
def test_singletons_equal_kneighbors_none(N, indexes, n, d, k, formula):
    """No boundary tie on these shapes (tests/test_groups_cpu.py asserts it): the grouped call is the X=None call."""
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    ix.set_groups(_groups.singletons(n))
    for det in (True, False):
        dist, idx = ix.kneighbors_grouped(k, deterministic=det, decimals=10, formula=FORMULAS[formula])
        opts = ix.make_opts(k, exclude_self=True, deterministic=det, formula=FORMULAS[formula])
        want_d, want_i = ix.kneighbors_host(None, opts, nq=n)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(dist, want_d)


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_a_group_that_covers_a_column_step(N, indexes, formula):
    """Rows 100 .. 699 are one group: its members have exactly 100 candidates, k = 100 takes them all, k = 101 is refused."""
    n, d = 700, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    codes = _groups.one_big_group(n, 100)
    check_against_model(ix, values(n, d, formula), codes, formula, ks=(9, 100))
    _, idx = ix.kneighbors_grouped(100, deterministic=True, decimals=10, formula=FORMULAS[formula])
    assert (np.sort(idx[100:], axis=1) == np.arange(100)).all()
    with pytest.raises(N.HipBackendError, match="Expected n_neighbors <= n_samples_fit - largest group, but n_neighbors = 101, "
                                                "n_samples_fit = 700, largest group = 600") as e:
        ix.kneighbors_grouped(101, deterministic=True, decimals=10, formula=FORMULAS[formula])
    assert e.value.code == N.ERR_K_TOO_LARGE


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_ties_on_a_lattice(N, formula):
    rng = np.random.default_rng(5)
    fit = rng.integers(0, 3, (700, 4)).astype(np.float64)
    codes = rng.integers(0, 200, 700).astype(np.int32)
    full = _groups.value_rows(fit, np.arange(700), formula)
    ix = N.Index(fit)
    try:
        check_against_model(ix, full, codes, formula, ks=(1, 5))
    finally:
        ix.close()


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_duplicate_rows(N, formula):
    base = fit_rows(350, 8)
    fit = np.vstack([base, base])
    full = _groups.value_rows(fit, np.arange(700), formula)
    ix = N.Index(fit)
    try:
        together = (np.arange(700) % 350).astype(np.int32)  # a copy and its original in one group
        check_against_model(ix, full, together, formula, ks=(5,))
        dist, _ = ix.kneighbors_grouped(5, deterministic=True, decimals=10, formula=FORMULAS[formula])
        assert (dist > 0).all()
        apart = _groups.singletons(700)
        check_against_model(ix, full, apart, formula, ks=(5,))
        dist, idx = ix.kneighbors_grouped(5, deterministic=True, decimals=10, formula=FORMULAS[formula])
        np.testing.assert_array_equal(idx[:, 0], (np.arange(700) + 350) % 700)
        assert (dist[:, 0] == 0).all() and (dist[:, 1] > 0).all()
    finally:
        ix.close()


@pytest.mark.parametrize("formula", ["expanded", "direct"])
def test_windows_carry_the_global_row(N, indexes, formula):
    n, d = 700, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    ix.set_groups(_groups.random_sizes(n, 1, 7, seed=n))
    full_d, full_i = ix.kneighbors_grouped(5, deterministic=True, decimals=10, formula=FORMULAS[formula])
    dist, idx = ix.kneighbors_grouped(5, deterministic=True, decimals=10, formula=FORMULAS[formula], row_offset=300, n_rows=100)
    assert idx.shape == (100, 5)
    np.testing.assert_array_equal(idx, full_i[300:400])
    np.testing.assert_array_equal(dist, full_d[300:400])
    # the reorder's second key is |index - global row|: a tied pair must come out as in the full call (decimals = 0 ties many)
    coarse_d, coarse_i = ix.kneighbors_grouped(5, deterministic=True, decimals=0, formula=FORMULAS[formula])
    dist, idx = ix.kneighbors_grouped(5, deterministic=True, decimals=0, formula=FORMULAS[formula], row_offset=300, n_rows=100)
    np.testing.assert_array_equal(idx, coarse_i[300:400])
    np.testing.assert_array_equal(dist, coarse_d[300:400])
    want_d, want_i = _groups.grouped_from_values(values(n, d, formula)[300:400], np.arange(300, 400),
                                                 _groups.random_sizes(n, 1, 7, seed=n), 5, decimals=0)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(dist, want_d)
    assert (coarse_i != full_i).any()  # (the coarse rounding did reorder something)
    for bad in (dict(row_offset=650, n_rows=100), dict(row_offset=-1, n_rows=10)):
        with pytest.raises(N.HipBackendError, match="outside the 700 reference rows") as e:
            ix.kneighbors_grouped(5, deterministic=True, decimals=10, formula=FORMULAS[formula], **bad)
        assert e.value.code == N.ERR_INVALID


def test_debug_record_and_counters(N, indexes):
    n, d = 700, 13
    ix = indexes((n, d), lambda: N.Index(fit_rows(n, d)))
    codes = _groups.two_piece(n)
    ix.set_groups(codes)
    before = ix.stats()
    ix.kneighbors_grouped(9, deterministic=True, decimals=10, formula=FORMULAS["direct"])
    rec = ix.debug_last_grouped()
    assert rec["formula_plus_1"] == 2 and rec["k"] == 9 and rec["rows"] == n and rec["slices"] == 1
    assert rec["largest_group"] == 10 and rec["n_groups"] == n - 10 + 1
    assert rec["workgroups"] == (n + 7) // 8 and 0 < rec["lds_bytes"] <= 160 * 1024
    after = ix.stats()
    assert after["queries"] - before["queries"] == n
    assert after["exact_only_queries"] - before["exact_only_queries"] == n
    ix.kneighbors_host(fit_rows(n, d)[:10], ix.make_opts(5))
    assert all(v == 0 for v in ix.debug_last_grouped().values())


def test_refusals(N):
    ix = N.Index(fit_rows(37, 3))
    try:
        with pytest.raises(N.HipBackendError, match="needs sknnr_index_set_groups first") as e:
            ix.kneighbors_grouped(1, deterministic=True, decimals=10, formula=0)
        assert e.value.code == N.ERR_INVALID
        bad = _groups.singletons(37)
        bad[5] = -1
        with pytest.raises(N.HipBackendError, match="group codes must be >= 0") as e:
            ix.set_groups(bad)
        assert e.value.code == N.ERR_INVALID
        with pytest.raises(N.HipBackendError, match=r"one group code per reference row \(37\), got 36") as e:
            ix.set_groups(_groups.singletons(36))
        assert e.value.code == N.ERR_INVALID
        ix.set_groups(_groups.singletons(37))
        ix.kneighbors_grouped(1, deterministic=True, decimals=10, formula=0)
        ix.set_groups(None)  # cleared: refused again
        with pytest.raises(N.HipBackendError, match="needs sknnr_index_set_groups first"):
            ix.kneighbors_grouped(1, deterministic=True, decimals=10, formula=0)
    finally:
        ix.close()


def test_many_workgroups_and_a_grid_stride_pass(N):
    """20,000 rows: 2,500 passes on 1,024 workgroups.  The model answers a seeded sample of 200 rows."""
    n, d, k = 20_000, 32, 5
    fit = synth.make_features(n, d, seed=3)
    codes = _groups.random_sizes(n, 1, 6, seed=1)
    rows = np.sort(np.random.default_rng(2).choice(n, 200, replace=False))
    ix = N.Index(fit)
    try:
        ix.set_groups(codes)
        for formula in ("expanded", "direct"):
            dist, idx = ix.kneighbors_grouped(k, deterministic=True, decimals=10, formula=FORMULAS[formula])
            assert ix.debug_last_grouped()["workgroups"] == 1024
            want_d, want_i = _groups.grouped_kneighbors(fit, codes, k, formula=formula, rows=rows)
            np.testing.assert_array_equal(idx[rows], want_i)
            np.testing.assert_array_equal(dist[rows], want_d)
            assert not (codes[idx] == codes[:, None]).any()
    finally:
        ix.close()
