"""Every coarse2_kernel instance that default dispatch reaches, pinned bit for bit to the oracle.

The second-generation pre-filter (coarse2.hip.h) serves every headline number, but most parity tests use fewer
reference rows than use_coarse2 needs and so run coarse_kernel, and a call of fewer than about 65k rows goes whole to the
4-wave thin variant.  Here every call names the launch it expects (tests/_prefilter_dispatch.py restates the dispatch),
asserts that ``Index.debug_last_prefilter()`` reports exactly that launch, compares indices and distances with
``oracle.kneighbors`` (deterministic reorder, row_offset 1000, plus a deterministic=False subset), and bounds the share
of rows that the certificate hands to the exact scan: a pre-filter that ranks badly must not hide behind the fall-back.

Instances: 4,500 reference rows (synth.make_problem, 24 duplicated reference rows, 16 queries that copy a reference
row), d = 13 / 32 / 41 / 64 (one per K-step count; 13 and 41 pad their last K-step).  Bulk calls have 66,893 rows, which
is all-bulk at 16 and at 12 waves; thin calls take the first 6,144 of them.  Each runs with the cell order forced on
(SKNNR_CELLS=6, which is depth 3 at this size) and forced off (SKNNR_CELLS=0).

COVERAGE below lists all 42 reachable (KS, M, E) combinations: list length M, rank beyond the list E.  For each it names
the test_instance cases (d, kk) that launch it.  Each such case runs at the bulk wave count given and at 4 waves
(thin).  kk is the k of a call on given rows; test_self_queries repeats every kk >= 2 as X=None with k = kk - 1.  kk
takes both ends of every band, so both the sentinel count (E = 0) and every rank are run.  One neighbour at three
and four K-steps (kk = 1 at d = 41, 64) has no second-generation kernel; those cases assert generation 1.

Finding, not fixed here: at 4,500 reference rows the pooled-list instances (E > 0) hand a large share of their rows to
the exact scan, growing with the rank M + E.  Largest shares measured on an MI355X with the synthetic law: lists of 8 at
rank 12 / 15 / 16: 6 / 12 / 22 %, lists of 12 at rank 22 / 24: 34 / 44 %, lists of 16 at rank 27 / 31 / 32: 55 / 93 / 98 %;
the crafted laws reach 25-92 % (hand-over) and 94 % (two cells).  The answers stay bit-exact; only the pre-filter's
work is wasted.  E = 0 lists and the first-generation kernel stay under 5 % (at most 4.0 % measured).  FALLBACK_POOLED
pins the measured shares so that they cannot grow unnoticed.  The seed window at this size is one stage of tiles, so the
starting threshold of rank M + E is drawn from few per-unit minima; that this is the cause is a likely explanation, not a
measured one.

Teeth (scratch builds, never committed): with the skip margin of launch_coarse2_waves set to zero, 52 tests of this module
fail on wrong neighbours; with the certificate's eps_units2 set to zero, 34 fail on wrong neighbours.

Two compiled instances are unreachable under default dispatch: lists of 6 with rank 9 (6 .. 7 neighbours go to lists of
8 wherever that kernel exists) and lists of 16 with rank 22 (16 .. 20 neighbours go to lists of 12).  Only process-static
environment knobs reach them, and this module does not set those.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import _prefilter_dispatch as P

N_REF = 4_500
NQ_BULK = 66_893
NQ_THIN = 6_144
ROW_OFFSET = 1_000
WIDTHS = (13, 32, 41, 64)
KK_BANDS = (1, 2, 5, 6, 7, 8, 10, 11, 13, 14, 15, 16, 20, 21, 23, 24, 25, 26, 30, 31)
FALLBACK_MAX = 0.05  # share of a call's rows the certificate may hand to the exact scan
# Pooled lists (E > 0) at this reference-set size, per law and (M, E): the largest share measured on an MI355X over every
# call of that kind in this module, x 1.2 + 2 points, at most 0.99 (module docstring: a finding, pinned so that it cannot
# grow unnoticed)
FALLBACK_POOLED = {
    "synth": {(8, 4): 0.10, (8, 7): 0.17, (8, 8): 0.29, (12, 10): 0.43, (12, 12): 0.55, (16, 11): 0.69, (16, 15): 0.99,
              (16, 16): 0.99},
    "hand_over": {(8, 4): 0.32, (8, 8): 0.68, (12, 10): 0.77, (12, 12): 0.81, (16, 11): 0.88, (16, 15): 0.94,
                  (16, 16): 0.99},
    "one_cell": {(12, 10): 0.11},
    "two_cells": {(12, 10): 0.99},
    "raster": {(12, 10): 0.41},
    "affine": {(12, 10): 0.38},
}

# (KS, M, E): (d, kk of the test_instance cases that launch it, waves of its bulk launch)
COVERAGE = {
    (1, 2, 0): (13, (1,), 16),
    (1, 6, 0): (13, (2, 5), 16),
    (1, 8, 0): (13, (6, 7), 16),
    (1, 8, 4): (13, (8, 10), 16),
    (1, 8, 7): (13, (11, 13), 16),
    (1, 8, 8): (13, (14, 15), 16),
    (1, 12, 10): (13, (16, 20), 16),
    (1, 12, 12): (13, (21, 23), 16),
    (1, 16, 11): (13, (24, 25), 12),
    (1, 16, 15): (13, (26, 30), 12),
    (1, 16, 16): (13, (31,), 12),
    (2, 2, 0): (32, (1,), 16),
    (2, 6, 0): (32, (2, 5), 16),
    (2, 8, 0): (32, (6, 7), 16),
    (2, 8, 4): (32, (8, 10), 16),
    (2, 8, 7): (32, (11, 13), 16),
    (2, 8, 8): (32, (14, 15), 16),
    (2, 12, 10): (32, (16, 20), 12),
    (2, 12, 12): (32, (21, 23), 12),
    (2, 16, 11): (32, (24, 25), 12),
    (2, 16, 15): (32, (26, 30), 12),
    (2, 16, 16): (32, (31,), 12),
    (3, 6, 0): (41, (2, 5), 16),
    (3, 8, 0): (41, (6, 7), 16),
    (3, 8, 4): (41, (8, 10), 16),
    (3, 8, 7): (41, (11, 13), 16),
    (3, 8, 8): (41, (14, 15), 16),
    (3, 12, 10): (41, (16, 20), 12),
    (3, 12, 12): (41, (21, 23), 12),
    (3, 16, 11): (41, (24, 25), 12),
    (3, 16, 15): (41, (26, 30), 12),
    (3, 16, 16): (41, (31,), 12),
    (4, 6, 0): (64, (2, 5), 16),
    (4, 8, 0): (64, (6, 7), 12),
    (4, 8, 4): (64, (8, 10), 12),
    (4, 8, 7): (64, (11, 13), 12),
    (4, 8, 8): (64, (14, 15), 12),
    (4, 12, 10): (64, (16, 20), 12),
    (4, 12, 12): (64, (21, 23), 12),
    (4, 16, 11): (64, (24, 25), 12),
    (4, 16, 15): (64, (26, 30), 12),
    (4, 16, 16): (64, (31,), 12),
}

gpu = pytest.mark.gpu


def test_coverage_table_matches_dispatch():
    """The table above is what dispatch does: exactly the reachable instances, each launched by the cases it names, in
    bulk at the waves it names and thin at 4 waves (no GPU: the restatement only)."""
    assert sorted(COVERAGE) == P.reachable_instances()
    assert len(COVERAGE) == 42
    covered = {}
    for d in WIDTHS:
        for kk in KK_BANDS:
            bulk = P.expected_launch(N_REF, d, kk, NQ_BULK, cells_env=6)
            thin = P.expected_launch(N_REF, d, kk, NQ_THIN, cells_env=6)
            if bulk["generation"] != 2:
                assert kk == 1 and P.ks_of(d) >= 3 and bulk["generation"] == thin["generation"] == 1
                continue
            key = (bulk["ks"], bulk["m_list"], bulk["rank_extra"])
            assert (bulk["thin_rows"], thin["bulk_rows"], thin["thin_rows"]) == (0, 0, NQ_THIN), (d, kk)
            assert bulk["bulk_rows"] >= NQ_BULK and bulk["cell_depth"] == thin["cell_depth"] == 3
            covered.setdefault(key, (d, [], bulk["bulk_waves"]))[1].append(kk)
    assert {key: (d, tuple(kks), w) for key, (d, kks, w) in covered.items()} == COVERAGE
    # the launch-arithmetic edges below, re-derived from launch_coarse2
    assert [P.coarse2_split(n, 16) for n in (65_536, 65_537, 327_603, 328_704)] == [
        (0, 65_536), (66_560, 0), (262_144, 65_536), (328_704, 0)]
    assert [P.coarse2_split(n, 12) for n in (65_280, 65_281, 261_811, 262_656)] == [
        (0, 65_280), (66_048, 0), (196_608, 65_280), (262_656, 0)]
    assert (P.min_coarse2_n_ref(2), P.min_coarse2_n_ref(4)) == (3_585, 3_841)


def test_hand_over_layout():
    """The hand-over law's layout (no GPU): 30 clusters of 42 rows, each on the positions of one lane half only, three
    per tile, consecutive clusters on alternate halves."""
    cluster = _hand_over_clusters()
    assert cluster.max() == 29 and all((cluster == c).sum() == 42 for c in range(30))
    pos = np.flatnonzero(cluster >= 0)
    half = pos % 8 >= 4
    for c in range(30):
        on = cluster[pos] == c
        assert (half[on] == bool(c % 2)).all()
        assert np.bincount(pos[on] // 32).max() == 3


# ---------------------------------------------------------------------------------------------------------------------
# shared state: one handle per (data, environment), oracle results cached by (d, k, law)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def handles(N):
    """handles(key, ref, **env): one handle per key, created with the environment variables given (all of them are read
    at index creation), kept for the module."""
    made = {}

    def get(key, ref, **env):
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                for name, value in env.items():
                    mp.setenv(name, str(value))
                made[key] = N.Index(ref)
        return made[key]

    yield get
    for ix in made.values():
        ix.close()


@functools.lru_cache(maxsize=2)
def _problem(d, nq=NQ_BULK):
    from sknnr_amd import synth

    x_ref, _, x_q = synth.make_problem(N_REF, nq, d, t=1, n_dup_refs=24, n_dup_queries=16)
    return x_ref, x_q


_LAWS = {}  # law name -> function of d giving (reference rows, query rows or None for X=None)


@functools.lru_cache(maxsize=3)
def _oracle(d, k, law, deterministic=True):
    """The oracle's answer for the queries of ``law``, cached so that cells on / off and bulk / thin share it."""
    from oracle import oracle as O

    ref, q = _LAWS[law](d)
    if q is None:
        return O.kneighbors(ref, None, k, "expanded", deterministic=deterministic)
    return O.kneighbors(ref, q, k, "expanded", deterministic=deterministic, row_offset=ROW_OFFSET)


def _call(ix, q, k, nq=None, **opts):
    """One kneighbors call on fresh statistics: (dist, idx, launch record, share of rows sent to the exact scan)."""
    exclude_self = q is None
    row_offset = 0 if exclude_self else ROW_OFFSET
    ix.reset_stats()
    dist, idx = ix.kneighbors_host(q, ix.make_opts(k, exclude_self=exclude_self, row_offset=row_offset, **opts), nq=nq)
    st = ix.stats()
    rows = len(idx)
    assert st["queries"] == rows and st["exact_only_queries"] == 0 and st["coarse_queries"] == rows, st
    return dist, idx, ix.debug_last_prefilter(), st["exact_fallbacks"] / rows


def _fallback_bound(rec, law):
    """The pinned fall-back share of a launch: FALLBACK_MAX where the lists hold kk + 1 (E = 0) or the first-generation
    kernel ran; pooled ranks (E > 0) are pinned per law and (M, E) in FALLBACK_POOLED."""
    if rec["generation"] != 2 or rec["rank_extra"] == 0:
        return FALLBACK_MAX
    return FALLBACK_POOLED[law][(rec["m_list"], rec["rank_extra"])]


def _check(got, want, expect, record, late, what="", law="synth"):
    """The launch record and the answer bit for bit; the fall-back share is recorded as a test property and an excess
    over its pinned bound is collected in ``late``, so that a test still runs its other calls (the caller asserts
    ``late`` empty at its end)."""
    dist, idx, rec, fallback = got
    record(f"fallback {what}".strip(), round(fallback, 6))
    od, oi = want
    assert rec == expect, f"{what}: launched {rec}, dispatch says {expect}"
    np.testing.assert_array_equal(idx, oi, err_msg=what)
    np.testing.assert_array_equal(dist, od, err_msg=what)
    bound = _fallback_bound(rec, law)
    if fallback > bound:
        late.append(f"{what}: {fallback:.2%} of the rows failed the certificate (pinned: {bound:.0%})")


# ---------------------------------------------------------------------------------------------------------------------
# the instance matrix
# ---------------------------------------------------------------------------------------------------------------------
_LAWS["synth"] = lambda d: _problem(d)
_LAWS["self"] = lambda d: (_problem(d)[0], None)


@gpu
@pytest.mark.parametrize("kk", KK_BANDS)
@pytest.mark.parametrize("d", WIDTHS)
def test_instance(N, handles, record_property, d, kk):
    """One (KS, kk) case of COVERAGE: bulk (66,893 rows) and thin (its first 6,144 rows), cells on and off."""
    x_ref, x_q = _problem(d)
    od, oi = _oracle(d, kk, "synth")
    late = []
    for cells in (6, 0):
        ix = handles(("synth", d, cells), x_ref, SKNNR_CELLS=cells)
        _check(_call(ix, x_q, kk), (od, oi), P.expected_launch(N_REF, d, kk, NQ_BULK, cells), record_property, late,
               f"bulk, cells {cells}")
        _check(_call(ix, x_q[:NQ_THIN], kk), (od[:NQ_THIN], oi[:NQ_THIN]), P.expected_launch(N_REF, d, kk, NQ_THIN, cells),
               record_property, late, f"thin, cells {cells}")
    assert not late, late


@gpu
@pytest.mark.parametrize("d, kk", [(13, 2), (13, 14), (32, 21), (41, 8), (41, 25), (64, 6), (64, 31)])
def test_instance_without_deterministic_order(N, handles, record_property, d, kk):
    """deterministic=False: the lists come back in the engine's own order, ties included (bulk and thin, cells on)."""
    x_ref, x_q = _problem(d)
    od, oi = _oracle(d, kk, "synth", deterministic=False)
    ix = handles(("synth", d, 6), x_ref, SKNNR_CELLS=6)
    late = []
    _check(_call(ix, x_q, kk, deterministic=False), (od, oi), P.expected_launch(N_REF, d, kk, NQ_BULK, 6), record_property,
           late, "bulk")
    _check(_call(ix, x_q[:NQ_THIN], kk, deterministic=False), (od[:NQ_THIN], oi[:NQ_THIN]),
           P.expected_launch(N_REF, d, kk, NQ_THIN, 6), record_property, late, "thin")
    assert not late, late


@gpu
@pytest.mark.parametrize("kk", [kk for kk in KK_BANDS if kk >= 2])
@pytest.mark.parametrize("d", WIDTHS)
def test_self_queries(N, handles, record_property, d, kk):
    """X=None: the reference rows query themselves with k = kk - 1 (kk neighbours searched), cells on and off."""
    x_ref, _ = _problem(d)
    want = _oracle(d, kk - 1, "self")
    late = []
    for cells in (6, 0):
        ix = handles(("synth", d, cells), x_ref, SKNNR_CELLS=cells)
        _check(_call(ix, None, kk - 1, nq=N_REF), want, P.expected_launch(N_REF, d, kk, N_REF, cells), record_property, late,
               f"cells {cells}")
    assert not late, late


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic: where launch_coarse2 switches between the bulk and the thin launch
# ---------------------------------------------------------------------------------------------------------------------
NQ_EDGES = 328_704
_LAWS["edges"] = lambda d: _problem(d, NQ_EDGES)


@gpu
@pytest.mark.parametrize("k, nq, bulk, thin", [
    (5, 65_536, 0, 65_536),            # 16 waves: 64 workgroups, all of them thin
    (5, 65_537, 66_560, 0),            # 65 workgroups: more than a quarter of the CUs -- all bulk
    (5, 327_603, 262_144, 65_536),     # one full round + 64 thin: the side-stream finaliser fork
    (5, 328_704, 328_704, 0),          # one full round + 65
    (26, 65_280, 0, 65_280),           # 12 waves (lists of 16): 85 workgroups, all of them thin
    (26, 65_281, 66_048, 0),
    (26, 261_811, 196_608, 65_280),
    (26, 262_656, 262_656, 0),
])
def test_launch_arithmetic_edges(N, handles, record_property, k, nq, bulk, thin):
    """Row counts at both sides of the bulk / thin switch at 16 and 12 waves (d = 13): the launch record's row split and
    the answer, cells on and off.  The first rows of one 328,704-row query set, one oracle result per k."""
    d = 13
    x_ref, x_q = _problem(d, NQ_EDGES)
    od, oi = _oracle(d, k, "edges")
    assert P.coarse2_split(nq, P.coarse2_waves(1, P.coarse_list_len(N_REF, d, k))) == (bulk, thin)
    late = []
    for cells in (6, 0):
        ix = handles(("synth", d, cells), x_ref, SKNNR_CELLS=cells)
        got = _call(ix, x_q[:nq], k)
        assert (got[2]["bulk_rows"], got[2]["thin_rows"]) == (bulk, thin)
        _check(got, (od[:nq], oi[:nq]), P.expected_launch(N_REF, d, k, nq, cells), record_property, late, f"cells {cells}")
    assert not late, late


@gpu
@pytest.mark.parametrize("d, n_ref", [(32, 3_585), (32, 3_584), (64, 3_841), (64, 3_840)])
def test_smallest_second_generation_reference_set(N, O, record_property, d, n_ref):
    """The fewest reference rows the second-generation kernel takes (128 tiles after rounding up to whole stages: the last
    stage is mostly padding and its last live tile holds one row), and one row fewer (first generation): both equal the
    oracle, at 5 and 20 neighbours, cells on and off, bulk."""
    from sknnr_amd import synth

    x_ref, _, x_q = synth.make_problem(n_ref, NQ_BULK, d, t=1, n_dup_refs=24, n_dup_queries=16)
    gen = 2 if n_ref == P.min_coarse2_n_ref(P.ks_of(d)) else 1
    late = []
    for k in (5, 20):
        want = O.kneighbors(x_ref, x_q, k, "expanded", row_offset=ROW_OFFSET)
        for cells in (6, 0):
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("SKNNR_CELLS", str(cells))
                ix = N.Index(x_ref)
            try:
                expect = P.expected_launch(n_ref, d, k, NQ_BULK, cells)
                assert expect["generation"] == gen
                _check(_call(ix, x_q, k), want, expect, record_property, late, f"k {k}, cells {cells}")
            finally:
                ix.close()
    assert not late, late


# ---------------------------------------------------------------------------------------------------------------------
# data laws aimed at specific code
# ---------------------------------------------------------------------------------------------------------------------
HAND_OVER_RADIUS = 0.1


def _hand_over_clusters():
    """Image position -> cluster of the hand-over law (-1: background).  acc_row (coarse.hip.h) gives lane half 0 the
    positions p % 8 < 4 of a tile and half 1 the others.  A cluster holds three positions of one half in each of 14
    consecutive tiles, and consecutive clusters alternate halves.  Three per tile, because a unit that brings one lane
    more hits than its queue takes (kQueueCap = 5, up to 2 left from the last visit) poisons the query (coarse2.hip.h):
    this law is about the hand-over, not about that rule."""
    cluster = np.full(N_REF, -1)
    c = 0
    for t0 in (4, 50, 96):  # three ranges of 14 tiles, background rows between them
        for j in range(5):
            for h in (0, 1):
                slots = [p for p in range(32) if (p % 8 >= 4) == bool(h)][3 * j:3 * j + 3]
                cluster[[32 * (t0 + t) + s for t in range(14) for s in slots]] = c
                c += 1
    return cluster


def _hand_over_problem(d):
    """Tight clusters (_hand_over_clusters) inside a Gaussian background, queries near the cluster centres: every query's
    first 31 neighbours are rows of its cluster, so one lane's list overflows and every pooled list hands entries over to
    its partner.  With SKNNR_IMAGE_ORDER=0 and SKNNR_CELLS=0, image position = row index."""
    rng = np.random.default_rng([31, d])
    cluster = _hand_over_clusters()
    n_c = cluster.max() + 1
    centres = rng.standard_normal((n_c, d))
    x = rng.standard_normal((N_REF, d))
    for c in range(n_c):
        rows = np.flatnonzero(cluster == c)
        x[rows] = centres[c] + HAND_OVER_RADIUS * rng.standard_normal((len(rows), d))
    q = centres[np.arange(NQ_BULK) % n_c] + 0.3 * HAND_OVER_RADIUS * rng.standard_normal((NQ_BULK, d))
    return x, q


_LAWS["hand_over"] = _hand_over_problem


@gpu
@pytest.mark.parametrize("kk", [8, 10, 15, 16, 20, 23, 24, 26, 31])
@pytest.mark.parametrize("d", [13, 41])
def test_hand_over_between_pooled_lists(N, handles, record_property, d, kk):
    """Lists of 8, 12 and 16 where every query's neighbours crowd one lane's list (bulk and thin): the answers are exact
    and the fall-back share stays within its pinned bound."""
    x_ref, x_q = _hand_over_problem(d)
    od, oi = _oracle(d, kk, "hand_over")
    cluster = _hand_over_clusters()
    assert (cluster[oi] == (np.arange(NQ_BULK) % (cluster.max() + 1))[:, None]).all(), "the law does not hold"
    ix = handles(("hand_over", d), x_ref, SKNNR_IMAGE_ORDER=0, SKNNR_CELLS=0)
    late = []
    _check(_call(ix, x_q, kk), (od, oi), P.expected_launch(N_REF, d, kk, NQ_BULK), record_property, late, "bulk",
           "hand_over")
    _check(_call(ix, x_q[:NQ_THIN], kk), (od[:NQ_THIN], oi[:NQ_THIN]), P.expected_launch(N_REF, d, kk, NQ_THIN),
           record_property, late, "thin", "hand_over")
    assert not late, late


def _principal_offset(x_ref, signs):
    """A point of the reference cloud at (1.5, 1.2, 1.2) standard deviations along its three leading principal axes, with
    the signs given: far, against the jitter below, from the median split planes of the cell tree's first levels."""
    mean = x_ref.mean(axis=0)
    _, sv, vt = np.linalg.svd(x_ref - mean, full_matrices=False)
    sd = sv[:3] / np.sqrt(len(x_ref))
    return mean + sum(s * a * sd[i] * vt[i] for i, (s, a) in enumerate(zip(signs, (1.5, 1.2, 1.2))))


def _one_cell_problem(d):
    """Every query within a small jitter of one point: one bucket holds (practically) every row."""
    x_ref, _ = _problem(d)
    rng = np.random.default_rng([41, d])
    return x_ref, _principal_offset(x_ref, (1, 1, -1)) + 0.05 * rng.standard_normal((NQ_BULK, d))


def _two_cell_problem(d):
    """Queries near two opposite points of the cloud, interleaved row by row: two distant cells, each bucket a
    scattered half of the call."""
    x_ref, _ = _problem(d)
    rng = np.random.default_rng([43, d])
    centres = np.stack([_principal_offset(x_ref, (1, 1, 1)), _principal_offset(x_ref, (-1, -1, -1))])
    return x_ref, centres[np.arange(NQ_BULK) % 2] + 0.05 * rng.standard_normal((NQ_BULK, d))


_LAWS["one_cell"] = _one_cell_problem
_LAWS["two_cells"] = _two_cell_problem


@gpu
@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("law", ["one_cell", "two_cells"])
def test_bucketing_laws(N, handles, record_property, law, k):
    """Cells on, bulk calls, d = 32: queries crowded into one cell, and split between two distant ones."""
    d = 32
    x_ref, x_q = _LAWS[law](d)
    ix = handles(("synth", d, 6), x_ref, SKNNR_CELLS=6)
    late = []
    _check(_call(ix, x_q, k), _oracle(d, k, law), P.expected_launch(N_REF, d, k, NQ_BULK, 6), record_property, late, law=law)
    assert not late, late


def _raster_problem(d):
    """Reference rows on a raster's value range; query rows that a uint8 raster holds (also sent as float32)."""
    x_ref, x_q = _problem(d)
    return 20.0 * x_ref + 128.0, np.clip(np.rint(20.0 * x_q + 128.0), 0, 255)


_LAWS["raster"] = _raster_problem


@gpu
@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_narrow_query_rows_with_cells(N, handles, record_property, dtype, k):
    """query_dtype rows, cells on, bulk (d = 13): the prep kernel widens them and names their cells in registers; the
    answer is the float64 call's on the widened rows, and the oracle's."""
    d = 13
    x_ref, x_q = _raster_problem(d)
    q = x_q.astype(dtype)
    ix = handles(("raster", d), x_ref, SKNNR_CELLS=6)
    expect = P.expected_launch(N_REF, d, k, NQ_BULK, 6)
    want = _oracle(d, k, "raster")
    late = []
    _check(_call(ix, q, k, query_dtype=N.dtype_code(dtype)), want, expect, record_property, late, "narrow rows", "raster")
    _check(_call(ix, q.astype(np.float64), k), want, expect, record_property, late, "float64 rows", "raster")
    assert not late, late


@gpu
@pytest.mark.parametrize("k", [5, 20])
def test_affine_index_with_cells(N, O, handles, record_property, k):
    """The GNN / MSN query path with cells on, bulk: raw 20-column rows, the index's affine map to 13 columns in the prep
    kernel, each row's cell named from the transformed values in registers."""
    rng = np.random.default_rng(47)
    d_in, d = 20, 13
    raw_ref = rng.standard_normal((N_REF, d_in)) * 3.0 + 1.0
    raw_q = rng.standard_normal((NQ_BULK, d_in)) * 3.0 + 1.0
    raw_q[:16] = raw_ref[::200][:16]
    center, scale = raw_ref.mean(axis=0), raw_ref.std(axis=0)
    proj = rng.standard_normal((d_in, d)) / np.sqrt(d_in)
    ref_t = O.affine(raw_ref, center, scale, proj)
    ix = handles(("affine",), ref_t, SKNNR_CELLS=6)
    ix.set_affine(d_in, center, scale, proj)
    want = O.kneighbors(ref_t, O.affine(raw_q, center, scale, proj), k, "expanded", row_offset=ROW_OFFSET)
    late = []
    _check(_call(ix, raw_q, k, apply_affine=True), want, P.expected_launch(N_REF, d, k, NQ_BULK, 6), record_property, late,
           law="affine")
    assert not late, late


@gpu
def test_self_queries_in_bulk(N, O, record_property):
    """X=None with 66,893 reference rows (d = 13, k = 5, cells on: depth 6): the self query is a bulk call."""
    from sknnr_amd import synth

    n_ref, d, k = NQ_BULK, 13, 5
    x_ref, _, _ = synth.make_problem(n_ref, 16, d, t=1, n_dup_refs=24)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SKNNR_CELLS", "6")
        ix = N.Index(x_ref)
    try:
        expect = P.expected_launch(n_ref, d, k + 1, n_ref, 6)
        assert expect["cell_depth"] == 6 and expect["bulk_rows"] > 0 and expect["thin_rows"] == 0
        late = []
        _check(_call(ix, None, k, nq=n_ref), O.kneighbors(x_ref, None, k, "expanded"), expect, record_property, late)
        assert not late, late
    finally:
        ix.close()
