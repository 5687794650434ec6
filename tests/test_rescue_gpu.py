"""The rescue re-sweep (sknnr_amd/csrc/rescue.hip.h): rows the finalisers list are swept again under the bound their
re-scored candidates give, and only what that still cannot certify reaches the float64 scan.

Every call: indices and distances are assert_array_equal to ``oracle.kneighbors``, and the record of
``Index.debug_last_rescue()`` obeys its identities -- offered = the growth of ``exact_fallbacks``; every offered row is
rescued or handed on, and the rows without a threshold and the overflowed ones are among those handed on;
``debug_last_scan()`` reports the rows handed on as the rows it consumed.

4,500 reference rows (the smallest set the instance tests use for the second-generation kernel), d = 13 / 32 / 41 / 64
(one per K-step count, two of them padded), 6,144-row thin calls and one 66,893-row bulk + thin call at d = 32.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import _rescue as R

gpu = pytest.mark.gpu
N_REF = 4_500
NQ_THIN = 6_144
NQ_BULK = 66_893
ROW_OFFSET = 1_000
WIDTHS = (13, 32, 41, 64)


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@functools.lru_cache(maxsize=8)
def _problem(d, nq=NQ_THIN, n_ref=N_REF):
    from sknnr_amd import synth

    x_ref, _, x_q = synth.make_problem(n_ref, nq, d, t=1, n_dup_refs=24, n_dup_queries=16)
    return x_ref, x_q


@pytest.fixture(scope="module")
def handles(N):
    made = {}

    def get(d):
        if d not in made:
            made[d] = N.Index(_problem(d)[0])
        return made[d]

    yield get
    for ix in made.values():
        ix.close()


def _call(ix, q, k, nq=None, row_offset=None, deterministic=True, served=None):
    """(dist, idx, rescue record) of one call on fresh statistics, the record's identities checked.  ``served``: whether
    the rescue must have been launched (None: exactly when the second-generation kernel ran and at most 12 neighbours
    were searched)."""
    exclude_self = q is None
    if row_offset is None:
        row_offset = 0 if exclude_self else ROW_OFFSET
    ix.reset_stats()
    dist, idx = ix.kneighbors_host(q, ix.make_opts(k, exclude_self=exclude_self, row_offset=row_offset, deterministic=deterministic), nq=nq)
    st, rec, scan = ix.stats(), ix.debug_last_rescue(), ix.debug_last_scan()
    assert st["queries"] == len(idx) and st["exact_only_queries"] == 0, st
    in_scope = ix.debug_last_prefilter()["generation"] == 2 and k + exclude_self <= R.CAP - 4
    if served is None:
        served = in_scope
    assert in_scope or not served, ix.debug_last_prefilter()
    if not served:
        assert rec["launched"] == 0 and st["rescued_rows"] == 0 and scan["rows"] == st["exact_fallbacks"], (rec, st, scan)
        return dist, idx, rec
    assert rec["launched"] == 1 and rec["ks"] == (ix.d + 15) // 16, rec
    assert rec["offered"] == st["exact_fallbacks"], (rec, st)
    assert rec["rescued"] == st["rescued_rows"] == rec["rescued_total"], (rec, st)
    # offered = not rescuable + overflowed + rescued + (rescuable, not overflowed, yet not certified by the rescue)
    rest = rec["handed_on"] - rec["not_rescuable"] - rec["overflowed"]
    assert rest >= 0 and rec["not_rescuable"] + rec["overflowed"] + rec["rescued"] + rest == rec["offered"], rec
    assert scan["rows"] == rec["handed_on"], (scan, rec)
    return dist, idx, rec


def _equal(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_thin_calls(N, O, handles, d, record_property):
    """k = 1, 5, 7, 10 on given rows, X=None with k = 4 and 9 (row_offset 1000 on the given rows), one call without the
    deterministic ordering."""
    ref, q = _problem(d)
    ix = handles(d)
    for k in (1, 5, 7, 10):
        got = _call(ix, q, k, served=d <= 32 or k > 1)  # (lists of 2 at three and four K-steps: the first-generation kernel)
        _equal(got, O.kneighbors(ref, q, k, "expanded", row_offset=ROW_OFFSET), f"d={d} k={k}")
        record_property(f"d={d} k={k}", str(got[2]))
    for k in (4, 9):
        got = _call(ix, None, k, nq=N_REF, served=True)
        _equal(got, O.kneighbors(ref, None, k, "expanded"), f"d={d} k={k} X=None")
        record_property(f"d={d} k={k} X=None", str(got[2]))
    got = _call(ix, q, 5, deterministic=False, served=True)
    _equal(got, O.kneighbors(ref, q, 5, "expanded", deterministic=False, row_offset=ROW_OFFSET), f"d={d} k=5 heap order")


@gpu
def test_bulk_and_thin_call(N, O, handles, record_property):
    ref, q = _problem(32, NQ_BULK)
    got = _call(handles(32), q, 5, served=True)
    _equal(got, O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET), "bulk + thin")
    record_property("bulk + thin", str(got[2]))


@gpu
def test_calls_outside_the_scope_keep_the_scan(N, O, handles):
    """More than 12 neighbours searched (the finish has 16 lanes per row) and a reference set of the first-generation
    kernel: no rescue, the scan consumes what the finalisers listed."""
    ref, q = _problem(32)
    got = _call(handles(32), q, 13, served=False)
    _equal(got, O.kneighbors(ref, q, 13, "expanded", row_offset=ROW_OFFSET), "k=13")
    ref, q = _problem(32, NQ_THIN, 3_000)
    ix = N.Index(ref)
    got = _call(ix, q, 5, served=False)
    _equal(got, O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET), "3,000 reference rows")
    ix.close()


def _mirror_problem(O, d, k, seed):
    """Law 1: for 256 chosen queries the reference row q + (1 + 2^-30)(q - a) behind the oracle's k-th neighbour a: the
    k-th and k+1-th distances differ by far less than the certificate's eps and are never equal.  Returns the reference
    rows, the queries, the chosen query rows and the oracle's k + 1 distances of the chosen rows on the final set."""
    ref, q = (a.copy() for a in _problem(d))
    rng = np.random.default_rng(seed)
    chosen = np.sort(rng.choice(np.arange(16, NQ_THIN), 256, replace=False))  # (not the copied queries)
    _, oi = O.kneighbors(ref, q[chosen], k, "expanded")
    a = ref[oi[:, k - 1]]
    ref = np.concatenate([ref, q[chosen] + (1.0 + 2.0 ** -30) * (q[chosen] - a)])
    od, _ = O.kneighbors(ref, q[chosen], k + 1, "expanded")
    return ref, q, chosen, od


def _rows_under_the_bound(ix, ref, rows, d_k, ks):
    """How many reference rows the rescue can collect for each query row, at most: a collected row has
    main < t_resc + margin; main >= corrected - margin and corrected >= s^2 d^2 - |q'|^2 - eps, so
    s^2 d^2 < t_resc + |q'|^2 + 2 margin + eps; t_resc is (tau + noise) s^2 + eps - |q'|^2 rounded up by two floats, and
    tau, the k-th re-scored distance of the finaliser's candidates, is within 2 eps / s^2 of the true k-th squared
    distance (its lists hold the k smallest corrected values).  Together, with noise far below eps:
        s^2 d^2 <= s^2 d_k^2 + 2 margin + 5 eps."""
    c = ix.debug_image_constants()
    s, mu = c["s"], c["mu"][:ref.shape[1]]
    rb = s * (ref - mu)
    ymax = np.sqrt((rb * rb).sum(axis=1).max())
    out = []
    for row, dk in zip(rows, d_k):
        qb = s * (row - mu)
        qn = (qb * qb).sum()
        eps = (12.0 + 2.0 * ks) * 2.0 ** -24 * (np.sqrt(qn) + ymax) ** 2
        margin = 2.0 ** -9 * 1.02 * ymax * np.sqrt(qn)
        d2 = ((ref - row) ** 2).sum(axis=1)
        out.append(np.count_nonzero(s * s * d2 <= s * s * dk * dk + 2.0 * margin + 5.0 * eps))
    return np.array(out)


@gpu
def test_law_mirror(N, O, record_property, monkeypatch):
    """Rows the rescue must answer.  The chosen queries are filtered on the CPU: no exact tie at the boundary, and no more
    than CAP reference rows under the rescue's bound (_rows_under_the_bound: at most 10 of them on this data).

    (A ball of 1.5 x the k-th distance, the first proposal for that filter, says nothing about the bound in 13 or more
    features: on these sets it holds 47 .. 155 rows at d = 13, 400 .. 890 at d = 32 and 1,800 .. 2,800 at d = 64, while the
    bound's own margin is 0.7 % of the k-th squared distance and covers 6 .. 10 rows.)"""
    d, k = 32, 5
    ref, q, chosen, od = _mirror_problem(O, d, k, seed=3)
    want = O.kneighbors(ref, q, k, "expanded", row_offset=ROW_OFFSET)
    ix = N.Index(ref)
    under = _rows_under_the_bound(ix, ref, q[chosen], od[:, k - 1], (d + 15) // 16)
    record_property("mirror: rows under the bound, most", int(under.max()))
    chosen = chosen[(od[:, k - 1] != od[:, k]) & (under <= R.CAP)]
    assert len(chosen) >= 200, f"{len(chosen)} chosen queries remain: change the seed"
    got = _call(ix, q, k, served=True)
    _equal(got, want, "mirror")
    record_property("mirror, whole call", str(got[2]))
    # the chosen rows alone: whatever of them the finaliser lists, the rescue answers
    sub = _call(ix, q[chosen], k, served=True)
    _equal(sub, O.kneighbors(ref, q[chosen], k, "expanded", row_offset=ROW_OFFSET), "mirror, chosen rows")
    record_property("mirror, chosen rows", str(sub[2]))
    assert sub[2]["offered"] >= 1, sub[2]
    assert sub[2]["handed_on"] == 0 and sub[2]["rescued"] == sub[2]["offered"], sub[2]
    ix.close()
    # the switch: today's path in the same library, identical outputs
    monkeypatch.setenv("SKNNR_RESCUE", "0")
    off = N.Index(ref)
    monkeypatch.delenv("SKNNR_RESCUE")
    got_off = _call(off, q, k, served=False)
    _equal(got_off, want, "mirror, SKNNR_RESCUE=0")
    off.close()


@gpu
def test_law_duplicates(N, O, record_property):
    """make_problem's 24 duplicated reference rows and 16 copied queries, and reference rows repeated twelve times beside
    600 queries (exact ties; more hits in one unit than a lane's queue holds: poisoned queries)."""
    ref, q = (a.copy() for a in _problem(32))
    ref[600:1200] = np.repeat(ref[:50], 12, axis=0)
    q[:600] = ref[600:1200] + 1e-9
    ix = N.Index(ref)
    for k in (1, 5):
        got = _call(ix, q, k)
        _equal(got, O.kneighbors(ref, q, k, "expanded", row_offset=ROW_OFFSET), f"duplicates k={k}")
        record_property(f"duplicates k={k}", str(got[2]))
        assert got[2]["offered"] > 0
    # the 600 rows beside twelve copies, k = 5 alone: every one has an exact tie across the boundary -- listed as tied (not
    # rescuable) or handed on by the rescue's own tie test, never rescued
    sub = _call(ix, q[:600], 5, served=True)
    _equal(sub, O.kneighbors(ref, q[:600], 5, "expanded", row_offset=ROW_OFFSET), "duplicates, tied rows")
    record_property("duplicates, tied rows", str(sub[2]))
    assert sub[2]["offered"] == 600 and sub[2]["rescued"] == 0 and sub[2]["handed_on"] == 600, sub[2]
    ix.close()


@gpu
def test_law_crowd(N, O, record_property):
    """40 distinct near-copies of one reference row (relative spacing 2^-20) with 64 queries beside them: more than CAP rows
    fall under the bound."""
    ref, q = (a.copy() for a in _problem(32))
    rng = np.random.default_rng(9)
    centre = ref[100].copy()
    ref[2000:2040] = centre * (1.0 + 2.0 ** -20 * np.arange(1, 41))[:, None]
    assert len(np.unique(ref[2000:2040], axis=0)) == 40
    q[1000:1064] = centre + 2.0 ** -20 * np.abs(centre) * rng.standard_normal((64, 32))
    near = [np.count_nonzero(np.sqrt(((ref - row) ** 2).sum(axis=1)) <= 2.0 ** -12 * np.linalg.norm(centre)) for row in q[1000:1064]]
    assert min(near) > R.CAP
    ix = N.Index(ref)
    got = _call(ix, q, 5, served=True)
    _equal(got, O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET), "crowd")
    record_property("crowd", str(got[2]))
    assert got[2]["overflowed"] > 0, got[2]
    ix.close()


@gpu
def test_law_not_rescuable(N, O, record_property):
    """Query rows whose image overflows f16 (|s (x - mu)| >= 32768): no |q'|^2, no threshold."""
    ref, q = (a.copy() for a in _problem(32))
    ix = N.Index(ref)
    s = ix.debug_image_constants()["s"]
    q[50:58] = ref[:8] + 40_000.0 / s
    got = _call(ix, q, 5, served=True)
    _equal(got, O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET), "image overflow")
    record_property("image overflow", str(got[2]))
    assert got[2]["not_rescuable"] >= 8, got[2]
    ix.close()


@gpu
def test_law_pooled_lists(N, O, handles, record_property):
    """k = 10 at d = 32 (lists of 8, rank + 4): the instance that hands 6 % of its rows to the scan at 4,500 rows.  The
    rescued share is recorded, not asserted."""
    ref, q = _problem(32)
    ix = handles(32)
    got = _call(ix, q, 10, served=True)
    pre = ix.debug_last_prefilter()
    assert (pre["generation"], pre["m_list"], pre["rank_extra"]) == (2, 8, 4), pre
    _equal(got, O.kneighbors(ref, q, 10, "expanded", row_offset=ROW_OFFSET), "pooled lists")
    record_property("pooled lists: rescued share of offered", got[2]["rescued"] / max(1, got[2]["offered"]))
    record_property("pooled lists", str(got[2]))
