"""Every coarse_kernel<KS, M> instance (coarse.hip.h, 40 of them), pinned launch by launch to its list contract.

The first-generation pre-filter is the only one for more than 64 features, for one neighbour at 33 .. 64 features and for
every reference set under about 3,600 rows.  It is a candidate generator: whatever it gets wrong, the certificate refuses
and the float64 scan repairs, so answers alone cannot see a dropped hit, a wrong sentinel count, a stale threshold or a
lost queue entry.  Here every call

- names the launch it expects (tests/_prefilter_dispatch.py) and asserts ``Index.debug_last_prefilter()`` reports it;
- compares indices and distances bit for bit with ``oracle.kneighbors`` (row_offset 1000);
- reads the two lists the kernel filed per query (``Index.debug_coarse_candidates``) and checks them against the matrix of
  ranking values of ``Index.debug_coarse_matrix`` clause by clause (tests/_coarse_lists.py, check_lists);
- asserts that ``stats()["exact_fallbacks"]`` EQUALS what finalize_core decides for lists that honour the contract
  (predicted_fallbacks, from the oracle's squared distances); rows the restatement cannot decide widen that to an
  interval and may be at most 1 % of a call (none occurs).  The share itself is recorded as a test property, not
  bounded.

Shapes: 1,300 reference rows (synth.make_problem, 12 duplicated reference rows, 8 queries that copy a reference row): 41
tiles, which is 6 stages at KS <= 2, 11 at KS 3 .. 4 and 21 at KS >= 5 (odd, the last stage half padding), and below
min_coarse2_n_ref at every KS.  6,145 query rows: two row quanta, the second almost all padding.  One width per KS
(13, 20, 40 and 72 pad their last K-step); kk takes both ends of every list length: no sentinel, and the most it gets.

COVERAGE lists all 40 (KS, M) with the (d, kk) cases of test_instance that launch each and the launch's wave count:

    KS 1 (d = 13):  M 2: kk 1 (16 waves)  M 6: kk 2, 5 (16)  M 8: kk 6, 7 (16)  M 16: kk 8, 15 (12)  M 32: kk 16, 31 (8)
    KS 2 (d = 20):  M 2: kk 1 (16)        M 6: kk 2, 5 (16)  M 8: kk 6, 7 (16)  M 16: kk 8, 15 (12)  M 32: kk 16, 31 (8)
    KS 3 (d = 40):  M 2: kk 1 (12)        M 6: kk 2, 5 (12)  M 8: kk 6, 7 (12)  M 16: kk 8, 15 (12)  M 32: kk 16, 31 (8)
    KS 4 (d = 64):  M 2: kk 1 (12)        M 6: kk 2, 5 (12)  M 8: kk 6, 7 (12)  M 16: kk 8, 15 (12)  M 32: kk 16, 31 (8)
    KS 5 (d = 72):  M 2: kk 1 (12)        M 6: kk 2, 5 (12)  M 8: kk 6, 7 (12)  M 16: kk 8, 15 (12)  M 32: kk 16, 31 (8)
    KS 6 (d = 96):  M 2: kk 1 (12)        M 6: kk 2, 5 (12)  M 8: kk 6, 7 (12)  M 16: kk 8, 15 (8)   M 32: kk 16, 31 (8)
    KS 7 (d = 112): M 2: kk 1 (12)        M 6: kk 2, 5 (12)  M 8: kk 6, 7 (8)   M 16: kk 8, 15 (8)   M 32: kk 16, 31 (8)
    KS 8 (d = 128): M 2: kk 1 (8)         M 6: kk 2, 5 (8)   M 8: kk 6, 7 (8)   M 16: kk 8, 15 (8)   M 32: kk 16, 31 (8)

test_self_queries repeats every kk >= 2 as X=None with k = kk - 1; test_without_deterministic_order runs one case per list
length; the edges (1 .. 129 reference rows, 6,144 rows) and three data laws follow.

Measured on an MI355X: every call's fall-back count equals the prediction, with no undetermined row; on the synthetic
law the shares are 0.46 - 1.99 % of the given rows and 0.46 - 2.38 % of the X=None rows, the largest at KS 6 with lists
of 32 (profiles/r15_coarse1_fallback_share.txt, the first measurement at KS 5 .. 8).

Teeth (scratch builds, never committed), of the 191 GPU tests of this module: with skip_scale = 0 in launch_coarse 36 fail
-- 27 on the lists (a row among the J smallest is missing: "J smallest" 27, one of them also "rows below B", two also
the fall-back count) while their answers still match, 9 on wrong neighbours; with n_sentinel off by one all 191 fail on
"sentinel prefix", 167 of them also on the fall-back count.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import _coarse_lists as C
import _prefilter_dispatch as P

N_REF = 1_300
NQ = 6_145
NQ_LAW = 1_024
ROW_OFFSET = 1_000
WIDTHS = (13, 20, 40, 64, 72, 96, 112, 128)
KKS = (1, 2, 5, 6, 7, 8, 15, 16, 31)
LAW_KKS = (1, 5, 7, 15, 31)
UNDETERMINED_MAX = 0.01  # share of a call's rows the restatement may leave undecided

# (KS, M): (d, kk of the test_instance cases that launch it, waves of the launch)
COVERAGE = {
    (1, 2): (13, (1,), 16),
    (1, 6): (13, (2, 5), 16),
    (1, 8): (13, (6, 7), 16),
    (1, 16): (13, (8, 15), 12),
    (1, 32): (13, (16, 31), 8),
    (2, 2): (20, (1,), 16),
    (2, 6): (20, (2, 5), 16),
    (2, 8): (20, (6, 7), 16),
    (2, 16): (20, (8, 15), 12),
    (2, 32): (20, (16, 31), 8),
    (3, 2): (40, (1,), 12),
    (3, 6): (40, (2, 5), 12),
    (3, 8): (40, (6, 7), 12),
    (3, 16): (40, (8, 15), 12),
    (3, 32): (40, (16, 31), 8),
    (4, 2): (64, (1,), 12),
    (4, 6): (64, (2, 5), 12),
    (4, 8): (64, (6, 7), 12),
    (4, 16): (64, (8, 15), 12),
    (4, 32): (64, (16, 31), 8),
    (5, 2): (72, (1,), 12),
    (5, 6): (72, (2, 5), 12),
    (5, 8): (72, (6, 7), 12),
    (5, 16): (72, (8, 15), 12),
    (5, 32): (72, (16, 31), 8),
    (6, 2): (96, (1,), 12),
    (6, 6): (96, (2, 5), 12),
    (6, 8): (96, (6, 7), 12),
    (6, 16): (96, (8, 15), 8),
    (6, 32): (96, (16, 31), 8),
    (7, 2): (112, (1,), 12),
    (7, 6): (112, (2, 5), 12),
    (7, 8): (112, (6, 7), 8),
    (7, 16): (112, (8, 15), 8),
    (7, 32): (112, (16, 31), 8),
    (8, 2): (128, (1,), 8),
    (8, 6): (128, (2, 5), 8),
    (8, 8): (128, (6, 7), 8),
    (8, 16): (128, (8, 15), 8),
    (8, 32): (128, (16, 31), 8),
}

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the table, and the restatement alone on the chosen inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_coverage_table_matches_dispatch():
    """All 40 instances, each launched by the cases the table names at the waves it names: generation 1, two row quanta."""
    assert sorted(COVERAGE) == [(ks, m) for ks in range(1, 9) for m in C.LIST_LENGTHS]
    covered = {}
    for d in WIDTHS:
        for kk in KKS:
            rec = P.expected_launch(N_REF, d, kk, NQ)
            assert (rec["generation"], rec["rank_extra"], rec["thin_rows"], rec["cell_depth"]) == (1, 0, 0, 0), (d, kk)
            assert rec["bulk_rows"] == 12_288 and rec["bulk_waves"] == P.coarse1_waves(rec["ks"], rec["m_list"])
            assert kk + 1 <= rec["m_list"]
            covered.setdefault((rec["ks"], rec["m_list"]), (d, [], rec["bulk_waves"]))[1].append(kk)
    assert {key: (d, tuple(kks), w) for key, (d, kks, w) in covered.items()} == COVERAGE
    assert all(N_REF < P.min_coarse2_n_ref(ks) for ks in range(1, 5))
    # both ends of every list length: no sentinel, and the most a list of that length gets
    assert {P.coarse_list_len_plain(kk) - (kk + 1) for kk in KKS} == {0, 3, 1, 7, 15}
    tiles = (N_REF + 31) // 32
    assert tiles == 41 and [-(-tiles // tps) for tps in (8, 4, 2)] == [6, 11, 21]


def _host_image(ref, q):
    """The pre-filter's ranking values and |q'|^2 in float64 arithmetic, rounded to float32: what an ideal pre-filter
    ranks (the index build's mu and power-of-two scale, sknnr_index_create)."""
    mu = ref.mean(axis=0)
    amax = np.abs(ref - mu).max()
    s = 2.0 ** (7 - np.frexp(amax)[1])
    rb, qb = s * (ref - mu), s * (q - mu)
    v = (rb * rb).sum(axis=1)[None] - 2.0 * qb @ rb.T
    return v.astype(np.float32), (qb * qb).sum(axis=1), C.image_constants(ref, mu, s)


@pytest.mark.parametrize("d", WIDTHS)
def test_restatement_decides_the_chosen_inputs(d):
    """Before any device run: on all 6,145 queries and as a self query, with an ideal pre-filter's values, predicted_fallbacks
    leaves at most 1 % of the rows undecided at every kk, under both tie rules (it leaves none)."""
    from oracle import oracle as O

    x_ref, x_q = _problem(d)
    for q in (x_q, x_ref):
        v, qn, consts = _host_image(x_ref, q)
        for kk in KKS:
            d2, idx = _sorted_d2(O, q, x_ref, kk)
            for deterministic in (True, False):
                _, und = C.predicted_fallbacks(v, d2, idx, qn, consts, kk, deterministic=deterministic)
                assert und.sum() <= UNDETERMINED_MAX * len(q), (d, kk, deterministic, int(und.sum()))


def test_law_layouts():
    """The data laws' layouts (no GPU): the crowded half holds its 48 rows on positions of one lane half, three per tile."""
    for h in (0, 1):
        rows = _crowded_rows(h)
        assert len(rows) == 48 and ((rows % 8 >= 4) == bool(h)).all() and np.bincount(rows // 32).max() == 3
    ref, _ = _duplicates_problem(20)
    assert len(np.unique(ref, axis=0)) == 33 and (ref[:40] == ref[0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# shared state: one handle per data set, matrices and oracle results cached
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
def sets(N):
    """sets(key, ref, **env): the handle of a data set (created once, with the environment given: all of it is read at index
    creation), with its image constants and caches of ranking-value matrices and oracle results by query set."""
    made = {}

    def get(key, ref, **env):
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                for name, value in env.items():
                    mp.setenv(name, str(value))
                ix = N.Index(ref)
            c = ix.debug_image_constants()
            made[key] = dict(ix=ix, ref=ref, consts=C.image_constants(ref, c["mu"], c["s"]), matrices={}, oracle={},
                             plain_order=str(env.get("SKNNR_IMAGE_ORDER")) == "0")
        return made[key]

    yield get
    for entry in made.values():
        entry["ix"].close()


def _matrix(entry, name, q):
    """(V, qn) of the query rows ``q`` (None: the reference rows), in caller row order, cached under ``name``."""
    if name not in entry["matrices"]:
        rows = entry["ref"] if q is None else q
        assert rows.shape[0] * entry["ref"].shape[0] <= 1 << 24
        v, qn, s, eps_c = entry["ix"].debug_coarse_matrix(rows)
        assert s == entry["consts"]["s"] and eps_c == (11 + 6 * entry["consts"]["ks"]) * 2.0 ** -24
        entry["matrices"][name] = (v, qn)
    return entry["matrices"][name]


@functools.lru_cache(maxsize=2)
def _problem(d):
    from sknnr_amd import synth

    x_ref, _, x_q = synth.make_problem(N_REF, NQ, d, t=1, n_dup_refs=12, n_dup_queries=8)
    return x_ref, x_q


def _sorted_d2(O, q, ref, kk):
    """Each query's min(kk + 1, n_ref) smallest squared distances in the reference's arithmetic, ascending, and their rows."""
    d2, idx = O.argkmin(q, ref, min(kk + 1, len(ref)), "expanded", squared=True)
    order = np.argsort(d2, axis=1, kind="stable")
    return np.take_along_axis(d2, order, axis=1), np.take_along_axis(idx, order, axis=1)


def _oracle(O, entry, name, q, kk, deterministic):
    """The oracle's answer and its sorted squared distances for the query set ``name`` of a data set, computed once."""
    key = (name, kk, deterministic)
    if key not in entry["oracle"]:
        ref, self_rows = entry["ref"], q is None
        want = O.kneighbors(ref, q, kk - 1 if self_rows else kk, "expanded", deterministic=deterministic,
                            row_offset=0 if self_rows else ROW_OFFSET)
        entry["oracle"][key] = (want, _sorted_d2(O, ref if self_rows else q, ref, kk))
    return entry["oracle"][key]


def _run(O, entry, name, q, kk, record, what, deterministic=True, expect_rows=None):
    """One call, checked four ways (module docstring).  ``q`` None: X=None with k = kk - 1.  Returns the call's fall-backs
    and the mask of rows whose image is finite."""
    ix, ref = entry["ix"], entry["ref"]
    self_rows = q is None
    rows = ref if self_rows else q
    n, k = len(rows), kk - 1 if self_rows else kk
    v, qn = _matrix(entry, name, q)
    d = ref.shape[1]
    ix.reset_stats()
    opts = ix.make_opts(k, exclude_self=self_rows, row_offset=0 if self_rows else ROW_OFFSET, deterministic=deterministic)
    dist, idx = ix.kneighbors_host(q, opts, nq=n if self_rows else None)
    st = ix.stats()
    rec = ix.debug_last_prefilter()
    val, pos, perm = ix.debug_coarse_candidates(n)
    assert st["queries"] == n and st["exact_only_queries"] == 0 and st["coarse_queries"] == n, st
    expect = P.expected_launch(len(ref), d, kk, n)
    assert expect["generation"] == 1 and rec == expect, f"{what}: launched {rec}, dispatch says {expect}"
    if expect_rows is not None:
        assert rec["bulk_rows"] == expect_rows

    want, (d2, near) = _oracle(O, entry, name, q, kk, deterministic)
    np.testing.assert_array_equal(idx, want[1], err_msg=what)
    np.testing.assert_array_equal(dist, want[0], err_msg=what)

    finite = np.isfinite(qn)
    m = rec["m_list"]
    assert sorted(perm.tolist()) == list(range(len(ref))), what
    if entry["plain_order"]:
        assert (perm == np.arange(len(ref))).all(), f"{what}: image position is not the row index"
    broken = C.list_violations(val, pos, perm, v, kk, m, rows=finite)

    fallback, und = C.predicted_fallbacks(v, d2, near, qn, entry["consts"], kk, deterministic=deterministic)
    assert und.sum() <= UNDETERMINED_MAX * n, f"{what}: {int(und.sum())} of {n} rows undetermined"
    lo = int((fallback & ~und).sum())
    got = int(st["exact_fallbacks"])
    record(f"fallback {what}".strip(), round(got / n, 6))
    # (both verdicts in one message: lists that break the contract usually move the count too)
    late = [f"{name}: {cnt} queries, first {q}" for name, cnt, q in broken]
    if not lo <= got <= lo + int(und.sum()):
        late.append(f"{got} rows fell back, the contract predicts {lo} (+ {int(und.sum())} undetermined)")
    assert not late, f"{what}: " + "; ".join(late)
    return got, finite


# ---------------------------------------------------------------------------------------------------------------------
# the instance matrix
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kk", KKS)
@pytest.mark.parametrize("d", WIDTHS)
def test_instance(N, O, sets, record_property, d, kk):
    """One (KS, kk) case of COVERAGE: 6,145 rows."""
    x_ref, x_q = _problem(d)
    _run(O, sets(("synth", d), x_ref), "queries", x_q, kk, record_property, "given rows", expect_rows=12_288)


@gpu
@pytest.mark.parametrize("kk", [kk for kk in KKS if kk >= 2])
@pytest.mark.parametrize("d", WIDTHS)
def test_self_queries(N, O, sets, record_property, d, kk):
    """X=None: the reference rows query themselves with k = kk - 1 (kk neighbours searched)."""
    x_ref, _ = _problem(d)
    _run(O, sets(("synth", d), x_ref), "self", None, kk, record_property, "self")


@gpu
@pytest.mark.parametrize("d, kk", [(13, 1), (40, 5), (72, 7), (96, 15), (128, 31)])
def test_without_deterministic_order(N, O, sets, record_property, d, kk):
    """deterministic=False, one case per list length: any exact tie among the kept rows goes to the scan."""
    x_ref, x_q = _problem(d)
    _run(O, sets(("synth", d), x_ref), "queries", x_q, kk, record_property, "engine order", deterministic=False)


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_ref", [1, 5, 31, 33, 64, 65, 129])
def test_small_reference_sets(N, O, sets, record_property, n_ref):
    """d = 72 (two tiles per stage): a single stage, fewer rows than the list asks for (1 row at kk 1, 5 at kk 5, 31 at
    kk 31), one live tile; 65 rows put one row in the second stage, 129 make three stages with the last half padding."""
    d = 72
    x_ref, x_q = _problem(d)
    entry = sets(("small", n_ref), np.ascontiguousarray(x_ref[:n_ref]))
    assert P.ks_of(d) == 5 and -(-((n_ref + 31) // 32) // 2) == {1: 1, 5: 1, 31: 1, 33: 1, 64: 1, 65: 2, 129: 3}[n_ref]
    for kk in [kk for kk in LAW_KKS if kk <= n_ref]:
        _run(O, entry, "queries", x_q[:NQ_LAW], kk, record_property, f"n_ref {n_ref}, kk {kk}")


@gpu
@pytest.mark.parametrize("d, kk", [(13, 5), (72, 7)])
def test_one_row_quantum(N, O, sets, record_property, d, kk):
    """6,144 rows: one row quantum, no padding row (test_instance runs 6,145: two quanta)."""
    x_ref, x_q = _problem(d)
    _run(O, sets(("synth", d), x_ref), "one quantum", x_q[:6_144], kk, record_property, "6,144 rows", expect_rows=6_144)


@gpu
def test_image_overflow(N, O, sets, record_property):
    """Queries whose image overflows f16 (every 7th row x 1e7): exempt from the list contract, answered exactly, and every
    one of them counted as a fall-back."""
    d, kk = 40, 5
    x_ref, x_q = _problem(d)
    q = x_q[:NQ_LAW].copy()
    q[::7] *= 1e7
    got, finite = _run(O, sets(("synth", d), x_ref), "overflow", q, kk, record_property, "overflow")
    assert (~finite).sum() == len(q[::7]) and got >= (~finite).sum()


# ---------------------------------------------------------------------------------------------------------------------
# data laws, all with SKNNR_IMAGE_ORDER=0: image position = row index
# ---------------------------------------------------------------------------------------------------------------------
def _descending_problem(d):
    """Reference rows sorted by decreasing distance from a tight query cluster: almost every tile brings rows nearer than
    everything before it, so the queue overflows and direct insertion runs."""
    rng = np.random.default_rng([53, d])
    x = rng.standard_normal((N_REF, d))
    centre = 0.5 * rng.standard_normal(d)
    x = x[np.argsort(-((x - centre) ** 2).sum(axis=1))]
    return x, centre + 0.01 * rng.standard_normal((NQ_LAW, d))


def _crowded_rows(h):
    """48 positions of lane half h, three in each of 16 tiles spread over the image."""
    slots = [p for p in range(32) if (p % 8 >= 4) == bool(h)]
    return np.array([32 * (2 * t + 3) + slots[(3 * t + j) % 16] for t in range(16) for j in range(3)])


def _crowded_problem(d, h):
    """Each query's 32 nearest rows on positions of one lane half only (half 0 carries the sentinels)."""
    rng = np.random.default_rng([59, d, h])
    x = rng.standard_normal((N_REF, d))
    centre = rng.standard_normal(d)
    rows = _crowded_rows(h)
    x[rows] = centre + 0.05 * rng.standard_normal((len(rows), d))
    return x, centre + 0.02 * rng.standard_normal((NQ_LAW, d))


def _duplicates_problem(d):
    """Blocks of 40 exact duplicates: ties at B and inside the lists."""
    rng = np.random.default_rng([61, d])
    base = rng.standard_normal((33, d))
    return np.ascontiguousarray(base[np.arange(N_REF) // 40]), rng.standard_normal((NQ_LAW, d))


@gpu
@pytest.mark.parametrize("kk", LAW_KKS)
@pytest.mark.parametrize("d", [20, 96])
def test_law_descending(N, O, sets, record_property, d, kk):
    x_ref, x_q = _descending_problem(d)
    # the law: for every query, at least nine tiles in ten hold a row nearer than every row before them
    d2 = ((x_q[:64, None, :] - x_ref[None]) ** 2).sum(axis=2)
    pad = np.full((64, 42 * 32 - N_REF), np.inf)
    tile_min = np.concatenate([d2, pad], axis=1).reshape(64, 42, 32).min(axis=2)[:, :41]
    assert ((tile_min[:, 1:] < np.minimum.accumulate(tile_min, axis=1)[:, :-1]).mean(axis=1) >= 0.9).all(), "the law does not hold"
    _, oi = O.kneighbors(x_ref, x_q, kk, "expanded")
    assert oi.min() >= N_REF - 160, "the law does not hold"
    _run(O, sets(("descending", d), x_ref, SKNNR_IMAGE_ORDER=0), "queries", x_q, kk, record_property, "descending")


@gpu
@pytest.mark.parametrize("kk", LAW_KKS)
@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("d", [20, 96])
def test_law_crowded_half(N, O, sets, record_property, d, h, kk):
    x_ref, x_q = _crowded_problem(d, h)
    _, oi = O.kneighbors(x_ref, x_q, 32, "expanded")
    assert ((oi % 8 >= 4) == bool(h)).all() and np.isin(oi, _crowded_rows(h)).all(), "the law does not hold"
    entry = sets(("crowded", d, h), x_ref, SKNNR_IMAGE_ORDER=0)
    _run(O, entry, "queries", x_q, kk, record_property, f"crowded half {h}")


@gpu
@pytest.mark.parametrize("kk", LAW_KKS)
@pytest.mark.parametrize("d", [20, 96])
def test_law_duplicate_blocks(N, O, sets, record_property, d, kk):
    x_ref, x_q = _duplicates_problem(d)
    od, oi = O.kneighbors(x_ref, x_q, kk, "expanded")
    assert (od[:, 0] == od[:, min(kk, 20) - 1]).all(), "the law does not hold"
    _run(O, sets(("duplicates", d), x_ref, SKNNR_IMAGE_ORDER=0), "queries", x_q, kk, record_property, "duplicate blocks")
