"""The host restatement of the first-generation list contract (tests/_coarse_lists.py) against references of its own (no
GPU): a plain replay of the sweep must pass ``check_lists`` on random and adversarial value matrices at every list length
and every J, three mutated replays must fail it, and ``predicted_fallbacks`` must decide as exact rational arithmetic,
rounded once per operation, decides."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest

import _coarse_lists as C
import _rescue as R


def _matrices(rng, m):
    """(name, V) value matrices in image order (perm = identity), float32."""
    n_pos = 32 * 7 + 19
    yield "random", rng.standard_normal((8, n_pos)).astype(np.float32)
    # descending: every tile brings hits, the queue overflows and direct insertion runs
    yield "descending", (np.arange(n_pos, 0, -1, dtype=np.float32)[None] + rng.random((4, 1)).astype(np.float32))
    yield "all equal", np.full((3, n_pos), 2.5, dtype=np.float32)
    # ties at the boundary: few distinct values, many copies of each
    yield "ties", rng.integers(0, 5, (8, n_pos)).astype(np.float32)
    # more hits per tile than the queue takes, on one lane half only (half 0 carries the sentinels)
    for h in (0, 1):
        v = rng.standard_normal((4, n_pos)).astype(np.float32) + 100.0
        on = np.flatnonzero((np.arange(n_pos) % 8 >= 4) == bool(h))
        v[:, on[: 2 * m + 8]] = -np.arange(2 * m + 8, dtype=np.float32)[None]
        yield f"crowded half {h}", v
    yield "ascending", np.arange(n_pos, dtype=np.float32)[None].repeat(2, axis=0)


@pytest.mark.parametrize("m", C.LIST_LENGTHS)
def test_replay_honours_the_contract(m):
    """Every list length with every J = 2 .. M (every sentinel count 0 .. M - 2), margin 0 and a wide one."""
    rng = np.random.default_rng([7, m])
    perm = None
    for name, v in _matrices(rng, m):
        perm = np.arange(v.shape[1], dtype=np.int32)
        for kk in range(1, m):
            for margin in (0.0, 0.75):
                val, pos = C.replay(v, kk, m, margin=margin)
                C.check_lists(val, pos, perm, v, kk, m)


@pytest.mark.parametrize("m", C.LIST_LENGTHS)
def test_fewer_rows_than_the_list_holds(m):
    """n_ref < J: every row is listed and the rest stays empty; a permuted image."""
    rng = np.random.default_rng([11, m])
    for n_ref in sorted({1, 2, m - 1, m}):
        v_img = rng.standard_normal((5, n_ref)).astype(np.float32)
        perm = rng.permutation(n_ref).astype(np.int32)
        v = np.empty_like(v_img)
        v[:, perm] = v_img
        for kk in {1, m - 1}:
            val, pos = C.replay(v_img, kk, m)
            C.check_lists(val, pos, perm, v, kk, m)
            if n_ref < kk + 1:
                assert ((pos >= 0).sum(axis=(1, 2)) == n_ref).all()


def _stale_thr_case(m):
    """One lane (half 1) sees, inside one tile: queue_cap large values (queued), the M smallest (inserted directly, the list
    is full and thr must drop to its last entry), then a value between the list's last entry and the stale threshold."""
    assert m <= 8  # 16 registers per lane and tile
    regs = [100.0 + i for i in range(C.queue_cap(m))] + [float(i + 1) for i in range(m)] + [50.0]
    v = np.full((1, 64), 1000.0, dtype=np.float32)
    for r, x in enumerate(regs):
        v[0, C.acc_row(r, 1)] = x
    return v


def test_mutated_replays_fail():
    """One sentinel too many, thr not tightened on direct insertion, a dropped queue entry: check_lists names each."""
    rng = np.random.default_rng(13)
    m, kk = 6, 3
    v = rng.standard_normal((8, 200)).astype(np.float32)
    perm = np.arange(200, dtype=np.int32)
    C.check_lists(*C.replay(v, kk, m), perm, v, kk, m)
    names = {name for name, _, _ in C.list_violations(*C.replay(v, kk, m, mutation="sentinel"), perm, v, kk, m)}
    assert {"sentinel prefix", "unused slots"} <= names, names

    for m in (2, 6, 8):
        kk = m - 1
        v = _stale_thr_case(m)
        perm = np.arange(64, dtype=np.int32)
        C.check_lists(*C.replay(v, kk, m), perm, v, kk, m)
        names = {name for name, _, _ in C.list_violations(*C.replay(v, kk, m, mutation="stale_thr"), perm, v, kk, m)}
        assert names & {"rows below B", "J smallest"}, (m, names)

    for m in C.LIST_LENGTHS:
        kk = m - 1
        # every value of the first tile is a hit (thr starts at FLT_MAX): a lane's queue_cap-th register fills its queue,
        # and that is where each lane's nearest row sits
        v = rng.standard_normal((2, 96)).astype(np.float32)
        v[:, [C.acc_row(C.queue_cap(m) - 1, h) for h in (0, 1)]] = (-1000.0, -1001.0)
        perm = np.arange(96, dtype=np.int32)
        C.check_lists(*C.replay(v, kk, m), perm, v, kk, m)
        names = {name for name, _, _ in C.list_violations(*C.replay(v, kk, m, mutation="drop_queued"), perm, v, kk, m)}
        assert "rows below B" in names, (m, names)


def test_check_lists_names_each_clause():
    """Hand-made breaches of the other clauses: wrong half, a position twice, a value off by one bit, a position beyond
    the image, a descending pair."""
    rng = np.random.default_rng(17)
    m, kk = 6, 5
    v = rng.standard_normal((4, 100)).astype(np.float32)
    perm = rng.permutation(100).astype(np.int32)
    val, pos = C.replay(v[:, perm], kk, m)
    C.check_lists(val, pos, perm, v, kk, m)

    def names(val, pos):
        return {name for name, _, _ in C.list_violations(val, pos, perm, v, kk, m)}

    p = pos.copy(); p[0, 0, 0] ^= 4
    assert "own half" in names(val, p)
    p = pos.copy(); p[1, 1, 1] = p[1, 1, 0]
    assert "no position twice" in names(val, p)
    w = val.copy(); w[2, 1, 0] = np.nextafter(w[2, 1, 0], np.float32(-np.inf))
    assert "value bits" in names(w, pos)
    p = pos.copy(); p[3, 1, 0] = 100 + 4
    assert "position range" in names(val, p)
    w, p = val.copy(), pos.copy()
    w[0, 1, [0, 1]] = w[0, 1, [1, 0]]; p[0, 1, [0, 1]] = p[0, 1, [1, 0]]
    assert "ascending" in names(w, p)
    # queries left out by the mask are not looked at
    w = val.copy(); w[2] = np.nan
    C.check_lists(w, pos, perm, v, kk, m, rows=np.arange(4) != 2)


# ---------------------------------------------------------------------------------------------------------------------
# predicted_fallbacks against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _rnd(x: Fraction) -> Fraction:
    """One float64 rounding (Fraction -> float is correctly rounded)."""
    return Fraction(float(x))


def _sqrt_rnd(x: Fraction) -> Fraction:
    """Correctly rounded float64 square root of a float64 value, checked against its two neighbours exactly."""
    r = math.sqrt(float(x))
    lo, hi = Fraction(math.nextafter(r, 0.0)), Fraction(math.nextafter(r, math.inf))
    f = Fraction(r)
    assert ((lo + f) / 2) ** 2 <= x <= ((f + hi) / 2) ** 2
    return f


def _certified_rational(qn, b, tau, c):
    """finalize_core's inequality, every operation exact and then rounded once, as the kernel is compiled."""
    qn, b, tau = Fraction(float(qn)), Fraction(float(b)), Fraction(float(tau))
    s, ymax, mu2 = Fraction(c["s"]), Fraction(c["ymax"]), Fraction(c["mu2"])
    nrm = _rnd(_sqrt_rnd(qn) + ymax)
    eps_c = _rnd(Fraction(11 + 6 * c["ks"]) * Fraction(1, 2 ** 24))
    eps = _rnd(_rnd(eps_c * nrm) * nrm)
    inv_s = _rnd(1 / s)
    nr = _rnd(_rnd(nrm * inv_s) + mu2)
    noise_a = _rnd(Fraction(c["d"] + 4) * Fraction(1, 2 ** 53))
    noise = _rnd(_rnd(noise_a * nr) * nr)
    inv_s2 = _rnd(1 / _rnd(s * s))
    bound = _rnd(_rnd(_rnd(_rnd(qn + b) - eps) * inv_s2) - noise)
    return bound > tau


def test_predicted_fallbacks_against_rational_arithmetic():
    """Rows whose kk-th distance sits within a few float64 steps of the certificate's bound, either side, and rows far from
    it: the numpy restatement decides as the rational one does.  Then the tie rules and the reference sets smaller than
    kk."""
    rng = np.random.default_rng(19)
    d, kk, n_ref = 40, 3, 12
    c = dict(s=0.25, ymax=37.3, mu2=5.1, d=d, ks=3)
    n = 60
    v = np.sort(rng.uniform(-300.0, -100.0, (n, n_ref)).astype(np.float32), axis=1)
    qn = rng.uniform(400.0, 900.0, n)
    b = v[:, kk].astype(np.float64)
    eps, noise = R.certificate_terms(qn, c["ymax"], c["s"], d, c["ks"], c["mu2"], generation=1)
    edge = R.bound(qn, b, eps, noise, 1.0 / (c["s"] * c["s"]))
    steps = rng.integers(-3, 4, n)
    tau = np.array([e if k == 0 else _step(e, k) for e, k in zip(edge, steps)])
    tau[40:] = edge[40:] * rng.uniform(0.5, 1.5, n - 40)
    d2 = np.stack([tau * f for f in (0.25, 0.5, 1.0, 2.0)], axis=1)  # ascending, kk-th = tau, no ties
    idx = np.tile(np.arange(kk + 1), (n, 1))
    got, und = C.predicted_fallbacks(v, d2, idx, qn, c, kk)
    want = np.array([not _certified_rational(qn[i], b[i], tau[i], c) for i in range(n)])
    assert (got == want).all() and 5 < want.sum() < n - 5
    assert not und[want].any()

    # tie rules, on rows that the bound certifies comfortably
    sure = np.flatnonzero(~want & (tau < 0.9 * edge))[:4]
    assert len(sure) == 4
    vv, qq = v[sure], qn[sure]
    dd = d2[sure].copy()
    dd[0, kk] = dd[0, kk - 1]            # across the boundary
    dd[1, 0] = dd[1, 1]                  # among the kept rows
    f_det, _ = C.predicted_fallbacks(vv, dd, idx[sure], qq, c, kk, deterministic=True)
    f_any, _ = C.predicted_fallbacks(vv, dd, idx[sure], qq, c, kk, deterministic=False)
    assert f_det.tolist() == [True, False, False, False] and f_any.tolist() == [True, True, False, False]
    # a needed row that is not below B: the restatement cannot decide
    far = idx[sure].copy()
    far[2, 0] = n_ref - 1
    _, und = C.predicted_fallbacks(vv, d2[sure], far, qq, c, kk)
    assert und.tolist() == [False, False, True, False]
    # image overflow (qn = +inf), and fewer reference rows than neighbours searched
    f, u = C.predicted_fallbacks(vv, d2[sure], idx[sure], np.full(4, np.inf), c, kk)
    assert f.all() and not u.any()
    f, u = C.predicted_fallbacks(vv[:, :2], d2[sure][:, :2], idx[sure][:, :2], qq, c, kk)
    assert f.all() and not u.any()
    # exactly kk reference rows: B is FLT_MAX, the bound certifies
    f, u = C.predicted_fallbacks(vv[:, :kk], d2[sure][:, :kk], idx[sure][:, :kk], qq, c, kk)
    assert not f.any() and not u.any()


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def test_image_constants_sum_in_column_order():
    """ymax and mu2 as the index build sums them: one rounding per column, against the rational sums."""
    rng = np.random.default_rng(23)
    ref = rng.standard_normal((9, 5)) * 3.0 + 1.0
    mu = ref.mean(axis=0)
    c = C.image_constants(ref, mu, 0.5)
    best = Fraction(0)
    for row in ref:
        yn = Fraction(0)
        for x, m_ in zip(row, mu):
            b = _rnd(Fraction(0.5) * _rnd(Fraction(float(x)) - Fraction(float(m_))))
            yn = _rnd(yn + _rnd(b * b))
        best = max(best, yn)
    assert Fraction(c["ymax"]) == _sqrt_rnd(best)
    m2 = Fraction(0)
    for m_ in mu:
        m2 = _rnd(m2 + _rnd(Fraction(float(m_)) ** 2))
    assert Fraction(c["mu2"]) == _rnd(2 * _rnd(_sqrt_rnd(m2) * Fraction(1.0 + 1e-12)))
    assert (c["d"], c["ks"]) == (5, 1)
