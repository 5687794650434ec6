"""The rescue threshold t_resc (sknnr_amd/csrc/exact.hip.h, rescue_threshold) restated in numpy (tests/_rescue.py): over
the ranges the instance tests produce it satisfies the certificate's inequality as coded, and it is tight -- at most two
floats above the float64 solution, below which the inequality fails up to the rounding of its own float64 operations."""

from __future__ import annotations

import numpy as np

import _rescue as R

WIDTHS = ((13, 1), (32, 2), (41, 3), (64, 4))  # (features, K-steps)


def _draws(n=4000, seed=11):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        d, ks = WIDTHS[rng.integers(len(WIDTHS))]
        s = 2.0 ** rng.integers(-6, 11)
        ymax = 10.0 ** rng.uniform(0.0, 3.3)  # |s (r - mu)| of the farthest reference row
        qn = (rng.uniform(0.1, 1.5) * ymax) ** 2
        mu2 = rng.uniform(0.0, 100.0) / s  # 2 |mu| in unscaled units (0: the direct formula)
        if rng.random() < 0.3:
            mu2 = 0.0
        d2_scaled = 10.0 ** rng.uniform(-6.0, 0.6) * ymax * ymax  # the kk-th re-scored distance, in image units
        yield d, ks, s, ymax, qn, mu2, d2_scaled / (s * s)


def test_threshold_satisfies_the_certificate_and_is_tight():
    n, n_nan = 0, 0
    for d, ks, s, ymax, qn, mu2, tau in _draws():
        s2, inv_s2 = np.float64(s * s), np.float64(1.0) / np.float64(s * s)
        eps, noise = R.certificate_terms(qn, ymax, s, d, ks, mu2)
        t, t0 = R.rescue_threshold(qn, tau, eps, noise, s2, inv_s2)
        n += 1
        if np.isnan(t):
            n_nan += 1
            continue
        assert t.dtype == np.float32
        # the inequality as coded, with t_resc in the place of t_min
        assert R.bound(qn, t, eps, noise, inv_s2) > tau, (qn, tau, t)
        # rounded up, plus one float of safety: the second float below is at or under the float64 solution ...
        below = np.nextafter(np.nextafter(t, -R.F32_INF), -R.F32_INF)
        assert np.float64(below) <= t0 < np.float64(np.nextafter(t, -R.F32_INF)), (t, t0)
        # ... where the inequality can hold only by the rounding of its float64 operations: each of the eight operations
        # (four here, four in t0) is off by at most 2^-53 of the largest magnitude in play, scaled by 1 / s^2
        big = max(abs(qn), abs(np.float64(t)), eps, (tau + noise) * s2)
        assert R.bound(qn, below, eps, noise, inv_s2) - tau <= 16 * 2.0 ** -53 * big * inv_s2, (qn, tau, t)
    # no float satisfies the inequality only where t_resc cancels against |q'|^2: (d2 ~ |q'|^2 to 2^-29) is not drawn often
    assert n_nan <= n // 100, (n_nan, n)


def test_rows_without_a_bound_are_not_rescuable():
    eps, noise = R.certificate_terms(100.0, 30.0, 4.0, 32, 2, 1.0)
    for qn, tau in ((100.0, np.inf), (np.inf, 1.0), (np.nan, 1.0), (100.0, np.nan)):
        t, _ = R.rescue_threshold(qn, tau, eps, noise, np.float64(16.0), np.float64(1.0 / 16.0))
        assert np.isnan(t), (qn, tau, t)
    # (a finite case next to them)
    t, _ = R.rescue_threshold(100.0, 3.0, eps, noise, np.float64(16.0), np.float64(1.0 / 16.0))
    assert np.isfinite(t) and R.bound(100.0, t, eps, noise, np.float64(1.0 / 16.0)) > 3.0
