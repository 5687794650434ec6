"""Host restatement of the rescue threshold (sknnr_amd/csrc/exact.hip.h, rescue_threshold) and of the certificate it is
solved from (finalize_core), in numpy float32 / float64 -- every operation rounded once, as the kernel is compiled
(-ffp-contract=off)."""

from __future__ import annotations

import numpy as np

CAP = 16  # kRescueCap: candidates per listed row (sknnr_amd/csrc/rescue.hip.h)
F32_INF = np.float32(np.inf)


def eps_units(ks, generation=2):
    """The certificate's error budget in units of 2^-24 (sknnr_hip.hip: eps_units, first generation; eps_units2, second)."""
    return 11.0 + 6.0 * ks if generation == 1 else 12.0 + 2.0 * ks


def certificate_terms(qn, ymax, s, d, ks, mu2, generation=2):
    """eps and noise of finalize_core for a query with |q'|^2 = qn (scalars or arrays): eps_c = eps_units 2^-24, by default
    the second generation's (12 + 2 ks)."""
    qn, ymax, s, mu2 = (np.float64(v) for v in (qn, ymax, s, mu2))
    nrm = np.sqrt(qn) + ymax
    eps = np.float64(eps_units(ks, generation) * 2.0 ** -24) * nrm * nrm
    nr = nrm * (np.float64(1.0) / s) + mu2
    noise = np.float64((d + 4) * 2.0 ** -53) * nr * nr
    return eps, noise


def bound(qn, t, eps, noise, inv_s2):
    """The certificate's left-hand side as coded: (qn + t_min - eps) * inv_s2 - noise."""
    return (np.float64(qn) + np.float64(t) - eps) * inv_s2 - noise


def rescue_threshold(qn, tau, eps, noise, s2, inv_s2):
    """(t_resc, t0): the float the kernel files (NaN: not rescuable) and the float64 solution it was rounded up from."""
    with np.errstate(all="ignore"):
        t0 = ((np.float64(tau) + noise) * s2 + eps) - np.float64(qn)
        t = np.float32(t0)
        if not np.float64(t) > t0:
            t = np.nextafter(t, F32_INF)
        t = np.nextafter(t, F32_INF)
        ok = bound(qn, t, eps, noise, inv_s2) > tau
    return (t if ok and t < F32_INF and qn < np.inf and tau < np.inf else np.float32(np.nan)), t0
