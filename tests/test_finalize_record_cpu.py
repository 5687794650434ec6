"""The merged candidate record (tests/_finalize_record.py restates coarse2_kernel's epilogue) against a brute-force sort,
and the claim the finaliser rests on: whenever the truncation rule does not fire, the record yields the same re-score
window and the same candidates inside it as the two full lists."""

from __future__ import annotations

import numpy as np
import pytest

import _finalize_record as R

FLT_MAX = np.finfo(np.float32).max
N_REF = 1000


def _lists(rng, m, kk, ties, sentinels, padding):
    """Two ascending lists as the pre-filter leaves them: list 0 starts with m - (kk + 1) sentinels, tails may be unfilled,
    some positions may lie in the image's padding."""
    out = []
    for half in (0, 1):
        n_sent = (m - (kk + 1)) if (half == 0 and sentinels) else 0
        n_fill = int(rng.integers(0, m - n_sent + 1)) if sentinels else m
        draw = rng.integers(0, 4, n_fill).astype(np.float32) if ties else rng.standard_normal(n_fill).astype(np.float32)
        v = np.concatenate([np.full(n_sent, -FLT_MAX, np.float32), np.sort(draw), np.full(m - n_sent - n_fill, FLT_MAX, np.float32)])
        p = np.concatenate([np.full(n_sent, -1), rng.integers(0, N_REF + (40 if padding else 0), n_fill), np.full(m - n_sent - n_fill, -1)])
        out += [v, p.astype(np.int32)]
    return out


def _brute(v0, p0, v1, p1):
    ent = [(float(v), l, s, int(p)) for l, (vs, ps) in enumerate(((v0, p0), (v1, p1))) for s, (v, p) in enumerate(zip(vs, ps))
           if 0 <= p < N_REF]
    ent.sort(key=lambda e: e[:3])
    ent = ent[:R.RECORD_LEN]
    v = np.array([e[0] for e in ent] + [np.inf] * (R.RECORD_LEN - len(ent)), np.float32)
    p = np.array([e[3] for e in ent] + [-1] * (R.RECORD_LEN - len(ent)), np.int32)
    return v, p


CASES = [(m, kk) for m, kks in ((2, (1,)), (6, (1, 2, 5)), (8, (6, 7))) for kk in kks]


@pytest.mark.parametrize("ties", (False, True))
@pytest.mark.parametrize("sentinels", (False, True))
@pytest.mark.parametrize("m,kk", CASES)
def test_record_is_the_sorted_union(m, kk, ties, sentinels):
    rng = np.random.default_rng(100 * m + 10 * kk + 2 * ties + sentinels)
    for trial in range(300):
        v0, p0, v1, p1 = _lists(rng, m, kk, ties, sentinels, padding=trial % 3 == 0)
        got_v, got_p = R.merge_record(v0, p0, v1, p1, N_REF)
        want_v, want_p = _brute(v0, p0, v1, p1)
        np.testing.assert_array_equal(got_v, want_v)
        np.testing.assert_array_equal(got_p, want_p)
        # valid entries first, ascending; the bound is the M-th smallest of the raw union (sentinels and padding count)
        n_valid = int(R.valid(got_p, N_REF).sum())
        assert R.valid(got_p[:n_valid], N_REF).all() and (np.diff(got_v[:n_valid]) >= 0).all()
        assert R.bound(v0, v1) == np.sort(np.concatenate([v0, v1]))[m - 1]


@pytest.mark.parametrize("ties", (False, True))
@pytest.mark.parametrize("m,kk", CASES)
def test_window_from_record_equals_window_from_lists(m, kk, ties):
    rng = np.random.default_rng(7 * m + kk + 50 * ties)
    fired = quiet = 0
    for trial in range(600):
        v0, p0, v1, p1 = _lists(rng, m, kk, ties, sentinels=True, padding=trial % 3 == 0)
        rv, rp = R.merge_record(v0, p0, v1, p1, N_REF)
        all_v, all_p = np.concatenate([v0, v1]), np.concatenate([p0, p1])
        ok_all, ok_rec = R.valid(all_p, N_REF), R.valid(rp, N_REF)
        tau_lists, tau_rec = R.kth_valid(all_v, ok_all, kk), R.kth_valid(rv, ok_rec, kk)
        assert tau_rec == tau_lists                      # kk <= 7 < RECORD_LEN: the cut never reaches the kk-th entry
        assert tau_rec == (np.float64(rv[kk - 1]) if ok_rec[kk - 1] else np.inf)  # ... which is record slot kk - 1
        width = [0.0, 0.5, 1.0, 3.0][trial % 4]          # 2 eps + 2 noise s^2 of the finaliser: any non-negative width
        window = tau_lists + width
        need_lists = ok_all & (all_v.astype(np.float64) <= window)
        need_rec = ok_rec & (rv.astype(np.float64) <= window)
        if need_rec[R.RECORD_LEN - 1]:                   # the truncation rule: the query goes to the exact scan
            fired += 1
            continue
        quiet += 1
        assert sorted(zip(all_v[need_lists], all_p[need_lists])) == sorted(zip(rv[need_rec], rp[need_rec]))
    assert quiet > 0 and (fired > 0 or not ties or 2 * m <= R.RECORD_LEN)
