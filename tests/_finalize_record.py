"""numpy restatement of the merged candidate record that coarse2_kernel's epilogue files (sknnr_amd/csrc/coarse2.hip.h,
Coarse2Record) and of what finalize_record_kernel derives from it (sknnr_amd/csrc/exact.hip.h).

A query owns two ascending lists of M (value, image position) entries, list 0 on the lower lane and list 1 on the
upper.  Position -1 marks a sentinel (-FLT_MAX at the head of list 0) or an unfilled slot (FLT_MAX at a tail); positions
from n_ref on are image padding.  The record keeps the RECORD_LEN smallest VALID entries of the union, ascending by
(value, list, slot); unused slots hold (+inf, -1).  Every entry finds its own slot by counting the entries ahead of it,
the way a lane does: the valid entries before it in its own list, plus the partner's valid entries that are smaller
(list 1: smaller or equal, so that list 0 goes first among equal values).
"""

from __future__ import annotations

import numpy as np

RECORD_LEN = 8   # kRecordLen
MAX_LIST = 6     # kRecordMaxList: lists of 2 and 6 file records (up to 5 neighbours searched: k, + 1 for X=None)
MAX_KS = 2       # coarse2_record_supported: K-steps (16 features each) of the instances that file records


def valid(pos, n_ref):
    pos = np.asarray(pos)
    return (pos >= 0) & (pos < n_ref)


def merge_record(v0, p0, v1, p1, n_ref):
    """(values float32[RECORD_LEN], positions int32[RECORD_LEN]) of one query."""
    vals = (np.asarray(v0, np.float32), np.asarray(v1, np.float32))
    poss = (np.asarray(p0, np.int32), np.asarray(p1, np.int32))
    oks = (valid(poss[0], n_ref), valid(poss[1], n_ref))
    out_v = np.full(RECORD_LEN, np.inf, np.float32)
    out_p = np.full(RECORD_LEN, -1, np.int32)
    for half in (0, 1):
        pv = np.where(oks[1 - half], vals[1 - half], np.float32(np.nan))  # no comparison holds for NaN
        ahead = 0
        for i in range(len(vals[half])):
            v = vals[half][i]
            with np.errstate(invalid="ignore"):
                r = ahead + int(((pv < v) if half == 0 else (pv <= v)).sum())
            if oks[half][i] and r < RECORD_LEN:
                assert out_p[r] == -1, "two entries claim one slot"
                out_v[r], out_p[r] = v, poss[half][i]
            ahead += int(oks[half][i])
    return out_v, out_p


def bound(v0, v1):
    """pair_union_rank<M, 0>: the M-th smallest entry of the two raw lists together, max_i min(a_i, b_{M-1-i})."""
    a, b = np.asarray(v0, np.float32), np.asarray(v1, np.float32)
    return np.max(np.minimum(a, b[::-1]))


def kth_valid(values, ok, kk):
    """The kk-th smallest valid value (+inf when there are fewer): the finaliser's tau_c."""
    s = np.sort(np.asarray(values, np.float64)[np.asarray(ok)])
    return s[kk - 1] if len(s) >= kk else np.inf


def uses_record(launch: dict, kk: int, raw: bool = False) -> bool:
    """use_record() of sknnr_hip.hip for a call whose pre-filter launch is ``launch`` (tests/_prefilter_dispatch.py,
    expected_launch) with SKNNR_FINALIZE_RECORD unset."""
    return (launch["generation"] == 2 and not raw and launch["ks"] <= MAX_KS and launch["m_list"] <= MAX_LIST
            and launch["rank_extra"] == 0)
