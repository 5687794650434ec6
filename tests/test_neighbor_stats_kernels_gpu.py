"""The summary kernels (sknnr_amd/csrc/summary.hip.h) run alone through ``sknnr_summarize_from_neighbors`` on synthetic
``(dist, idx)`` device buffers -- no search runs here -- and compared with the numpy restatement (tests/_neighbor_stats.py)
by ``assert_array_equal`` over the WHOLE output buffer: every value (NaN positions equal) and the 64 guard bytes in front of
and behind it, which must keep their pattern.  The scheme is that of test_narrow_kernels_gpu.py.

Shapes: nq of {1, 2, 63, 64, 65, 255, 256, 257, 1000} x k of {1, 2, 3, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 192} x t
of {1, 2, 3, 5}.  The k cover both kernels (k <= 8 in registers, above it the wide one), numpy's 8-term block boundary, its
128-term split and the split point's ``% 8`` adjustment (129 -> 64 + 65, 136 -> 64 + 72, 192 -> 96 + 96).  The weights
(uniform, distance, explicit) and the statistic tables rotate over the cases; the tables include all-``mean``, no ``mean``,
and every statistic in the first and in the last column (``test_the_rotation_covers``).

Data: 400 reference rows whose target columns are labels of 2, 3 or 7 classes -- ``3 c - 2`` plus an inexact fraction, in
several binades, so that a sum of labels depends on the order of its additions; distances are multiples
of 0.5, sorted per row, so that equal and zero distances, and with them tied votes, are common; one row in eight starts
with one to three exact zeros.  Explicit weights come from {0, 0.5, 1, 2, 1/3, 0.1}, with some rows all zero (``mode``
then gives NaN).  The inexact weights (1 / 1.5, 1 / 2.5, 1/3, 0.1) make every sum depend on the order of its additions.
``test_the_cases_hold_tied_votes`` asserts, on the restatement alone and on the compared cases themselves, that every
(weights, k <= 17) combination has rows of a ``mode`` column whose top vote is tied (k = 1 cannot: one neighbour, one label);
``test_the_cases_tell_the_two_orders_of_the_mean_apart`` that the ``std`` cases under uniform weights, t >= 2 and k >= 8 see
the difference between the sequential and the pairwise mean.  Every device buffer carries 257 rows of slack, so that a
kernel that ran a whole workgroup past the end would stay inside its buffers and show in the bytes behind the output.

Every case also checks ``sknnr_debug_last_summary`` (the kernel that ran; none for an all-``mean`` table; whether the
predict kernels ran), and that the ``mean`` columns of a mixed table equal ``sknnr_predict_from_neighbors`` of the same
inputs.

Measured on an MI355X: the 531 tests of this module (504 kernel cases, 27 others) take 4.9 s, of which 1.9 s are the first
case's device set-up and 1.3 s the device-free check of the two orders of the mean; no kernel case takes more than 0.1 s.

Scratch mutations of summary.hip.h (never committed; the slack rows keep every access inside its buffer), each run once
against this module, and the kernel cases that fail under them, of 504 (no other test of the module fails):

=====================================================================  ======  ==========================================
mutation                                                               failed  where
=====================================================================  ======  ==========================================
``vote >= best_vote`` for the vote's strict ``>`` and its tie rule        159  only cases with a ``mode`` column (159 of
                                                                               the 229 that have one): every k from 1 (the
                                                                               all-zero explicit rows, NaN lost) to 192,
                                                                               both kernels, all three weight modes
a sequential sum for ``np_sum`` and ``np_sum_small``                      130  k >= 8 only (k = 8: 10 cases, the 8-term
                                                                               tree; k > 8: 120); 128 through ``std``, 2
                                                                               through the votes of ``mode`` alone
the unit compiled with contraction on (fma in ``std`` and its mean)       109  only cases with a ``std`` column, k >= 8 (5
                                                                               at k = 8, 104 above), all weight modes
the tail bound rounded up to the workgroup (whole workgroups run)         398  every case that launches the kernel with
                                                                               ``nq * columns`` no multiple of 256 (all
                                                                               but nq = 256 and a few nq = 64 cases), on
                                                                               the bytes behind the output
the pairwise for the sequential ``m`` (uniform weights, t >= 2)            35  only uniform weights, t >= 2, a ``std``
                                                                               column and k >= 8 (3 at k = 8, 32 above)
=====================================================================  ======  ==========================================

Below 8 terms numpy's pairwise sum is the sequential one and an fma of exactly representable products changes nothing, so
the three order mutations cannot show at k < 8; the inexact labels are what makes them show from k = 8 on.
"""

from __future__ import annotations

import numpy as np
import pytest

import _neighbor_stats as NS

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
SLACK_ROWS = 257  # rows of slack behind every device buffer: more than one 256-thread workgroup can reach past the end
NQS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
KS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 192)
TS = (1, 2, 3, 5)
WEIGHTS = ("uniform", "distance", "explicit")
N_REF = 400
CLASSES = (2, 3, 7)
S = NS.STATISTICS
# statistic tables per t: all-mean, no mean, every statistic first and last
TABLES = {
    1: [(s,) for s in S],
    2: [("mean", "mean")] + [(s, S[(i + 2) % 6]) for i, s in enumerate(S)] + [(S[(i + 3) % 6], s) for i, s in enumerate(S)]
       + [("mode", "std"), ("min", "nearest")],
    3: [("mean", "mean", "mean"), ("mean", "mean", "mode"), ("mode", "std", "max"), ("min", "nearest", "std")]
       + [(s, "mean", S[(i + 1) % 6]) for i, s in enumerate(S)] + [(S[(i + 4) % 6], "mode", s) for i, s in enumerate(S)],
    5: [("mean",) * 5, ("mode", "min", "max", "nearest", "std"), ("std", "mode", "mode", "min", "nearest")]
       + [(s, "mean", "std", "mode", S[(i + 5) % 6]) for i, s in enumerate(S)]
       + [(S[(i + 1) % 6], "max", "mean", "nearest", s) for i, s in enumerate(S)],
}


def cases():
    out = []
    for a, nq in enumerate(NQS):
        for b, k in enumerate(KS):
            for c, t in enumerate(TS):
                n = a * len(KS) * len(TS) + b * len(TS) + c
                tabs = TABLES[t]
                out.append((nq, k, t, WEIGHTS[(a + b + c) % 3], tabs[(a * 5 + b * 3 + c + n // 7) % len(tabs)]))
    return out


# The next three tests check the CASES, on the restatement alone: they touch no device and nothing the feature adds (so they
# pass wherever numpy runs).  They live here, under the module's gpu mark, because they guard what test_summary_kernels
# compares: its rotation, its tied votes and its order-sensitive means.
def test_the_rotation_covers():
    seen = cases()
    for t in TS:
        tabs = {tab for _, _, tt, _, tab in seen if tt == t}
        assert tabs == set(TABLES[t]), (t, set(TABLES[t]) - tabs)
        for s in S:
            assert any(tab[0] == s for tab in tabs) and any(tab[-1] == s for tab in tabs)
        assert any(all(s == "mean" for s in tab) for tab in tabs)
        assert t == 1 or any("mean" not in tab for tab in tabs)
    for w in WEIGHTS:
        for k in KS:
            assert {s for _, kk, _, ww, tab in seen if kk == k and ww == w for s in tab} == set(S), (w, k)
        for nq in NQS:
            assert any(n == nq and ww == w for n, _, _, ww, _ in seen)


def class_values(n_classes, rng):
    """Distinct label values that are no integers and lie in several binades: ``3 c - 2`` plus an inexact fraction scaled by
    a power of two, so that a sum of labels depends on the order of its additions."""
    return 3.0 * np.arange(n_classes) - 2.0 + rng.uniform(0.05, 0.45, size=n_classes) * np.exp2(rng.integers(-6, 2, size=n_classes))


def targets(t):
    rng = np.random.default_rng(1000 + t)
    cols = []
    for j in range(t):
        n_classes = CLASSES[(j + t) % 3]
        cols.append(class_values(n_classes, rng)[rng.integers(0, n_classes, size=N_REF)])
    return np.ascontiguousarray(np.stack(cols, axis=1))


def neighbours(nq, k, weights, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N_REF, size=(nq, k)).astype(np.int64)
    dist = np.sort(rng.integers(1, 13, size=(nq, k)) * 0.5, axis=1)
    zero = np.flatnonzero(rng.integers(0, 8, size=nq) == 0)
    for r in zero:
        dist[r, : min(k, 1 + r % 3)] = 0.0
    w = None
    if weights == "explicit":
        w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 1 / 3, 0.1]), size=(nq, k))
        w[rng.integers(0, 16, size=nq) == 0] = 0.0
    return dist, idx, w


def case_seed(nq, k, t):
    return nq * 1000 + k * 7 + t


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("k", [k for k in KS if 2 <= k <= 17])
def test_the_cases_hold_tied_votes(weights, k):
    """On the restatement alone, over the very inputs ``test_summary_kernels`` compares: among the cases of this (weights, k)
    some row of a ``mode`` column has its largest vote shared by two labels.  (k = 1: one neighbour, one label, no tie.)"""
    tied = 0
    for nq, kk, t, ww_, table in cases():
        if kk != k or ww_ != weights or "mode" not in table:
            continue
        y = targets(t)
        dist, idx, w = neighbours(nq, k, weights, seed=case_seed(nq, k, t))
        ww = NS.weights_of(dist, idx, w, weights)
        tied += sum(int(NS.top_vote_tied(y[idx, j], ww).sum()) for j, s in enumerate(table) if s == "mode")
    assert tied > 0, (weights, k)


def test_the_cases_tell_the_two_orders_of_the_mean_apart():
    """On the restatement alone: under uniform weights and t >= 2 the ``std`` is taken around the mean whose k values are
    added in order; the inexact labels make that differ from the pairwise mean in the compared cases with k >= 8."""
    differ = 0
    for nq, k, t, weights, table in cases():
        if weights != "uniform" or t < 2 or k < 8 or "std" not in table:
            continue
        y = targets(t)
        dist, idx, _ = neighbours(nq, k, weights, seed=case_seed(nq, k, t))
        for j, s in enumerate(table):
            if s == "std":
                v = np.ascontiguousarray(y[idx, j])
                seq = NS.mean_of(y, dist, idx, None, "uniform")[:, j]
                differ += int((seq != np.sum(v, axis=1) / k).sum())
    assert differ > 0


@pytest.fixture(scope="module")
def indices():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    ref = np.random.default_rng(5).standard_normal((N_REF, 2))
    made = {t: (_native.Index(ref, targets(t)), targets(t)) for t in TS}
    yield made
    for ix, _ in made.values():
        ix.close()


def guarded(nbytes, slack):
    import torch

    host = np.full(GUARD + nbytes + GUARD + slack, PATTERN, dtype=np.uint8)
    return host, torch.from_numpy(host.copy()).cuda()


def padded(a, fill):
    """``a`` on the device with SLACK_ROWS more rows of ``fill`` behind it: a workgroup's worth of rows past the end stays
    inside the buffer (and reads reference row 0 at distance and weight 1)."""
    import torch

    return torch.from_numpy(np.concatenate([a, np.full((SLACK_ROWS, a.shape[1]), fill, dtype=a.dtype)])).cuda()


@pytest.mark.parametrize("nq, k, t, weights, table", cases())
def test_summary_kernels(indices, nq, k, t, weights, table):
    import torch

    from sknnr_amd import _native

    ix, y = indices[t]
    dist, idx, w = neighbours(nq, k, weights, seed=case_seed(nq, k, t))
    with np.errstate(all="ignore"):
        want = NS.summarize(y, dist, idx, w, weights, table)
    host, d_out = guarded(nq * t * 8, SLACK_ROWS * t * 8)
    d_dist, d_idx = padded(dist, 1.0), padded(idx, 0)
    d_w = padded(w, 1.0) if w is not None else None
    mode = {"uniform": _native.WEIGHTS_UNIFORM, "distance": _native.WEIGHTS_DISTANCE, "explicit": _native.WEIGHTS_EXPLICIT}[weights]
    stat = np.array([NS.CODES[s] for s in table], dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    ix.summarize_from_neighbors_device(d_dist.data_ptr(), d_idx.data_ptr(), 0 if d_w is None else d_w.data_ptr(), nq, k,
                                       mode, stat, d_out.data_ptr() + GUARD, stream)
    rec = ix.debug_last_summary()
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    msg = f"nq={nq} k={k} t={t} {weights} {table}"
    end = GUARD + nq * t * 8
    values = got[GUARD:end].view(np.float64).reshape(nq, t)
    np.testing.assert_array_equal(values, want, err_msg=msg)
    # (the guards, and the slack behind, byte for byte; the values above as float64, since a NaN has more than one bit pattern)
    np.testing.assert_array_equal(got[:GUARD], host[:GUARD], err_msg="front guard: " + msg)
    np.testing.assert_array_equal(got[end:], host[end:], err_msg="back guard: " + msg)
    nc = sum(s != "mean" for s in table)
    assert rec == dict(path=0 if nc == 0 else (1 if k <= 8 else 2), rows=nq, cols=nc, k=k, predict_ran=int(nc < t), t=t,
                       weight_mode=mode, reserved=0), msg
    if 0 < nc < t:  # the mean columns of a mixed table: what the predict entry gives for the same inputs
        d_pred = torch.empty((nq, t), dtype=torch.float64, device="cuda")
        ix.predict_from_neighbors_device(d_dist.data_ptr(), d_idx.data_ptr(), 0 if d_w is None else d_w.data_ptr(), nq, k,
                                         mode, d_pred.data_ptr(), stream)
        torch.cuda.synchronize()
        cols = [j for j, s in enumerate(table) if s == "mean"]
        np.testing.assert_array_equal(values[:, cols], d_pred.cpu().numpy()[:, cols], err_msg="mean columns: " + msg)
        assert ix.debug_last_summary()["path"] == 0


def test_refusals_of_the_c_entry(indices):
    """Unknown codes, a missing table and k above the limit fail before any device work, with a message."""
    import ctypes

    from sknnr_amd import _native

    lib = _native.load()
    ix, _ = indices[3]
    buf = (ctypes.c_uint64 * 2048)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = (ctypes.c_int32 * 3)(0, 1, 5)
    h = ix.handle
    for bad in ((0, 6, 0), (-1, 0, 0), (0, 0, 99)):
        assert lib.sknnr_summarize_from_neighbors(h, p, p, None, 2, 3, 0, (ctypes.c_int32 * 3)(*bad), p, 0, None) == _native.ERR_INVALID
        assert b"is no sknnr_statistic" in lib.sknnr_last_error()
    assert lib.sknnr_summarize_from_neighbors(h, p, p, None, 2, 3, 0, None, p, 0, None) == _native.ERR_INVALID
    assert b"stat is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_summarize_from_neighbors(h, p, p, None, 2, 193, 0, ok, p, 0, None) == _native.ERR_UNSUPPORTED
    assert b"exceeds" in lib.sknnr_last_error()
    assert lib.sknnr_summarize_from_neighbors(h, None, p, None, 2, 3, 1, ok, p, 0, None) == _native.ERR_INVALID
    assert lib.sknnr_summarize_from_neighbors(h, p, p, None, 2, 3, 2, ok, p, 0, None) == _native.ERR_INVALID
    opts = _native.Index.make_opts(3)
    assert lib.sknnr_summarize(h, p, 2, ctypes.byref(opts), None, p, None, None, 0, None) == _native.ERR_INVALID
    assert b"stat is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_summarize(h, p, 2, ctypes.byref(opts), (ctypes.c_int32 * 3)(0, 7, 0), p, None, None, 0, None) == _native.ERR_INVALID
    assert b"stat[1] = 7" in lib.sknnr_last_error()
