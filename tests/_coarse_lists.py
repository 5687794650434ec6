"""The list contract of the first-generation pre-filter (sknnr_amd/csrc/coarse.hip.h, coarse_kernel), restated on the host
in numpy -- no GPU needed.

``check_lists`` asserts what the kernel promises about the two candidate lists it files per query, given the matrix of
ranking values ``V`` that ``Index.debug_coarse_matrix`` returns (coarse_matrix_kernel issues the same MFMAs in the same
order as the product kernel, so its values are bit-identical to the ones the product kernel ranks).  With J = kk + 1 and
B[q] the J-th smallest value of row q:

- the running threshold ``thr`` never drops below the final J-th best value, so a row below B is a hit once visited;
- a row below B is always visited, because |correct - main| <= margin (the skip test compares main with thr + margin);
- a lane drops an entry only when J entries (lane half 0, whose list starts with M - J sentinels) or M entries (half 1)
  at or below it remain.

``predicted_fallbacks`` restates finalize_core's decision (exact.hip.h) for lists that honour that contract, and
``replay`` is a plain model of the sweep itself (per-lane lists, sentinels, hit queue, flush, direct insertion on a full
queue, pair_union_rank_m) that tests/test_coarse_lists_cpu.py runs under ``check_lists``, whole and mutated.
"""

from __future__ import annotations

import numpy as np

import _rescue as R

FLT_MAX = np.float32(np.finfo(np.float32).max)
LIST_LENGTHS = (2, 6, 8, 16, 32)
SHIFT_INSERT_FROM = 32  # SKNNR_SHIFT_INSERT_FROM


def queue_cap(m):
    return 2 if m == 2 else 4


def queue_flush_at(m):
    return 2 if m == 2 else 3


def acc_row(r, h):
    """Row of the 32x32 accumulator held in register r of a lane in half h."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def jth_smallest(V, j):
    """B: the j-th smallest value of every row of V (FLT_MAX where the row has fewer than j values)."""
    n, n_ref = V.shape
    if n_ref < j:
        return np.full(n, FLT_MAX, dtype=np.float32)
    return np.partition(V, j - 1, axis=1)[:, j - 1]


def list_violations(val, pos, perm, V, kk, M, rows=None):
    """Every clause of the contract that the lists break: a list of (clause, queries in breach, first such query).
    ``rows``: mask of the queries to check (default: all; the caller leaves out those whose image is not finite)."""
    val = np.asarray(val)
    pos = np.asarray(pos)
    n, n_ref = V.shape
    J = kk + 1
    assert 1 <= kk and J <= M, (kk, M)
    assert val.shape == pos.shape == (n, 2, M) and val.dtype == np.float32 and V.dtype == np.float32
    assert perm.shape == (n_ref,)
    keep = np.ones(n, dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
    q_of = np.flatnonzero(keep)
    val, pos, V = val[keep], pos[keep].astype(np.int64), V[keep]
    n = len(q_of)
    bad = []

    def clause(name, ok_per_query):
        wrong = np.flatnonzero(~ok_per_query)
        if len(wrong):
            bad.append((name, len(wrong), int(q_of[wrong[0]])))

    if n == 0:
        return bad
    ns = M - J
    clause("ascending", (val[:, :, 1:] >= val[:, :, :-1]).all(axis=(1, 2)))
    real = pos >= 0
    lead = np.zeros((2, M), dtype=bool)
    lead[0, :ns] = True
    sentinel = (val == -FLT_MAX) & ~real
    clause("sentinel prefix", (sentinel[:, lead].all(axis=1) if ns else np.ones(n, dtype=bool))
           & ~sentinel[:, ~lead].any(axis=1))
    unused = ~real & ~lead[None]
    clause("unused slots", ((val == FLT_MAX) | ~unused).all(axis=(1, 2)) & ((pos == -1) | real).all(axis=(1, 2)))
    in_range = real & (pos < n_ref)
    clause("position range", (in_range == real).all(axis=(1, 2)))
    half_of = (pos % 8 >= 4).astype(np.int64)
    clause("own half", ((half_of == np.arange(2)[None, :, None]) | ~real).all(axis=(1, 2)))
    flat = np.where(real, pos, -1 - np.arange(2 * M).reshape(2, M)[None]).reshape(n, 2 * M)
    flat.sort(axis=1)
    clause("no position twice", (flat[:, 1:] != flat[:, :-1]).all(axis=1))
    # (a position out of range is reported above; read row 0 for it here)
    row = perm[np.where(in_range, pos, 0)]
    want = np.take_along_axis(V, row.reshape(n, 2 * M), axis=1).reshape(n, 2, M)
    clause("value bits", ((val.view(np.uint32) == want.view(np.uint32)) | ~in_range).all(axis=(1, 2)))
    B = jth_smallest(V, J)
    clause("rows below B", (in_range & (val < B[:, None, None])).sum(axis=(1, 2)) == (V < B[:, None]).sum(axis=1))
    listed = np.sort(np.where(real, val, FLT_MAX).reshape(n, 2 * M), axis=1)[:, :J]
    pad = np.full((n, max(J - n_ref, 0)), FLT_MAX, dtype=np.float32)
    padded = np.concatenate([V, pad], axis=1) if pad.shape[1] else V
    smallest = np.sort(np.partition(padded, J - 1, axis=1)[:, :J], axis=1)
    clause("J smallest", (listed == smallest).all(axis=1))
    if n_ref < J:
        clause("every row listed", real.sum(axis=(1, 2)) == n_ref)
    return bad


def check_lists(val, pos, perm, V, kk, M, rows=None):
    bad = list_violations(val, pos, perm, V, kk, M, rows)
    assert not bad, "; ".join(f"{name}: {cnt} queries, first {q}" for name, cnt, q in bad)


# ---------------------------------------------------------------------------------------------------------------------
# finalize_core's decision for lists that honour the contract
# ---------------------------------------------------------------------------------------------------------------------
def image_constants(ref, mu, s):
    """ymax and mu2 (expanded formula) as sknnr_index_create computes them: sequential float64 sums over the columns."""
    ref = np.asarray(ref, dtype=np.float64)
    d = ref.shape[1]
    yn = np.zeros(len(ref))
    m2 = np.float64(0.0)
    for c in range(d):
        b = s * (ref[:, c] - mu[c])
        yn = yn + b * b
        m2 = m2 + mu[c] * mu[c]
    return dict(s=float(s), ymax=float(np.sqrt(yn.max())), mu2=float(2.0 * (np.sqrt(m2) * (1.0 + 1e-12))), d=d,
                ks=(d + 15) // 16)


def predicted_fallbacks(V, d2, idx, qn, consts, kk, deterministic=True):
    """(fall-back, undetermined) per query, for a first-generation pre-filter that honours the contract.

    ``d2`` / ``idx``: each query's min(kk + 1, n_ref) smallest reference-arithmetic squared distances, ascending, and
    their rows (oracle.argkmin(..., squared=True), sorted); ``qn``: |q'|^2 as the preparation kernel filed it;
    ``consts``: image_constants.  The lists then give t_min = B and hold every row below B, and

        certified  <=>  n_usable >= kk  and  tau < inf  and  (qn + B - eps) inv_s2 - noise > tau

    with tau the kk-th smallest float64 d2 of the usable candidates.  Where the inequality holds for the true kk-th
    smallest d2, every row at or below it has a ranking value below B (the certificate's own argument), so it is listed
    and tau is that value; where it fails, tau is no smaller and it fails too.  X=None searches kk = k + 1 rows, the
    row itself among them: dropping it happens behind the decision.  The exact-tie rule hands over a certified query
    whose kk-th and (kk + 1)-th re-scored values are equal (deterministic) or that holds any pair of equal values among
    its first kk + 1 (not deterministic).

    Undetermined: the inequality holds, but a row the decision needs is not surely a usable candidate -- one of the kk
    nearest, or a row tied with the kk-th, whose ranking value is not below B (nor the only value at B) or lies outside
    the re-score window tau_c + 2 eps + 2 noise s^2.  By the certificate's argument there is none."""
    V = np.asarray(V)
    n, n_ref = V.shape
    J = kk + 1
    qn = np.asarray(qn, dtype=np.float64)
    s = np.float64(consts["s"])
    s2, inv_s2 = s * s, np.float64(1.0) / (s * s)
    fallback = np.ones(n, dtype=bool)
    undetermined = np.zeros(n, dtype=bool)
    if n_ref < kk:
        return fallback, undetermined
    with np.errstate(all="ignore"):
        eps, noise = R.certificate_terms(qn, consts["ymax"], s, consts["d"], consts["ks"], consts["mu2"], generation=1)
        B = jth_smallest(V, J).astype(np.float64)
        tau = d2[:, kk - 1]
        bound = R.bound(qn, B, eps, noise, inv_s2)
        certified = np.isfinite(qn) & (tau < np.inf) & (bound > tau)
        has_next = d2.shape[1] > kk
        if deterministic:
            tied = (d2[:, kk] == tau) if has_next else np.zeros(n, dtype=bool)
        else:
            tied = (np.diff(d2[:, :kk + 1], axis=1) == 0).any(axis=1)
        # which of the rows the decision reads are surely usable candidates
        tau_c = jth_smallest(V, kk).astype(np.float64)
        window = tau_c + 2.0 * eps + 2.0 * noise * s2
        v_of = np.take_along_axis(V, idx, axis=1).astype(np.float64)
        only_at_b = ((V <= B[:, None].astype(np.float32)).sum(axis=1) == J)[:, None]
        sure = ((v_of < B[:, None]) | ((v_of == B[:, None]) & only_at_b)) & (v_of <= window[:, None])
        reads = np.ones(d2.shape, dtype=bool)
        if has_next:
            reads[:, kk] = d2[:, kk] == tau
    fallback = ~certified | tied
    undetermined = certified & (reads & ~sure).any(axis=1)
    return fallback, undetermined


# ---------------------------------------------------------------------------------------------------------------------
# a plain replay of the sweep
# ---------------------------------------------------------------------------------------------------------------------
class _Lane:
    def __init__(self, m, n_sentinel):
        self.vals = [-FLT_MAX if i < n_sentinel else FLT_MAX for i in range(m)]
        self.idxs = [-1] * m
        self.thr = FLT_MAX
        self.queue = []


def list_insert(vals, idxs, v, i):
    """list_insert<M>, literally: the bubble below 32 entries (the last entry is overwritten whatever it holds), the
    positional form from 32 on (nothing changes unless v is below an entry)."""
    m = len(vals)
    if m >= SHIFT_INSERT_FROM:
        for p in range(m - 1, -1, -1):
            if v < vals[p]:
                lower_left = p > 0 and v < vals[p - 1]
                vals[p], idxs[p] = (vals[p - 1], idxs[p - 1]) if lower_left else (v, i)
    else:
        vals[m - 1], idxs[m - 1] = v, i
        for p in range(m - 1, 0, -1):
            if vals[p] < vals[p - 1]:
                vals[p], vals[p - 1] = vals[p - 1], vals[p]
                idxs[p], idxs[p - 1] = idxs[p - 1], idxs[p]


def pair_union_rank_m(a, b):
    m = len(a)
    return max(min(a[i], b[m - 1 - i]) for i in range(m))


def replay(V_img, kk, M, margin=0.0, mutation=None):
    """The sweep of one wave over ``V_img`` (up to 32 queries x positions of the image, float32): (val, pos) as the kernel
    files them, (nq, 2, M).  Main and corrected products are the same number here; ``margin`` widens the skip test as
    the kernel's does.  Every ballot is wave-wide, as in the kernel: one query's hit makes every query look.

    mutation: None, 'sentinel' (one sentinel too many), 'stale_thr' (thr not tightened on direct insertion) or
    'drop_queued' (the flush forgets the last queued entry of a full queue)."""
    V_img = np.asarray(V_img, dtype=np.float32)
    nq, n_pos = V_img.shape
    assert nq <= 32
    margin = np.float32(margin)
    n_sentinel = M - (kk + 1) + (1 if mutation == "sentinel" else 0)
    lanes = [[_Lane(M, n_sentinel if h == 0 else 0) for h in range(2)] for _ in range(nq)]
    n_tiles = (n_pos + 31) // 32
    tiles = np.full((nq, n_tiles * 32), np.inf, dtype=np.float32)  # padding positions: |r'|^2 = +inf
    tiles[:, :n_pos] = V_img
    groups = [range(3 * k, 16 if k == 4 else 3 * k + 3) for k in range(5)]

    def flush():
        for q in range(nq):
            for lane in lanes[q]:
                queued = lane.queue
                if mutation == "drop_queued" and len(queued) == queue_cap(M):
                    queued = queued[:-1]
                for v, i in queued:
                    if v < lane.vals[M - 1]:
                        list_insert(lane.vals, lane.idxs, v, i)
                lane.queue = []
            thr = pair_union_rank_m(lanes[q][0].vals, lanes[q][1].vals)
            lanes[q][0].thr = lanes[q][1].thr = thr

    for t in range(n_tiles):
        acc = [[[tiles[q, 32 * t + acc_row(r, h)] for r in range(16)] for h in range(2)] for q in range(nq)]
        loose = [[np.float32(lanes[q][h].thr + margin) for h in range(2)] for q in range(nq)]
        if not any(min(acc[q][h]) < loose[q][h] for q in range(nq) for h in range(2)):
            continue
        for g in groups:
            if not any(min(acc[q][h][r] for r in g) < loose[q][h] for q in range(nq) for h in range(2)):
                continue
            for r in g:
                for q in range(nq):
                    for h in range(2):
                        lane, v = lanes[q][h], acc[q][h][r]
                        if not v < lane.thr:
                            continue
                        if len(lane.queue) < queue_cap(M):
                            lane.queue.append((v, 32 * t + acc_row(r, h)))
                        else:
                            list_insert(lane.vals, lane.idxs, v, 32 * t + acc_row(r, h))
                            if mutation != "stale_thr":
                                lane.thr = min(lane.thr, lane.vals[M - 1])
        if any(len(lanes[q][h].queue) >= queue_flush_at(M) for q in range(nq) for h in range(2)):
            flush()
    flush()
    val = np.array([[lanes[q][h].vals for h in range(2)] for q in range(nq)], dtype=np.float32).reshape(nq, 2, M)
    pos = np.array([[lanes[q][h].idxs for h in range(2)] for q in range(nq)], dtype=np.int32).reshape(nq, 2, M)
    return val, pos
