"""The integer pre-filter of the weighted-Hamming search, restated on the host (no GPU needed).

tests/test_hamming_instances_gpu.py asserts that ``Index.debug_last_hamming()`` reports exactly what ``expected_record``
predicts and that the candidate lists the device wrote (``Index.debug_hamming_candidates``) are exactly what
``candidates`` computes.  A pre-filter that ranks by a wrong D^ but still hands the exact answer to the float64 re-score
fails there.  Sources, all in sknnr_amd/csrc:

- ``h16_ok``: ``sknnr_index_set_hamming_weights`` (sknnr_hip.hip): every reference id an integer in [0, 65535]
  (``hamming_pack_kernel``), at most 4,096 trees and ``hamming_rescore_lds`` <= 150 KiB (hamming.hip.h)
- ``quantise``: the 16-bit weights of ``sknnr_index_set_hamming_weights``.  numpy's float64 arithmetic is the host's:
  the host unit is built with -ffp-contract=off and no fast-math (sknnr_amd/_build.py)
- ``ham_int``: ``plan_search``; the 2^18-row device chunks and ``band = T + 2``: ``hamming_pass`` (sknnr_hip.hip)
- ``compacts``, ``seed_rows``, ``kHamCand``, ``kHamMaxKK``, the 256-row steps and ``candidates``:
  ``ham_compacts``, ``ham_seed_rows`` and ``hamming_coarse_kernel`` (hamming.hip.h)
- ``handed_to_scan``: ``hamming_rescore_kernel`` sends a row with fewer than kk candidates (or -1) to the exact scan

Only the default process environment is restated: ``SKNNR_HAMMING_INT`` is assumed unset.
"""

from __future__ import annotations

import numpy as np

CAND = 192                  # kHamCand: candidate slots per query row
MAX_KK = 32                 # kHamMaxKK: more neighbours (+ self) than this go to the float64 scan alone
STEP = 256                  # kHamWaves * 64: reference rows per step of hamming_coarse_kernel
CHUNK_ROWS = 1 << 18        # query rows per device chunk of the integer path
MAX_TREES = 4096            # the re-score's register image of the query (kMaxChunks = 8 chunks of 512 trees)
RESCORE_LDS_MAX = 150 * 1024
NONE = 0xFFFFFFFF           # the kernel's "no value" (unsigned)


def compacts(kk: int) -> bool:
    return kk >= 8


def seed_rows(n_ref: int, kk: int) -> int:
    if not compacts(kk):
        return 0
    rows = min(4096, max(256, n_ref // 16)) // 256 * 256
    return min(n_ref, rows)


def rescore_lds(t: int) -> int:
    """hamming_rescore_lds: the float64 weights, then per wave 64 candidates x one flag byte per 8 trees of every
    512-tree chunk."""
    return (t + 1) // 2 * 2 * 8 + 4 * 64 * ((t + 511) // 512 * 64)


def band(t: int) -> int:
    return t + 2


def ids_ok(ids) -> np.ndarray:
    """Per row: every id an integer in [0, 65535] (hamming_pack_kernel; -0.0 is 0)."""
    ids = np.asarray(ids, dtype=np.float64)
    ok = (ids >= 0.0) & (ids <= 65535.0) & (ids == np.floor(ids))
    return ok.all(axis=1)


def h16_ok(ref_ids) -> bool:
    t = np.shape(ref_ids)[1]
    return bool(ids_ok(ref_ids).all()) and t <= MAX_TREES and rescore_lds(t) <= RESCORE_LDS_MAX


def max_trees_served() -> int:
    t = MAX_TREES
    while rescore_lds(t) > RESCORE_LDS_MAX:
        t -= 1
    return t


def ham_int(ref_ids, kk: int) -> bool:
    return h16_ok(ref_ids) and kk <= MAX_KK


def quantise(w) -> np.ndarray:
    """The 16-bit weights: round(w / wmax * 65535), so the largest weight is 65535 and a zero weight stays 0."""
    w = np.asarray(w, dtype=np.float64)
    wmax = w.max()
    return np.minimum(65535.0, np.floor(w / wmax * 65535.0 + 0.5)).astype(np.int64)


def expected_record(ref_ids, nq: int, kk: int, handed: int) -> dict:
    """What debug_last_hamming() reports after one call of ``nq`` rows searching ``kk`` neighbours (k + 1 for X=None),
    ``handed`` being the restated rows with fewer than kk candidates (``handed_to_scan``)."""
    n_ref, t = np.shape(ref_ids)
    if not ham_int(ref_ids, kk):
        return dict(ran=0, kk=0, compacts=0, seed_rows=0, band=0, tree_pairs=0, chunks=0, handed_to_scan=0)
    return dict(ran=1, kk=kk, compacts=int(compacts(kk)), seed_rows=seed_rows(n_ref, kk), band=band(t),
                tree_pairs=(t + 1) // 2, chunks=(nq + CHUNK_ROWS - 1) // CHUNK_ROWS, handed_to_scan=handed)


def handed_to_scan(cnt, kk: int) -> int:
    """Rows hamming_rescore_kernel puts on the fail list: fewer candidates than neighbours asked for (-1 included)."""
    return int((np.asarray(cnt) < kk).sum())


def _packed(ids) -> np.ndarray:
    """The 16-bit ids as the pack kernel writes them: an id that is not a 16-bit integer packs as 0."""
    ids = np.asarray(ids, dtype=np.float64)
    ok = (ids >= 0.0) & (ids <= 65535.0) & (ids == np.floor(ids))
    return np.where(ok, ids, 0.0).astype(np.int64)


def dhat(ref_ids, q_ids, wq) -> np.ndarray:
    """D^(q, r) = sum_t wq_t [q_t != r_t] in integers, (nq, n_ref) int64."""
    r, q = _packed(ref_ids), _packed(q_ids)
    wq = np.asarray(wq, dtype=np.int64)
    out = np.zeros((q.shape[0], r.shape[0]), dtype=np.int64)
    if r.shape[1] <= q.shape[0]:
        for t in range(r.shape[1]):
            if wq[t]:
                out += wq[t] * (q[:, t, None] != r[None, :, t])
    else:
        for i in range(q.shape[0]):
            out[i] = (r != q[i]) @ wq
    return out


def _lim(kth: np.ndarray, b: int) -> np.ndarray:
    return np.where(kth > NONE - b, NONE, kth + b)


def _insert(top: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Each row of ``top`` (ascending) with its value of ``v`` put in, the largest dropped: the kernel's shift insert."""
    prev = np.concatenate([np.full((len(top), 1), -1, dtype=np.int64), top[:, :-1]], axis=1)
    return np.minimum(np.maximum(prev, v[:, None]), top)


def _select(D: np.ndarray, kk: int, b: int):
    """hamming_coarse_kernel's selection for the query rows of ``D`` (n, n_ref): (cnt, ids) before the bad-id rule."""
    n, n_ref = D.shape
    comp = compacts(kk)
    seed = seed_rows(n_ref, kk)
    top = np.full((n, kk), NONE, dtype=np.int64)
    seed_kth = np.full(n, NONE, dtype=np.int64)
    cnt = np.zeros(n, dtype=np.int64)
    cand = np.zeros((n, CAND), dtype=np.int64)
    cval = np.zeros((n, CAND), dtype=np.int64)
    for phase in ((0, 1) if seed > 0 else (1,)):
        j_end = seed if phase == 0 else n_ref
        for j0 in range(0, j_end, STEP):
            blk = D[:, j0:min(j0 + STEP, n_ref)]
            # the ballot: rows within band of the bound at the start of the step (a superset: the bound only drops)
            mask = blk <= _lim(np.minimum(top[:, -1], seed_kth), b)[:, None]
            order = np.argsort(~mask, axis=1, kind="stable")
            n_pos = mask.sum(axis=1)
            for s in range(int(n_pos.max(initial=0))):
                act = np.flatnonzero(n_pos > s)
                col = order[act, s]
                v = blk[act, col]
                lim = _lim(np.minimum(top[act, -1], seed_kth[act]), b)
                ok = v <= lim  # admitted against the bound of this moment, in ascending row order
                act, col, v, lim = act[ok], col[ok], v[ok], lim[ok]
                if act.size == 0:
                    continue
                if phase == 1:
                    if comp:
                        for i in np.flatnonzero(cnt[act] == CAND):
                            q = act[i]
                            keep = cval[q] <= lim[i]
                            kept = int(keep.sum())
                            cand[q, :kept] = cand[q, keep]
                            cval[q, :kept] = cval[q, keep]
                            cnt[q] = kept
                    c = cnt[act]
                    app = (c >= 0) & (c < CAND)
                    cand[act[app], c[app]] = j0 + col[app]
                    cval[act[app], c[app]] = v[app]
                    cnt[act[app]] += 1
                    cnt[act[c == CAND]] = -1  # (compaction on: still full after it)
                top[act] = _insert(top[act], v)
        if phase == 0:
            seed_kth = top[:, -1].copy()
            top[:] = NONE
    ids = np.full((n, CAND), -1, dtype=np.int64)
    lim = _lim(top[:, -1], b)
    for q in np.flatnonzero(cnt >= 0):
        c = cnt[q]
        keep = cval[q, :c] <= lim[q] if comp else np.ones(c, dtype=bool)
        kept = cand[q, :c][keep]
        ids[q, :kept.size] = kept
        cnt[q] = kept.size
    return cnt, ids


def candidates(ref_ids, q_ids, w, kk: int, D=None, block_elems: int = 1 << 23):
    """Exactly what hamming_coarse_kernel writes for the query rows ``q_ids`` (any number: no device chunking here):
    ``cnt`` (nq,) the candidates per row, -1 for an overflowing list or a row with an id that is not a 16-bit integer, and
    ``ids`` (nq, 192), row i's candidates ascending in ``ids[i, :cnt[i]]``, -1 past them.  ``D``: dhat of these rows, when
    the caller has it."""
    ref_ids = np.asarray(ref_ids, dtype=np.float64)
    q_ids = np.asarray(q_ids, dtype=np.float64)
    n_ref, t = ref_ids.shape
    wq = quantise(w)
    bad = ~ids_ok(q_ids)
    nq = q_ids.shape[0]
    cnt = np.empty(nq, dtype=np.int64)
    ids = np.empty((nq, CAND), dtype=np.int64)
    rows = max(1, block_elems // max(n_ref, 1))
    for r0 in range(0, nq, rows):
        sl = slice(r0, min(nq, r0 + rows))
        d = dhat(ref_ids, q_ids[sl], wq) if D is None else D[sl]
        cnt[sl], ids[sl] = _select(d, kk, band(t))
    cnt[bad] = -1
    ids[bad] = -1
    return cnt, ids
