"""Which Euclidean pre-filter launch a call makes, restated from the host code (no GPU needed).

tests/test_prefilter_instances_gpu.py asserts that ``Index.debug_last_prefilter()`` reports exactly what
``expected_launch`` predicts.  When dispatch changes in the library, these restatements stop matching and the
instance tests fail loudly instead of quietly testing another kernel.  Sources, all in sknnr_amd/csrc:

- ``coarse_list_len`` (both overloads), ``use_coarse2``, ``launch_coarse2``, ``chunk_rows``, and ``plan_search``, which
  applies them once per call: sknnr_hip.hip (tests/test_search_plan_cpu.py holds this file against ``plan_search`` itself,
  through ``sknnr_debug_search_plan``, without a GPU)
- ``coarse2_supported``, ``coarse2_waves``, ``coarse2_rank_extra``, ``tiles_per_stage2``, ``tile2_bytes``,
  ``kSeedTiles``, ``kCoarse2Nqb``, ``kCoarse2MaxKK*``: coarse2.hip.h
- ``coarse_waves`` (first generation), ``kRowQuantum``: coarse.hip.h
- the cell depth of an index: ``sknnr_index_create`` (sknnr_hip.hip), ``kCellMaxDepth``: bucket.hip.h; ``n_tiles2``:
  ``image_stages2`` (sknnr_hip.hip) times ``tiles_per_stage2``

Only the default build and default process environment are restated: the process-static knobs
(``SKNNR_COARSE_V2``, ``SKNNR_V2_BIG_K``, ``SKNNR_COARSE_TAIL``, ``SKNNR_CHUNK_ROWS``) are assumed unset.
"""

from __future__ import annotations

ROW_QUANTUM = 6144          # kRowQuantum
MAX_KK = 31                 # kCoarseMaxKK: more neighbours (+ self) than this go to the exact scan alone
SEED_TILES = 64             # kSeedTiles
NQB2 = 2                    # kCoarse2Nqb: 32-query blocks per wave
TAIL_WAVES = 4              # kCoarse2TailWaves
CUS = 256                   # kCusPerDevice
CELL_MAX_DEPTH = 6          # kCellMaxDepth
MAX_KK6, MAX_KK8, MAX_KK12, MAX_KK16 = 7, 15, 23, 31


def ks_of(d: int) -> int:
    return (d + 15) // 16


def tiles_per_stage2(ks: int) -> int:
    return 16 if ks <= 2 else 8


def tile2_bytes(ks: int) -> int:
    return ks * 1024 + 128


def n_tiles2(n_ref: int, ks: int) -> int:
    tps = tiles_per_stage2(ks)
    return ((n_ref + 31) // 32 + tps - 1) // tps * tps


def coarse2_supported(ks: int, m: int) -> bool:
    return ks <= 4 and m in (2, 6, 8, 12, 16) and (m != 2 or ks <= 2)


def coarse2_waves(ks: int, m: int) -> int:
    return 12 if (m == 16 or (m == 12 and ks >= 2) or (m == 8 and ks >= 4)) else 16


def coarse2_rank_extra(m: int, kk: int) -> int:
    if kk + 1 <= m:
        return 0
    if m == 6:
        return 3
    if m == 8:
        return 4 if kk <= 10 else (7 if kk <= 13 else 8)
    if m == 12:
        return 10 if kk <= 20 else 12
    return 6 if kk <= 20 else (11 if kk <= 25 else (15 if kk <= 30 else 16))


def use_coarse2(n_ref: int, d: int, m: int) -> bool:
    ks = ks_of(d)
    if ks > 4:
        return False
    t = n_tiles2(n_ref, ks)
    return t >= 2 * SEED_TILES and t * tile2_bytes(ks) < 1 << 32 and t * 32 < 1 << 26 and coarse2_supported(ks, m)


def min_coarse2_n_ref(ks: int) -> int:
    """The smallest reference set use_coarse2 accepts: 128 tiles after rounding up to whole stages."""
    tps = tiles_per_stage2(ks)
    tiles = 2 * SEED_TILES - tps + 1  # the fewest tiles that round up to 128
    return (tiles - 1) * 32 + 1


def coarse_list_len_plain(kk: int) -> int:
    return 2 if kk <= 1 else (6 if kk <= 5 else (8 if kk <= 7 else (16 if kk <= 15 else 32)))


def coarse_list_len(n_ref: int, d: int, kk: int) -> int:
    if 5 < kk <= MAX_KK6 and not use_coarse2(n_ref, d, 8) and use_coarse2(n_ref, d, 6):
        return 6
    if 7 < kk <= MAX_KK8 and use_coarse2(n_ref, d, 8):
        return 8
    if 15 < kk <= MAX_KK12 and use_coarse2(n_ref, d, 12):
        return 12
    if 15 < kk <= MAX_KK16 and use_coarse2(n_ref, d, 16):
        return 16
    return coarse_list_len_plain(kk)


def coarse1_waves(ks: int, m: int) -> int:
    light = ks <= 2 and m <= 8
    medium = (3 <= ks <= 6 and m <= 8) or (ks == 7 and m <= 6) or (ks <= 5 and m == 16)
    return 16 if light else (12 if medium else 8)


def cell_depth(n_ref: int, d: int, cells_env: int) -> int:
    """Depth of the cell tree of an index created with SKNNR_CELLS=cells_env (forced: the order replay is skipped)."""
    want = min(cells_env, CELL_MAX_DEPTH, d)
    while want > 0 and (n_ref >> want) < 512:
        want -= 1
    return want if (n_tiles2(n_ref, ks_of(d)) >= 2 * SEED_TILES and want >= 2) else 0


def coarse2_split(rows: int, bulk_waves: int) -> tuple[int, int]:
    """(rows of the bulk launch, rows of the 4-wave thin launch) of launch_coarse2 for one chunk of ``rows`` live rows."""
    qpb, qpb_tail = bulk_waves * NQB2 * 32, TAIL_WAVES * NQB2 * 32
    n_wg = (rows + qpb - 1) // qpb
    tail_wg = n_wg % CUS
    if tail_wg > CUS // (bulk_waves // TAIL_WAVES):
        tail_wg = 0
    bulk = (n_wg - tail_wg) * qpb
    thin = min(tail_wg * qpb, (rows - bulk + qpb_tail - 1) // qpb_tail * qpb_tail) if tail_wg else 0
    return bulk, thin


def expected_launch(n_ref: int, d: int, kk: int, nq: int, cells_env: int | None = None, depth: int | None = None) -> dict:
    """What debug_last_prefilter() reports after one Euclidean call of ``nq`` rows searching ``kk`` neighbours (k + 1 for
    X=None) on an index of ``n_ref`` x ``d`` rows.  The cell depth is ``depth`` when given, else that of an index made with
    SKNNR_CELLS=cells_env (``cells_env`` None: 0, for callers that force the plain order).  One device chunk per call."""
    rec = dict(generation=0, ks=0, m_list=0, rank_extra=0, bulk_waves=0, bulk_rows=0, thin_rows=0, cell_depth=0)
    ks = ks_of(d)
    if ks > 8 or kk > MAX_KK:
        return rec
    m = coarse_list_len(n_ref, d, kk)
    rec.update(ks=ks, m_list=m)
    if use_coarse2(n_ref, d, m):
        waves = coarse2_waves(ks, m)
        bulk, thin = coarse2_split(nq, waves)
        if depth is None:
            depth = 0 if cells_env is None else cell_depth(n_ref, d, cells_env)
        rec.update(generation=2, rank_extra=coarse2_rank_extra(m, kk), bulk_waves=waves if bulk else 0, bulk_rows=bulk,
                   thin_rows=thin, cell_depth=depth)
    else:
        rec.update(generation=1, bulk_waves=coarse1_waves(ks, m), bulk_rows=(nq + ROW_QUANTUM - 1) // ROW_QUANTUM * ROW_QUANTUM)
    return rec


def reachable_instances() -> list[tuple[int, int, int]]:
    """Every (KS, M, E) of coarse2_kernel that default dispatch reaches, over kk = 1 .. 31 on a large enough index."""
    out = set()
    for ks in (1, 2, 3, 4):
        for kk in range(1, MAX_KK + 1):
            m = coarse_list_len(1 << 20, 16 * ks, kk)
            if use_coarse2(1 << 20, 16 * ks, m):
                out.add((ks, m, coarse2_rank_extra(m, kk)))
    return sorted(out)
