"""The float64 exact scan (exact_scan_kernel, scan_merge_kernel: exact.hip.h), pinned launch by launch and bit for bit.

Every other kernel of the library may be approximate because a row it cannot certify goes to this scan, so nothing stands
behind the scan itself.  Every call here asserts:

- ``Index.debug_last_scan()`` equals the restatement (tests/_scan_dispatch.py ``expected_scan``): formula, the chunked
  instantiation, kk, workgroups and LDS bytes of the first launch, rows offered, slices S, rows handed to the replay;
- ``stats()["exact_only_queries"]`` equals the row count (fail-list cases: ``exact_fallbacks`` > 0 and the record's rows);
- indices and float64 distances equal the oracle bit for bit (``oracle.kneighbors`` composed from one cached
  ``oracle.argkmin`` per shape, ``oracle.kneighbors_hamming`` likewise; tests/test_scan_instances_cpu.py checks the
  composition against the functions themselves);
- for sliced calls, the rows ``scan_merge_kernel`` filed for the sequential replay equal ``expected_replays`` exactly: the
  slices as shards through ``oracle.shard_candidates`` and ``oracle.merge_shards``.  A merge rule that is too eager (every
  row replayed, the slicing dead code) or too lax fails here, not only on rare ties.

CASES names every launch; COVERAGE states, typed in, what each one is (formula, chunked, S, workgroups, LDS bytes), and
tests/test_scan_instances_cpu.py proves the statement from the restatement and that every edge below is in the table.  A
case runs with given rows (row_offset 1000) and as X=None on reference rows [700, 700 + rows) (k = kk - 1, the row's own
index dropped; fewer rows where the index is smaller), both with and without the deterministic order.

How a case makes every row scan-only (``route``): ``d>128`` (no MFMA image), ``kk>31`` (kk = 32 at d <= 128: beyond the
pre-filter's lists, still sliced), ``ids`` (Hamming node ids k + 0.5: not 16-bit integers, the integer path is off).

Laws: ``smooth`` = synth.make_problem; ``dup`` = the same with 200 rows copied twice more across the slice bounds and a
third of the queries exact copies of them; ``lattice`` = integers 0 .. 9 in the first four columns (zeros after), half of
the queries on the lattice and half off it; ``ids`` = three id levels per tree, real weights U(0.05, 1.05).

Groups:

- ``width``: d in 1, 7, 129, 1023, 1024 (last unchunked, dpad = d), 1025 (a chunk one column wide), 2048, 2049, all three
  formulas, 40 rows (sliced) and 6,150 rows (not sliced), 1,500 reference rows;
- ``kk``: 1, 2, 3, 32, 33 (slicing stops), 64, 128, 192 (191 as X=None) on every law, 300 rows; k = 193 and k = 192 with
  X=None are refused with the limit's message;
- ``lds``: per formula and d in 1000, 1024, 1025 the largest kk that fits 150 KiB (derived: expanded 34 / 24 / 24, direct
  and Hamming 192 = kScanMaxKK, which fits) equals the oracle and the first that does not (expanded 35 / 25 / 25) is
  refused; where kk <= 32 the same pair goes through ``merge_shards_host``;
- ``nref``: 32 (= kk), 511, 512, 513, 1,024, 1,025 and 16,385 reference rows (33 steps: S capped at 32, the last slice two
  steps), 12 or 8 rows (one pass);
- ``rows``: 1, scan_nq - 1, scan_nq, scan_nq + 1, 100 passes less 5 rows (S = 10, 24 workgroups idle), the last sliced count
  (512 passes) and the first unsliced one, and 1024 scan_nq + 5 (the grid-stride second pass), 13,000 reference rows;
- fail list: the tight cluster of test_certificate_failures_fall_back_to_the_exact_scan at 512 and 8,000 rows;
- shard merge: 1, 2, 7 and 64 shards at kk = 1 and 32, all formulas, lattice / ids rows (ties across shards);
- reorder: decimals -2, 0, 10, 17 and row_offset 2^31 - 100 on the lattice law.

Finding, asserted as it stands (tests/test_scan_instances_cpu.py): at kk = 1 under the expanded formula the slice that holds
the nearest row is always full and ends at that value, so the uniqueness rule -- oracle.merge_shards states the same one --
replays EVERY row; slicing a kk = 1 call buys nothing.  On smooth rows the replay count is otherwise the number of rows
whose kk nearest all lie in one slice (0 with many slices, about 1 % at 3 slices and kk = 5).  No defect was found in the
kernels or launchers.

Replay counts (``oracle.merge_shards`` over the slices; the device must file the same), expanded formula, written as
given rows deterministic / not, X=None deterministic / not, of the rows of the call.  Every direct and Hamming case: 0.

- kk group, 300 rows, S = 3.  kk = 1: 300 / 300 on every law (the finding above).  smooth: kk 2: 102 / 102, 120 / 120;
  kk 3: 32 / 32, 52 / 52; kk 32: 0.  lattice: kk 2: 162 / 199, 200 / 222; kk 3: 132 / 184, 209 / 287; kk 32: 141 / 283,
  248 / 300.  dup: kk 2: 217 / 217, 146 / 146; kk 3: 74 / 213, 121 / 121; kk 32: 80 / 300, 80 / 299.  The two variants
  at 300 of 300 (lattice kk 32 X=None, dup kk 32 given rows, both without the deterministic order) are replayed whole by
  the rule, and dup kk 32 X=None without the order nearly so: their answers say nothing about the merge, their counts
  do.  With DUP_ROWS = 20 the oracle replays 173 and 101 of 300 rows there (and 168 / 168, 118 / 118; 27 / 131, 55 / 55;
  8, 17 elsewhere), which would leave a real share merged; that law was checked on the CPU only, so it is not the one
  committed.
- width group, kk = 5 at d > 128 (S = 3): 40 given rows: 1 at d = 1024, 2048, 2049, else 0; X=None on 40 rows: 1 at
  d = 1024, else 0; X=None on 800 rows: 12, 11, 6, 2, 2, 6 at d = 129, 1023, 1024, 1025, 2048, 2049.  kk = 32 (d = 1, 7): 0.
- lds group (d = 1024, 1025; kk = 24, 30 rows): 0 given, 1 as X=None.  nref group: n_ref = 513 (the second slice is one
  row: the first is full and ends at the k-th value) 10 of 12 given, 11 of 12 as X=None; the others 0.  rows group: 0.

So the merge's hand-off is exercised mostly by the kk group (kk = 2, 3, 32 on all three laws) and by n_ref = 513; the
width cases add a few rows each.

Teeth (issue part 5), measured on an MI355X with scratch builds of this tree (never committed), 206 GPU tests:

- the "full slice ends at vk" clause of scan_merge_kernel dropped: 26 fail (9 width, 9 kk at kk = 1, 2, 3 on every law,
  2 lds, n_ref = 513, 5 shard merges), all on the replay count; no answer changes, a hidden tie that decides a neighbour
  is too rare to meet, which is why the count is pinned;
- ``scan_slices`` with ``n_ref / 512`` not rounded up (host and device: they share the function): 112 fail, every case
  whose index is not a multiple of 512 rows, on the record's S and the replay count; the answers stay right (the slice
  bounds use their own step count).  The record's S is computed on the host, so a change of the device's S alone
  would show in the replay count and the answers only;
- chunk 2 of ``load_chunk`` started at ``c0 + 1`` (its width taken from the shifted start: in bounds): 22 fail, every
  chunked case under all three formulas (18 width cases at d = 1025, 2048, 2049, the 3 lds cases at d = 1025 and the
  shard merge at d = 1025), all on wrong neighbours;
- the heap admitting ``v <= root`` (expanded formula): 25 fail (every kk on the lattice law, kk = 1, 2, 3 on the dup
  law, the fail list, the 5 reorder cases, the 8 shard merges), all on wrong neighbours.

No mutation fails none.

Wall time on an MI355X: this module 40 s (206 GPU tests, oracle and slice merges on the host included) of a 268 s
``-m gpu`` run (1,533 tests).  The parent commit's GPU suite (its library, every module but this one: 1,327 tests) ran in
240 s on the same kind of box.
"""

from __future__ import annotations

import collections
import functools

import numpy as np
import pytest

import _scan_dispatch as S

gpu = pytest.mark.gpu

ROW_OFFSET = 1_000      # of given rows
SELF_OFFSET = 700       # first reference row of an X=None call (less where the index is small)
DUP_ROWS = 200          # rows of the dup law that appear three times
FORMULAS = (S.EXPANDED, S.DIRECT, S.HAMMING)
WIDTHS = (1, 7, 129, 1023, 1024, 1025, 2048, 2049)
KKS = (1, 2, 3, 32, 33, 64, 128, 192)
LDS_WIDTHS = (1000, 1024, 1025)
NREFS = (32, 511, 512, 513, 1024, 1025, 16385)

Case = collections.namedtuple("Case", "formula law n_ref d kk rows route edges")


def _route(formula, d, kk):
    route = "ids" if formula == S.HAMMING else ("d>128" if d > 128 else "kk>31")
    assert route != "kk>31" or kk > 31
    return route


def _build_cases():
    cases = {}

    def add(group, formula, law, n_ref, d, kk, rows, edges=(), tag=None):
        name = f"{S.FORMULA_NAMES[formula]}/{group}/" + (tag or f"d{d}-kk{kk}-n{n_ref}-r{rows}-{law}")
        assert name not in cases
        cases[name] = Case(formula, law, n_ref, d, kk, rows, _route(formula, d, kk), tuple(edges))

    for f in FORMULAS:
        base = "ids" if f == S.HAMMING else "smooth"
        nq = S.scan_nq(f)
        for d in WIDTHS:
            kk = 5 if d > 128 else 32
            edges = {1: ["odd_d_below_8"], 7: ["odd_d_below_8"], 1024: ["last_unchunked"], 1025: ["chunk_of_one_column"],
                     2048: ["two_full_chunks"], 2049: ["two_chunks_and_one_column"]}.get(d, [])
            add("width", f, base, 1500, d, kk, 40, edges + ["sliced"])
            add("width", f, base, 1500, d, kk, 6150, edges + ["unsliced"])
        for law in (("ids",) if f == S.HAMMING else ("smooth", "lattice", "dup")):
            for kk in KKS:
                edges = {1: ["quicksort_n1"], 2: ["quicksort_n2"], 3: ["quicksort_n3"], 32: ["last_sliced_kk"],
                         33: ["slicing_stops"], 192: ["max_kk"]}.get(kk, [])
                add("kk", f, law, 1500, 129, kk, 300, edges)
        for d in LDS_WIDTHS:
            ok, refused = S.lds_boundary(d, f)  # derived, not typed in
            add("lds", f, base, 600, d, ok, 30, ["lds_largest_accepted"] + (["max_kk_fits"] if refused is None else []),
                tag=f"d{d}-accepted")
        for n_ref in NREFS:
            edges = {32: ["n_ref_is_kk"], 511: ["one_step_short"], 512: ["one_step"], 513: ["slice_of_one_row"],
                     1025: ["last_slice_mostly_padding"], 16385: ["slices_capped_at_32", "uneven_last_slice"]}.get(n_ref, [])
            add("nref", f, base, n_ref, 3, 32, nq, edges)
        for rows, edges in ((1, ["one_row_padding_slots"]), (nq - 1, ["partial_pass"]), (nq, []), (nq + 1, []),
                            (100 * nq - 5, ["idle_workgroups"]), (512 * nq, ["last_sliced_count"]),
                            (512 * nq + 1, ["first_unsliced_count"]), (1024 * nq + 5, ["second_pass"])):
            add("rows", f, base, 13000, 3, 32, rows, edges)
    return cases


CASES = _build_cases()

# name: (formula, chunked, slices S, workgroups of the first launch, dynamic LDS bytes) of the given-rows call
# COVERAGE_BEGIN
COVERAGE = {
    "expanded/width/d1-kk32-n1500-r40-smooth": (0, 0, 3, 1024, 57312),
    "expanded/width/d1-kk32-n1500-r6150-smooth": (0, 0, 1, 1024, 57312),
    "expanded/width/d7-kk32-n1500-r40-smooth": (0, 0, 3, 1024, 57888),
    "expanded/width/d7-kk32-n1500-r6150-smooth": (0, 0, 1, 1024, 57888),
    "expanded/width/d129-kk5-n1500-r40-smooth": (0, 0, 3, 1024, 63168),
    "expanded/width/d129-kk5-n1500-r6150-smooth": (0, 0, 1, 1024, 63168),
    "expanded/width/d1023-kk5-n1500-r40-smooth": (0, 0, 3, 1024, 148992),
    "expanded/width/d1023-kk5-n1500-r6150-smooth": (0, 0, 1, 1024, 148992),
    "expanded/width/d1024-kk5-n1500-r40-smooth": (0, 0, 3, 1024, 148992),
    "expanded/width/d1024-kk5-n1500-r6150-smooth": (0, 0, 1, 1024, 148992),
    "expanded/width/d1025-kk5-n1500-r40-smooth": (0, 1, 3, 1024, 148992),
    "expanded/width/d1025-kk5-n1500-r6150-smooth": (0, 1, 1, 1024, 148992),
    "expanded/width/d2048-kk5-n1500-r40-smooth": (0, 1, 3, 1024, 148992),
    "expanded/width/d2048-kk5-n1500-r6150-smooth": (0, 1, 1, 1024, 148992),
    "expanded/width/d2049-kk5-n1500-r40-smooth": (0, 1, 3, 1024, 148992),
    "expanded/width/d2049-kk5-n1500-r6150-smooth": (0, 1, 1, 1024, 148992),
    "expanded/kk/d129-kk1-n1500-r300-smooth": (0, 0, 3, 1024, 62208),
    "expanded/kk/d129-kk2-n1500-r300-smooth": (0, 0, 3, 1024, 62400),
    "expanded/kk/d129-kk3-n1500-r300-smooth": (0, 0, 3, 1024, 62688),
    "expanded/kk/d129-kk32-n1500-r300-smooth": (0, 0, 3, 1024, 69600),
    "expanded/kk/d129-kk33-n1500-r300-smooth": (0, 0, 1, 25, 69888),
    "expanded/kk/d129-kk64-n1500-r300-smooth": (0, 0, 1, 25, 77280),
    "expanded/kk/d129-kk128-n1500-r300-smooth": (0, 0, 1, 25, 92640),
    "expanded/kk/d129-kk192-n1500-r300-smooth": (0, 0, 1, 25, 108000),
    "expanded/kk/d129-kk1-n1500-r300-lattice": (0, 0, 3, 1024, 62208),
    "expanded/kk/d129-kk2-n1500-r300-lattice": (0, 0, 3, 1024, 62400),
    "expanded/kk/d129-kk3-n1500-r300-lattice": (0, 0, 3, 1024, 62688),
    "expanded/kk/d129-kk32-n1500-r300-lattice": (0, 0, 3, 1024, 69600),
    "expanded/kk/d129-kk33-n1500-r300-lattice": (0, 0, 1, 25, 69888),
    "expanded/kk/d129-kk64-n1500-r300-lattice": (0, 0, 1, 25, 77280),
    "expanded/kk/d129-kk128-n1500-r300-lattice": (0, 0, 1, 25, 92640),
    "expanded/kk/d129-kk192-n1500-r300-lattice": (0, 0, 1, 25, 108000),
    "expanded/kk/d129-kk1-n1500-r300-dup": (0, 0, 3, 1024, 62208),
    "expanded/kk/d129-kk2-n1500-r300-dup": (0, 0, 3, 1024, 62400),
    "expanded/kk/d129-kk3-n1500-r300-dup": (0, 0, 3, 1024, 62688),
    "expanded/kk/d129-kk32-n1500-r300-dup": (0, 0, 3, 1024, 69600),
    "expanded/kk/d129-kk33-n1500-r300-dup": (0, 0, 1, 25, 69888),
    "expanded/kk/d129-kk64-n1500-r300-dup": (0, 0, 1, 25, 77280),
    "expanded/kk/d129-kk128-n1500-r300-dup": (0, 0, 1, 25, 92640),
    "expanded/kk/d129-kk192-n1500-r300-dup": (0, 0, 1, 25, 108000),
    "expanded/lds/d1000-accepted": (0, 0, 1, 3, 153600),
    "expanded/lds/d1024-accepted": (0, 0, 2, 1024, 153504),
    "expanded/lds/d1025-accepted": (0, 1, 2, 1024, 153504),
    "expanded/nref/d3-kk32-n32-r12-smooth": (0, 0, 1, 1, 57504),
    "expanded/nref/d3-kk32-n511-r12-smooth": (0, 0, 1, 1, 57504),
    "expanded/nref/d3-kk32-n512-r12-smooth": (0, 0, 1, 1, 57504),
    "expanded/nref/d3-kk32-n513-r12-smooth": (0, 0, 2, 1024, 57504),
    "expanded/nref/d3-kk32-n1024-r12-smooth": (0, 0, 2, 1024, 57504),
    "expanded/nref/d3-kk32-n1025-r12-smooth": (0, 0, 3, 1024, 57504),
    "expanded/nref/d3-kk32-n16385-r12-smooth": (0, 0, 32, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r1-smooth": (0, 0, 26, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r11-smooth": (0, 0, 26, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r12-smooth": (0, 0, 26, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r13-smooth": (0, 0, 26, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r1195-smooth": (0, 0, 10, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r6144-smooth": (0, 0, 2, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r6145-smooth": (0, 0, 1, 1024, 57504),
    "expanded/rows/d3-kk32-n13000-r12293-smooth": (0, 0, 1, 1024, 57504),
    "direct/width/d1-kk32-n1500-r40-smooth": (1, 0, 3, 1024, 38208),
    "direct/width/d1-kk32-n1500-r6150-smooth": (1, 0, 1, 1024, 38208),
    "direct/width/d7-kk32-n1500-r40-smooth": (1, 0, 3, 1024, 38592),
    "direct/width/d7-kk32-n1500-r6150-smooth": (1, 0, 1, 1024, 38592),
    "direct/width/d129-kk5-n1500-r40-smooth": (1, 0, 3, 1024, 42112),
    "direct/width/d129-kk5-n1500-r6150-smooth": (1, 0, 1, 1024, 42112),
    "direct/width/d1023-kk5-n1500-r40-smooth": (1, 0, 3, 1024, 99328),
    "direct/width/d1023-kk5-n1500-r6150-smooth": (1, 0, 1, 1024, 99328),
    "direct/width/d1024-kk5-n1500-r40-smooth": (1, 0, 3, 1024, 99328),
    "direct/width/d1024-kk5-n1500-r6150-smooth": (1, 0, 1, 1024, 99328),
    "direct/width/d1025-kk5-n1500-r40-smooth": (1, 1, 3, 1024, 99328),
    "direct/width/d1025-kk5-n1500-r6150-smooth": (1, 1, 1, 1024, 99328),
    "direct/width/d2048-kk5-n1500-r40-smooth": (1, 1, 3, 1024, 99328),
    "direct/width/d2048-kk5-n1500-r6150-smooth": (1, 1, 1, 1024, 99328),
    "direct/width/d2049-kk5-n1500-r40-smooth": (1, 1, 3, 1024, 99328),
    "direct/width/d2049-kk5-n1500-r6150-smooth": (1, 1, 1, 1024, 99328),
    "direct/kk/d129-kk1-n1500-r300-smooth": (1, 0, 3, 1024, 41472),
    "direct/kk/d129-kk2-n1500-r300-smooth": (1, 0, 3, 1024, 41600),
    "direct/kk/d129-kk3-n1500-r300-smooth": (1, 0, 3, 1024, 41792),
    "direct/kk/d129-kk32-n1500-r300-smooth": (1, 0, 3, 1024, 46400),
    "direct/kk/d129-kk33-n1500-r300-smooth": (1, 0, 1, 38, 46592),
    "direct/kk/d129-kk64-n1500-r300-smooth": (1, 0, 1, 38, 51520),
    "direct/kk/d129-kk128-n1500-r300-smooth": (1, 0, 1, 38, 61760),
    "direct/kk/d129-kk192-n1500-r300-smooth": (1, 0, 1, 38, 72000),
    "direct/kk/d129-kk1-n1500-r300-lattice": (1, 0, 3, 1024, 41472),
    "direct/kk/d129-kk2-n1500-r300-lattice": (1, 0, 3, 1024, 41600),
    "direct/kk/d129-kk3-n1500-r300-lattice": (1, 0, 3, 1024, 41792),
    "direct/kk/d129-kk32-n1500-r300-lattice": (1, 0, 3, 1024, 46400),
    "direct/kk/d129-kk33-n1500-r300-lattice": (1, 0, 1, 38, 46592),
    "direct/kk/d129-kk64-n1500-r300-lattice": (1, 0, 1, 38, 51520),
    "direct/kk/d129-kk128-n1500-r300-lattice": (1, 0, 1, 38, 61760),
    "direct/kk/d129-kk192-n1500-r300-lattice": (1, 0, 1, 38, 72000),
    "direct/kk/d129-kk1-n1500-r300-dup": (1, 0, 3, 1024, 41472),
    "direct/kk/d129-kk2-n1500-r300-dup": (1, 0, 3, 1024, 41600),
    "direct/kk/d129-kk3-n1500-r300-dup": (1, 0, 3, 1024, 41792),
    "direct/kk/d129-kk32-n1500-r300-dup": (1, 0, 3, 1024, 46400),
    "direct/kk/d129-kk33-n1500-r300-dup": (1, 0, 1, 38, 46592),
    "direct/kk/d129-kk64-n1500-r300-dup": (1, 0, 1, 38, 51520),
    "direct/kk/d129-kk128-n1500-r300-dup": (1, 0, 1, 38, 61760),
    "direct/kk/d129-kk192-n1500-r300-dup": (1, 0, 1, 38, 72000),
    "direct/lds/d1000-accepted": (1, 0, 1, 4, 127680),
    "direct/lds/d1024-accepted": (1, 0, 1, 4, 129216),
    "direct/lds/d1025-accepted": (1, 1, 1, 4, 129216),
    "direct/nref/d3-kk32-n32-r8-smooth": (1, 0, 1, 1, 38336),
    "direct/nref/d3-kk32-n511-r8-smooth": (1, 0, 1, 1, 38336),
    "direct/nref/d3-kk32-n512-r8-smooth": (1, 0, 1, 1, 38336),
    "direct/nref/d3-kk32-n513-r8-smooth": (1, 0, 2, 1024, 38336),
    "direct/nref/d3-kk32-n1024-r8-smooth": (1, 0, 2, 1024, 38336),
    "direct/nref/d3-kk32-n1025-r8-smooth": (1, 0, 3, 1024, 38336),
    "direct/nref/d3-kk32-n16385-r8-smooth": (1, 0, 32, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r1-smooth": (1, 0, 26, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r7-smooth": (1, 0, 26, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r8-smooth": (1, 0, 26, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r9-smooth": (1, 0, 26, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r795-smooth": (1, 0, 10, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r4096-smooth": (1, 0, 2, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r4097-smooth": (1, 0, 1, 1024, 38336),
    "direct/rows/d3-kk32-n13000-r8197-smooth": (1, 0, 1, 1024, 38336),
    "hamming/width/d1-kk32-n1500-r40-ids": (2, 0, 3, 1024, 38208),
    "hamming/width/d1-kk32-n1500-r6150-ids": (2, 0, 1, 1024, 38208),
    "hamming/width/d7-kk32-n1500-r40-ids": (2, 0, 3, 1024, 38592),
    "hamming/width/d7-kk32-n1500-r6150-ids": (2, 0, 1, 1024, 38592),
    "hamming/width/d129-kk5-n1500-r40-ids": (2, 0, 3, 1024, 42112),
    "hamming/width/d129-kk5-n1500-r6150-ids": (2, 0, 1, 1024, 42112),
    "hamming/width/d1023-kk5-n1500-r40-ids": (2, 0, 3, 1024, 99328),
    "hamming/width/d1023-kk5-n1500-r6150-ids": (2, 0, 1, 1024, 99328),
    "hamming/width/d1024-kk5-n1500-r40-ids": (2, 0, 3, 1024, 99328),
    "hamming/width/d1024-kk5-n1500-r6150-ids": (2, 0, 1, 1024, 99328),
    "hamming/width/d1025-kk5-n1500-r40-ids": (2, 1, 3, 1024, 99328),
    "hamming/width/d1025-kk5-n1500-r6150-ids": (2, 1, 1, 1024, 99328),
    "hamming/width/d2048-kk5-n1500-r40-ids": (2, 1, 3, 1024, 99328),
    "hamming/width/d2048-kk5-n1500-r6150-ids": (2, 1, 1, 1024, 99328),
    "hamming/width/d2049-kk5-n1500-r40-ids": (2, 1, 3, 1024, 99328),
    "hamming/width/d2049-kk5-n1500-r6150-ids": (2, 1, 1, 1024, 99328),
    "hamming/kk/d129-kk1-n1500-r300-ids": (2, 0, 3, 1024, 41472),
    "hamming/kk/d129-kk2-n1500-r300-ids": (2, 0, 3, 1024, 41600),
    "hamming/kk/d129-kk3-n1500-r300-ids": (2, 0, 3, 1024, 41792),
    "hamming/kk/d129-kk32-n1500-r300-ids": (2, 0, 3, 1024, 46400),
    "hamming/kk/d129-kk33-n1500-r300-ids": (2, 0, 1, 38, 46592),
    "hamming/kk/d129-kk64-n1500-r300-ids": (2, 0, 1, 38, 51520),
    "hamming/kk/d129-kk128-n1500-r300-ids": (2, 0, 1, 38, 61760),
    "hamming/kk/d129-kk192-n1500-r300-ids": (2, 0, 1, 38, 72000),
    "hamming/lds/d1000-accepted": (2, 0, 1, 4, 127680),
    "hamming/lds/d1024-accepted": (2, 0, 1, 4, 129216),
    "hamming/lds/d1025-accepted": (2, 1, 1, 4, 129216),
    "hamming/nref/d3-kk32-n32-r8-ids": (2, 0, 1, 1, 38336),
    "hamming/nref/d3-kk32-n511-r8-ids": (2, 0, 1, 1, 38336),
    "hamming/nref/d3-kk32-n512-r8-ids": (2, 0, 1, 1, 38336),
    "hamming/nref/d3-kk32-n513-r8-ids": (2, 0, 2, 1024, 38336),
    "hamming/nref/d3-kk32-n1024-r8-ids": (2, 0, 2, 1024, 38336),
    "hamming/nref/d3-kk32-n1025-r8-ids": (2, 0, 3, 1024, 38336),
    "hamming/nref/d3-kk32-n16385-r8-ids": (2, 0, 32, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r1-ids": (2, 0, 26, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r7-ids": (2, 0, 26, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r8-ids": (2, 0, 26, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r9-ids": (2, 0, 26, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r795-ids": (2, 0, 10, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r4096-ids": (2, 0, 2, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r4097-ids": (2, 0, 1, 1024, 38336),
    "hamming/rows/d3-kk32-n13000-r8197-ids": (2, 0, 1, 1024, 38336),
}
# COVERAGE_END


def lds_refusals():
    """(formula, d, smallest refused kk) wherever a kk <= kScanMaxKK does not fit: derived from the restated layout."""
    return [(f, d, S.lds_boundary(d, f)[1]) for f in FORMULAS for d in LDS_WIDTHS if S.lds_boundary(d, f)[1] is not None]


# ---------------------------------------------------------------------------------------------------------------------
# laws and oracle answers (cached: the arrays are shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------
LAWS = ("smooth", "dup", "lattice", "ids")


@functools.lru_cache(maxsize=None)
def reference_rows(law, n_ref, d):
    """(reference rows, Hamming weights or None) of a law."""
    from sknnr_amd import synth

    rng = np.random.default_rng([41, LAWS.index(law), n_ref, d])
    w = None
    if law in ("smooth", "dup"):
        ref = synth.make_features(n_ref, d, seed=0)
        if law == "dup":
            m, third = min(DUP_ROWS, n_ref // 8), n_ref // 3
            ref[third:third + m] = ref[:m]
            ref[2 * third:2 * third + m] = ref[:m]
    elif law == "lattice":
        ref = np.zeros((n_ref, d))
        ref[:, :4] = rng.integers(0, 10, (n_ref, min(d, 4)))
    else:
        ref = rng.integers(0, 3, (n_ref, d)) + 0.5
        w = rng.random(d) + 0.05
        w.setflags(write=False)
    ref.setflags(write=False)
    return ref, w


@functools.lru_cache(maxsize=None)
def query_rows(law, n_ref, d, rows):
    from sknnr_amd import synth

    ref, _ = reference_rows(law, n_ref, d)
    rng = np.random.default_rng([43, LAWS.index(law), n_ref, d, rows])
    if law in ("smooth", "dup"):
        q = synth.make_features(rows, d, seed=1)
        if law == "dup":
            m = min(DUP_ROWS, n_ref // 8)
            q[:rows // 3] = ref[rng.integers(0, m, rows // 3)]
    elif law == "lattice":
        q = np.zeros((rows, d))
        q[:, :4] = rng.integers(0, 10, (rows, min(d, 4)))
        q[rows // 2:, :4] += 0.37 * rng.random((rows - rows // 2, min(d, 4)))
    else:
        q = rng.integers(0, 3, (rows, d)) + 0.5
    q.setflags(write=False)
    return q


def self_window(c):
    """(first row, rows) of the X=None variant of a case: reference rows [700, 700 + rows), less on a small index."""
    off = min(SELF_OFFSET, c.n_ref // 2)
    return off, min(c.rows, c.n_ref - off)


@functools.lru_cache(maxsize=None)
def _argkmin(law, n_ref, d, rows, formula, kk, self_rows):
    from oracle import oracle as O

    ref, w = reference_rows(law, n_ref, d)
    q = ref[self_rows[0]:self_rows[0] + self_rows[1]] if self_rows else query_rows(law, n_ref, d, rows)
    if formula == S.HAMMING:
        return O.argkmin_hamming(q, ref, w, kk)
    return O.argkmin(q, ref, kk, S.FORMULA_NAMES[formula])


def want(c, self_rows, deterministic, decimals=10, row_offset=ROW_OFFSET):
    """oracle.kneighbors / oracle.kneighbors_hamming of a case's call, from one cached argkmin per shape."""
    from oracle import oracle as O

    win = self_window(c) if self_rows else None
    d, i = _argkmin(c.law, c.n_ref, c.d, c.rows, c.formula, c.kk, win)
    if self_rows:
        row_offset = win[0]
        d, i = O.drop_self(d, i, row_offset)
    if deterministic:
        d, i = O.deterministic_reorder(d, i, decimals, row_offset)
    return d, i


@functools.lru_cache(maxsize=None)
def _slice_lists(law, n_ref, d, rows, formula, kk, self_rows, n_slices):
    ref, w = reference_rows(law, n_ref, d)
    q = ref[self_rows[0]:self_rows[0] + self_rows[1]] if self_rows else query_rows(law, n_ref, d, rows)
    return S.slice_candidates(ref, q, kk, formula, S.slice_bounds(n_ref, n_slices), w)


@functools.lru_cache(maxsize=None)
def _merged(law, n_ref, d, rows, formula, kk, self_rows, deterministic, n_slices):
    ref, w = reference_rows(law, n_ref, d)
    lists = _slice_lists(law, n_ref, d, rows, formula, kk, self_rows, n_slices)
    bounds = S.slice_bounds(n_ref, n_slices)
    if self_rows:
        return S.merge_slices(ref, None, kk - 1, formula, bounds, deterministic, row_offset=self_rows[0], nq=self_rows[1], w=w,
                              lists=lists)
    return S.merge_slices(ref, query_rows(law, n_ref, d, rows), kk, formula, bounds, deterministic, row_offset=ROW_OFFSET, w=w,
                          lists=lists)


def call_slices(c, self_rows):
    """S of a case's call: what scan_slices gives for its rows, 1 where the call cannot be sliced."""
    rows = self_window(c)[1] if self_rows else c.rows
    return S.scan_slices(rows, S.scan_nq(c.formula), c.n_ref, c.kk) if S.may_slice(c.formula, c.n_ref, c.kk) else 1


def merged(c, self_rows, deterministic):
    """(dist, idx, replays) of the slice-as-shard merge of a sliced call on the CPU (tests/_scan_dispatch.py merge_slices)."""
    return _merged(c.law, c.n_ref, c.d, c.rows, c.formula, c.kk, self_window(c) if self_rows else None, deterministic,
                   call_slices(c, self_rows))


def replays(c, self_rows, deterministic):
    return merged(c, self_rows, deterministic)[2] if call_slices(c, self_rows) > 1 else 0


def variants(c):
    """(self_rows, deterministic) of the calls of a case: given rows and X=None (kk >= 2), each with and without the
    deterministic order."""
    out = []
    for self_rows in (False, True):
        if not (self_rows and c.kk < 2):
            out += [(self_rows, True), (self_rows, False)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shared state: one handle per data set, kept for the module
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


def _index(N, ref, w):
    ix = N.Index(np.ascontiguousarray(ref))
    if w is not None:
        ix.set_hamming_weights(np.ascontiguousarray(w))
    return ix


@pytest.fixture(scope="module")
def handles(N):
    made = {}

    def get(law, n_ref, d):
        if (law, n_ref, d) not in made:
            made[law, n_ref, d] = _index(N, *reference_rows(law, n_ref, d))
        return made[law, n_ref, d]

    yield get
    for ix in made.values():
        ix.close()


def _compare(problems, what, got, wanted):
    (dist, idx), (od, oi) = got, wanted
    if not np.array_equal(idx, oi):
        problems.append(f"{what}: wrong neighbours in {int((idx != oi).any(axis=1).sum())} of {len(oi)} rows")
    elif not np.array_equal(dist, od):
        problems.append(f"{what}: wrong distances in {int((dist != od).any(axis=1).sum())} of {len(od)} rows")


def run_case(N, ix, c, record, decimals=10, row_offset=ROW_OFFSET, only=None):
    """Every variant of a case: answer, record, statistics and replay count, each checked and reported."""
    problems = []
    for self_rows, det in (only or variants(c)):
        what = f"{'X=None' if self_rows else 'X given'}, deterministic {det}"
        off, rows = self_window(c) if self_rows else (row_offset, c.rows)
        ix.reset_stats()
        opts = ix.make_opts(c.kk - 1 if self_rows else c.kk, exclude_self=self_rows, deterministic=det, decimals=decimals,
                            formula=c.formula, row_offset=off)
        got = ix.kneighbors_host(None if self_rows else query_rows(c.law, c.n_ref, c.d, c.rows), opts, nq=rows)
        st, rec = ix.stats(), ix.debug_last_scan()
        n_replay = replays(c, self_rows, det)
        record(f"replays ({what})", n_replay)
        expect = S.expected_scan(c.formula, c.n_ref, c.d, c.kk, rows, replays=n_replay)
        if rec != expect:
            problems.append(f"{what}: record {rec}, restated {expect}")
        if (st["queries"], st["exact_only_queries"], st["coarse_queries"]) != (rows, rows, 0):
            problems.append(f"{what}: statistics {st}")
        _compare(problems, what, got, want(c, self_rows, det, decimals, row_offset))
    assert not problems, "; ".join(problems)


def _group(group):
    return [n for n in CASES if f"/{group}/" in n]


# ---------------------------------------------------------------------------------------------------------------------
# the table's cases
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", _group("width"))
def test_widths(N, handles, record_property, name):
    """Odd widths below 8, the last unchunked width, a chunk of one column, two full chunks and 2,049 columns, sliced and
    not, under every formula: the chunked expanded formula reads qn from global memory and runs its fma chain across chunks."""
    c = CASES[name]
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property)


@gpu
@pytest.mark.parametrize("name", _group("kk"))
def test_kk(N, handles, record_property, name):
    """The heap replay, the quicksort's explicit stack, drop-self and the insertion reorder from kk = 1 to 192 on smooth,
    integer-lattice and duplicated rows, with and without the deterministic order."""
    c = CASES[name]
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property)


@gpu
@pytest.mark.parametrize("formula", FORMULAS)
def test_first_refused_k(N, handles, formula):
    """k = 193, and k = 192 with X=None, are refused with the limit in the message (validate_call)."""
    law = "ids" if formula == S.HAMMING else "smooth"
    ix = handles(law, 1500, 129)
    q = query_rows(law, 1500, 129, 300)
    with pytest.raises(N.HipBackendError, match=r"n_neighbors = 193 exceeds the HIP backend's limit of 192$") as e:
        ix.kneighbors_host(q, ix.make_opts(S.MAX_KK + 1, formula=formula))
    assert e.value.code == N.ERR_UNSUPPORTED
    with pytest.raises(N.HipBackendError, match=r"n_neighbors = 192 exceeds the HIP backend's limit of 191 with X=None") as e:
        ix.kneighbors_host(None, ix.make_opts(S.MAX_KK, formula=formula, exclude_self=True), nq=300)
    assert e.value.code == N.ERR_UNSUPPORTED


@gpu
@pytest.mark.parametrize("name", _group("lds"))
def test_lds_largest_accepted(N, handles, record_property, name):
    """The largest kk whose workgroup image passes the 150 KiB check: the launch asks for almost the whole LDS of a CU."""
    c = CASES[name]
    assert S.fits(c.d, c.kk, c.formula) and (c.kk == S.MAX_KK or not S.fits(c.d, c.kk + 1, c.formula))
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property)


@gpu
@pytest.mark.parametrize("formula, d, kk", lds_refusals())
def test_lds_smallest_refused(N, handles, formula, d, kk):
    """One neighbour more than fits is refused, for given rows and (one fewer k) for X=None, with the message of launch_scan;
    the record says no scan ran."""
    law = "ids" if formula == S.HAMMING else "smooth"
    ix = handles(law, 600, d)
    q = query_rows(law, 600, d, 30)
    for self_rows in (False, True):
        k = kk - 1 if self_rows else kk
        with pytest.raises(N.HipBackendError, match=rf"n_neighbors = {k} with d = {d} {S.REFUSAL}") as e:
            ix.kneighbors_host(None if self_rows else q, ix.make_opts(k, formula=formula, exclude_self=self_rows, row_offset=100), nq=30)
        assert e.value.code == N.ERR_UNSUPPORTED
        assert ix.debug_last_scan() == S.no_scan()


@gpu
@pytest.mark.parametrize("name", _group("nref"))
def test_reference_rows(N, handles, record_property, name):
    """Slice bounds fall on multiples of 512 reference rows: one step and its neighbours, a slice of one row, 33 steps."""
    c = CASES[name]
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property)


@gpu
@pytest.mark.parametrize("name", _group("rows"))
def test_row_counts(N, handles, record_property, name):
    """One row, a pass with padding slots, the slicing threshold from both sides, idle workgroups, the second pass."""
    c = CASES[name]
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property)


# ---------------------------------------------------------------------------------------------------------------------
# the scan behind the pre-filter: only the rows the finaliser lists, and the device's count drives S
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tight_cluster(rows):
    """The data of test_certificate_failures_fall_back_to_the_exact_scan (tests/test_hip_parity.py)."""
    rng = np.random.default_rng(5)
    base = rng.standard_normal((1, 16)) * 100.0
    ref = base + 1e-5 * rng.standard_normal((3000, 16))
    ref[0] += 50.0  # one far row keeps the coarse scale large
    return ref, base + 1e-5 * np.random.default_rng([5, rows]).standard_normal((rows, 16))


@gpu
def test_fail_list_entry(N, record_property):
    """512 and 8,000 rows of the tight cluster (k = 5): the listed rows fall on both sides of the slicing threshold of
    6,144; the record follows the device's count, the answers are compared over the whole call."""
    from oracle import oracle as O

    seen = []
    ix = N.Index(tight_cluster(512)[0])
    try:
        for rows in (512, 8000):
            ref, q = tight_cluster(rows)
            ix.reset_stats()
            got = ix.kneighbors_host(q, ix.make_opts(5, row_offset=ROW_OFFSET))
            st, rec = ix.stats(), ix.debug_last_scan()
            record_property(f"listed rows of {rows}", rec["rows"])
            assert st["coarse_queries"] == rows and st["exact_fallbacks"] == rec["rows"] > 0, (st, rec)
            n_slices = S.scan_slices(rec["rows"], S.scan_nq(S.EXPANDED), 3000, 5)
            seen.append(n_slices)
            # which rows the finaliser listed is the device's business: the replay count is pinned (``exact``) when every
            # row is listed or no row of the call would be replayed.  Otherwise it is ONLY BOUNDED here, by the rows of the
            # whole call that would be replayed (the record's own count is put into the expectation); the sliced hand-off
            # itself is pinned by the table's cases.  On this data about a third of the rows would be replayed (cancellation-
            # quantised ties), so the count is pinned only when the finaliser lists every row.
            sv, si = S.slice_candidates(ref, q, 5, S.EXPANDED, S.slice_bounds(3000, n_slices)) if n_slices > 1 else (None, None)
            would = 0 if n_slices == 1 else O.merge_shards(ref, q, sv, si, 5, "expanded", row_offset=ROW_OFFSET)[2]
            exact = rec["rows"] == rows or would == 0
            expect = S.expected_scan(S.EXPANDED, 3000, 16, 5, rows, listed=rec["rows"], replays=would if exact else rec["replayed_rows"])
            assert rec == expect and rec["replayed_rows"] <= would, (rec, expect, would)
            record_property(f"replay count pinned at {rows} rows", bool(exact))
            od, oi = O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET)
            np.testing.assert_array_equal(got[1], oi)
            np.testing.assert_array_equal(got[0], od)
    finally:
        ix.close()
    assert seen[0] > 1 and seen[1] == 1, f"slices {seen}: the two counts are meant to fall on both sides of the threshold"


# ---------------------------------------------------------------------------------------------------------------------
# the shard merge: the same kernel over the candidate lists of reference shards
# ---------------------------------------------------------------------------------------------------------------------
SHARD_ROWS, SHARD_QUERIES, SHARD_D = 2560, 60, 129


def shard_bounds_of(n_shards):
    cuts = [SHARD_ROWS * g // n_shards for g in range(n_shards + 1)]
    return list(zip(cuts[:-1], cuts[1:]))


def _shard_lists(N, ref, w, q, kk, formula, bounds):
    """(n_shards, rows, kk) candidates from one handle per shard (sknnr_shard_candidates)."""
    vals, idxs = [], []
    for a, b in bounds:
        ix = _index(N, ref[a:b], w)
        try:
            v, i = ix.shard_candidates_host(q, ix.make_opts(kk, formula=formula, deterministic=False), index_offset=a)
            assert ix.debug_last_scan()["formula_plus_1"] == formula + 1
        finally:
            ix.close()
        vals.append(v)
        idxs.append(i)
    return np.stack(vals), np.stack(idxs)


@gpu
@pytest.mark.parametrize("kk", [1, 32])
@pytest.mark.parametrize("n_shards", [1, 2, 7, 64])
@pytest.mark.parametrize("formula", FORMULAS)
def test_shard_merge(N, handles, record_property, formula, n_shards, kk):
    """shard_candidates_host + merge_shards_host on rows with ties across the shards: the shards' lists, the answers and
    the replay count against oracle.shard_candidates / oracle.merge_shards, given rows and X=None, with and without the
    deterministic order."""
    law = "ids" if formula == S.HAMMING else "lattice"
    ref, w = reference_rows(law, SHARD_ROWS, SHARD_D)
    bounds = shard_bounds_of(n_shards)
    full = handles(law, SHARD_ROWS, SHARD_D)
    problems = []
    for self_rows in (False, True):
        if self_rows and kk < 2:
            continue
        q = ref[SELF_OFFSET:SELF_OFFSET + SHARD_QUERIES] if self_rows else query_rows(law, SHARD_ROWS, SHARD_D, SHARD_QUERIES)
        sv, si = _shard_lists(N, ref, w, q, kk, formula, bounds)
        ov, oi = S.slice_candidates(ref, q, kk, formula, bounds, w)
        _compare(problems, f"shard lists (X=None {self_rows})", (sv.reshape(-1, kk), si.reshape(-1, kk)),
                 (ov.reshape(-1, kk), oi.reshape(-1, kk)))
        for det in (True, False):
            what = f"{'X=None' if self_rows else 'X given'}, deterministic {det}"
            off = SELF_OFFSET if self_rows else ROW_OFFSET
            md, mi, n_replay = S.merge_slices(ref, None if self_rows else q, kk - 1 if self_rows else kk, formula, bounds, det,
                                              row_offset=off, nq=SHARD_QUERIES, w=w)
            record_property(f"replays ({what})", n_replay)
            full.reset_stats()
            opts = full.make_opts(kk - 1 if self_rows else kk, exclude_self=self_rows, deterministic=det, formula=formula, row_offset=off)
            got = full.merge_shards_host(None if self_rows else q, opts, sv, si, nq=SHARD_QUERIES)
            rec = full.debug_last_scan()
            expect = S.expected_scan(formula, SHARD_ROWS, SHARD_D, kk, SHARD_QUERIES, replays=n_replay, shards=n_shards)
            if rec != expect:
                problems.append(f"{what}: record {rec}, restated {expect}")
            if full.stats()["exact_only_queries"] != SHARD_QUERIES:
                problems.append(f"{what}: statistics {full.stats()}")
            _compare(problems, what, got, (md, mi))
    assert not problems, "; ".join(problems)


@gpu
@pytest.mark.parametrize("formula, d, refused", [r for r in lds_refusals() if r[2] - 1 <= S.SLICE_MAX_KK])
def test_lds_boundary_through_the_shard_merge(N, handles, formula, d, refused):
    """Where the boundary lies at kk <= 32 (the merge serves no more) the shard merge meets it too: the largest accepted kk
    is merged (two shards of 300 rows) and equals the oracle, the smallest refused one raises the same message."""
    law = "ids" if formula == S.HAMMING else "smooth"
    ref, w = reference_rows(law, 600, d)
    q = query_rows(law, 600, d, 30)
    bounds = [(0, 300), (300, 600)]
    full = handles(law, 600, d)
    kk = refused - 1
    sv, si = _shard_lists(N, ref, w, q, kk, formula, bounds)
    md, mi, n_replay = S.merge_slices(ref, q, kk, formula, bounds, True, row_offset=ROW_OFFSET, w=w)
    got = full.merge_shards_host(q, full.make_opts(kk, formula=formula, row_offset=ROW_OFFSET), sv, si)
    assert full.debug_last_scan() == S.expected_scan(formula, 600, d, kk, 30, replays=n_replay, shards=2)
    np.testing.assert_array_equal(got[1], mi)
    np.testing.assert_array_equal(got[0], md)
    one_more = np.concatenate([sv, sv[:, :, -1:]], axis=2), np.concatenate([si, si[:, :, -1:]], axis=2)
    with pytest.raises(N.HipBackendError, match=rf"n_neighbors = {refused} with d = {d} {S.REFUSAL}") as e:
        full.merge_shards_host(q, full.make_opts(refused, formula=formula), *one_more)
    assert e.value.code == N.ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# the reorder's inputs
# ---------------------------------------------------------------------------------------------------------------------
REORDER = Case(S.EXPANDED, "lattice", 1500, 129, 8, 200, "d>128", ("reorder",))


@gpu
@pytest.mark.parametrize("formula", FORMULAS)
@pytest.mark.parametrize("decimals", [-2, 0, 10, 17])
def test_reorder_decimals(N, handles, record_property, formula, decimals):
    """decimals below zero divide by the power of ten, the others multiply (round_key's two branches), on tie-heavy rows."""
    c = REORDER._replace(formula=formula, law="ids" if formula == S.HAMMING else "lattice", route=_route(formula, 129, 8))
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property, decimals=decimals, only=[(False, True), (True, True)])


@gpu
@pytest.mark.parametrize("formula", FORMULAS)
def test_reorder_row_offset_near_2_31(N, handles, record_property, formula):
    """|index - row| with rows numbered from 2^31 - 100: the key needs 64 bits."""
    c = REORDER._replace(formula=formula, law="ids" if formula == S.HAMMING else "lattice", route=_route(formula, 129, 8))
    run_case(N, handles(c.law, c.n_ref, c.d), c, record_property, row_offset=2 ** 31 - 100, only=[(False, True)])
