"""The exact scan's restatement (tests/_scan_dispatch.py) and the case table of tests/test_scan_instances_gpu.py, checked
without a GPU: the constants against the sources, the table against the restatement, every edge the table must hold, the
LDS boundary, and the slice merge on the CPU -- a slice is a reference shard, so ``oracle.shard_candidates`` per slice and
``oracle.merge_shards`` must give ``oracle.kneighbors`` bit for bit, and their replay count is what the device must file.
On smooth rows that count is exactly the number of rows whose kk nearest all lie in one slice (the rule's "a full slice
ends at the k-th value" clause; no tie fires any other): 0 wherever a pass has 10 or more slices at kk = 32, a few rows
at 2 or 3 slices and kk = 5.  On the lattice and duplicate laws it is strictly between 0 and the row count in every
variant (given rows and X=None, with and without the deterministic order) at kk = 2, 3 and 32, but for the two variants
in ALL_REPLAY, which the rule replays whole.  So the GPU tests can hide neither behind a merge that replays everything nor
behind one that replays nothing.  The counts are listed in the docstring of tests/test_scan_instances_gpu.py.

Finding (the rule as oracle.merge_shards states it, which the device follows): at kk = 1 under the expanded formula the
slice that holds the nearest row is always full and ends at that value, so EVERY row is replayed and slicing a kk = 1
call buys nothing.  A single-slot heap keeps the first smallest value it meets, so the merged answer would be right; the
rule is stricter than it needs to be there.  Asserted here as it stands (count = rows), not changed."""

from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest

import _scan_dispatch as S
import test_scan_instances_gpu as G
from conftest import ROOT

CSRC = os.path.join(ROOT, "sknnr_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _const(text, name):
    """The value of ``constexpr <type> name = <integer expression>;`` with earlier constants of the restatement substituted."""
    expr = re.search(rf"constexpr\s+\w+\s+{name}\s*=\s*([^;]+);", text).group(1)
    return int(eval(expr, {"__builtins__": {}}, {"kScanWaves": S.SCAN_WAVES}))


def test_constants_match_the_sources():
    exact, host = _source("exact.hip.h"), _source("sknnr_hip.hip")
    assert _const(exact, "kScanWaves") == S.SCAN_WAVES
    assert _const(exact, "kScanRefs") == S.SCAN_REFS
    assert _const(exact, "kScanColChunk") == S.COL_CHUNK
    assert _const(exact, "kScanSliceMaxKK") == S.SLICE_MAX_KK
    assert _const(exact, "kScanMaxSlices") == S.MAX_SLICES
    assert _const(host, "kScanGridWg") == S.GRID_WG
    assert _const(host, "kScanMaxKK") == S.MAX_KK
    # the bound: once in launch_scan, once in the shard merge's replay, both 150 KiB on scan_block_bytes
    assert len(re.findall(r"if \(sh > kLdsLimit\)", host)) == 2 and _const(host, "kLdsLimit") == S.LDS_LIMIT
    assert host.count(S.REFUSAL) == 2
    qpw = re.search(r"constexpr int scan_qpw\(int formula\) \{ return formula == 0 \? (\d+) : (\d+); \}", exact)
    assert [int(qpw.group(1)), int(qpw.group(2)), int(qpw.group(2))] == [S.scan_qpw(f) for f in G.FORMULAS]
    assert re.search(r"constexpr int scan_nq\(int formula\) \{ return kScanWaves \* scan_qpw\(formula\); \}", exact)
    assert [S.scan_nq(f) for f in G.FORMULAS] == [12, 8, 8]
    assert re.search(r"const bool chunked = s\.d > kScanColChunk;", host) and re.search(r"const bool chunked = call\.d > kScanColChunk;", host)
    assert re.search(r"n_shards < 1 \|\| n_shards > (\d+)", host).group(1) == str(S.MAX_SHARDS)


def test_layout_by_hand():
    """scan_layout at one shape, added up by hand: 12 queries, d = 129 (dpad 130), kk = 5 (kkp 6, stack 14)."""
    L = S.scan_layout(129, 5, 12)
    assert (L["dpad"], L["kkp"], L["stk"]) == (130, 6, 14)
    assert (L["xs"], L["qn"], L["hv"], L["hi"], L["stack"]) == (0, 12480, 12576, 13056, 13344)
    assert L["d2"] == 14016 and L["total"] == 14016 + 8 * 12 * 512 == S.scan_block_bytes(129, 5, S.EXPANDED)
    assert S.scan_layout(1025, 5, 8)["dpad"] == S.scan_layout(1024, 5, 8)["dpad"] == 1024  # a chunk is the widest image


def test_slices_and_bounds():
    assert [S.scan_slices(n, 12, 13000, 32) for n in (1, 6144, 6145)] == [26, 2, 1]
    assert [S.scan_slices(n, 8, 13000, 32) for n in (4096, 4097)] == [2, 1]
    assert S.scan_slices(12, 12, 16385, 32) == 32 and S.scan_slices(12, 12, 16385, 33) == 1  # capped at 32; kk = 33 stops it
    assert S.scan_slices(40, 12, 512, 5) == 1 and S.scan_slices(40, 12, 513, 5) == 2  # at most one slice per step
    assert S.scan_slices(0, 12, 13000, 5) == 1
    assert S.slice_bounds(513, 2) == [(0, 512), (512, 513)]
    assert S.slice_bounds(1025, 3) == [(0, 512), (512, 1024), (1024, 1025)]
    b = S.slice_bounds(16385, 32)
    assert b[0] == (0, 512) and b[-1] == (15872, 16385) and [hi - lo for lo, hi in b].count(512) == 31
    for n_ref, n in ((1500, 3), (13000, 10), (13000, 26), (16385, 32)):
        b = S.slice_bounds(n_ref, n)
        assert b[0][0] == 0 and b[-1][1] == n_ref and all(x[1] == y[0] for x, y in zip(b, b[1:])) and all(lo < hi for lo, hi in b)


def test_coverage_table_is_what_the_restatement_gives():
    """Each named case is the launch its name says: formula, chunked flag, S, workgroups and LDS bytes."""
    assert list(G.COVERAGE) == list(G.CASES)
    for name, c in G.CASES.items():
        rec = S.expected_scan(c.formula, c.n_ref, c.d, c.kk, c.rows)
        assert G.COVERAGE[name] == (c.formula, rec["chunked"], rec["slices"], rec["workgroups"], rec["lds_bytes"]), name
        assert name.startswith(S.FORMULA_NAMES[c.formula] + "/")
        # the route: no pre-filter serves the call
        assert {"d>128": c.d > 128, "kk>31": c.kk > 31 and c.formula != S.HAMMING, "ids": c.formula == S.HAMMING}[c.route], name
        if c.formula == S.HAMMING:
            ref, _ = G.reference_rows(c.law, c.n_ref, c.d)
            assert (ref != np.floor(ref)).all()  # no 16-bit image of these ids: the integer path is off
        assert c.kk <= min(c.n_ref, S.MAX_KK)


# what makes a case the edge it is tagged with, in terms of the restated launch: (case, its given-rows record) -> bool
EDGES = {
    "odd_d_below_8": lambda c, r: c.d < 8 and c.d % 2 == 1,
    "last_unchunked": lambda c, r: c.d == S.COL_CHUNK and not r["chunked"] and S.scan_layout(c.d, c.kk, 8)["dpad"] == c.d,
    "chunk_of_one_column": lambda c, r: r["chunked"] and c.d - S.COL_CHUNK == 1,
    "two_full_chunks": lambda c, r: r["chunked"] and c.d == 2 * S.COL_CHUNK,
    "two_chunks_and_one_column": lambda c, r: r["chunked"] and c.d == 2 * S.COL_CHUNK + 1,
    "sliced": lambda c, r: r["slices"] > 1,
    "unsliced": lambda c, r: r["slices"] == 1 and c.rows > 512 * S.scan_nq(c.formula) and S.may_slice(c.formula, c.n_ref, c.kk),
    "quicksort_n1": lambda c, r: c.kk == 1,
    "quicksort_n2": lambda c, r: c.kk == 2,
    "quicksort_n3": lambda c, r: c.kk == 3,
    "last_sliced_kk": lambda c, r: c.kk == S.SLICE_MAX_KK and r["slices"] > 1,
    "slicing_stops": lambda c, r: c.kk == S.SLICE_MAX_KK + 1 and r["slices"] == 1 and r["workgroups"] < S.GRID_WG,
    "max_kk": lambda c, r: c.kk == S.MAX_KK,  # (and 191 as X=None: the same case's other variant)
    "lds_largest_accepted": lambda c, r: S.lds_boundary(c.d, c.formula)[0] == c.kk,
    "max_kk_fits": lambda c, r: c.kk == S.MAX_KK and S.fits(c.d, c.kk, c.formula),
    "n_ref_is_kk": lambda c, r: c.n_ref == c.kk,
    "one_step_short": lambda c, r: c.n_ref == S.SCAN_REFS - 1 and r["slices"] == 1 and r["workgroups"] == 1,
    "one_step": lambda c, r: c.n_ref == S.SCAN_REFS and r["slices"] == 1 and r["workgroups"] == 1,
    "slice_of_one_row": lambda c, r: S.slice_bounds(c.n_ref, r["slices"])[-1] == (512, 513),
    "last_slice_mostly_padding": lambda c, r: r["slices"] == 3 and S.slice_bounds(c.n_ref, 3)[-1] == (1024, 1025),
    "slices_capped_at_32": lambda c, r: r["slices"] == S.MAX_SLICES < S.n_steps(c.n_ref) and S.GRID_WG // 1 > S.MAX_SLICES,
    "uneven_last_slice": lambda c, r: len({hi - lo for lo, hi in S.slice_bounds(c.n_ref, r["slices"])}) > 1,
    "one_row_padding_slots": lambda c, r: c.rows == 1,
    "partial_pass": lambda c, r: c.rows == S.scan_nq(c.formula) - 1,
    "idle_workgroups": lambda c, r: r["slices"] > 1 and S.GRID_WG % r["slices"] != 0
    and -(-c.rows // S.scan_nq(c.formula)) * r["slices"] < S.GRID_WG,
    "last_sliced_count": lambda c, r: r["slices"] == 2 and S.scan_slices(c.rows + 1, S.scan_nq(c.formula), c.n_ref, c.kk) == 1,
    "first_unsliced_count": lambda c, r: r["slices"] == 1 and S.scan_slices(c.rows - 1, S.scan_nq(c.formula), c.n_ref, c.kk) == 2,
    "second_pass": lambda c, r: r["slices"] == 1 and S.GRID_WG * S.scan_nq(c.formula) < c.rows < 2 * S.GRID_WG * S.scan_nq(c.formula)
    and r["workgroups"] == S.GRID_WG,
}
# edges the chunked expanded formula alone has: qn from global memory, the fma chain across load_chunk calls
PER_FORMULA = ("odd_d_below_8", "last_unchunked", "chunk_of_one_column", "two_full_chunks", "two_chunks_and_one_column", "sliced",
               "unsliced", "quicksort_n1", "quicksort_n2", "quicksort_n3", "last_sliced_kk", "slicing_stops", "max_kk",
               "lds_largest_accepted", "n_ref_is_kk", "one_step_short", "one_step", "slice_of_one_row",
               "last_slice_mostly_padding", "slices_capped_at_32", "uneven_last_slice", "one_row_padding_slots", "partial_pass",
               "idle_workgroups", "last_sliced_count", "first_unsliced_count", "second_pass")


def test_every_edge_is_in_the_table():
    """Every tag holds for the case that carries it, and every edge is launched under each of the three formulas."""
    seen = {f: set() for f in G.FORMULAS}
    for name, c in G.CASES.items():
        rec = S.expected_scan(c.formula, c.n_ref, c.d, c.kk, c.rows)
        for edge in c.edges:
            assert EDGES[edge](c, rec), (name, edge)
            seen[c.formula].add(edge)
    assert set(PER_FORMULA) | {"max_kk_fits"} == set(EDGES)
    for f in G.FORMULAS:
        assert seen[f] >= set(PER_FORMULA), (f, set(PER_FORMULA) - seen[f])
    assert "max_kk_fits" in seen[S.DIRECT] and "max_kk_fits" in seen[S.HAMMING] and "max_kk_fits" not in seen[S.EXPANDED]
    for group, values, field in (("width", G.WIDTHS, "d"), ("kk", G.KKS, "kk"), ("nref", G.NREFS, "n_ref"), ("lds", G.LDS_WIDTHS, "d")):
        for f in G.FORMULAS:
            got = {getattr(c, field) for n, c in G.CASES.items() if f"/{group}/" in n and c.formula == f}
            assert got == set(values), (group, f)
    # the X=None variant of the kk = 192 cases asks for 191 neighbours, the most validate_call lets through
    assert all(G.variants(c)[-1] == (True, False) for n, c in G.CASES.items() if c.kk == S.MAX_KK)
    # every law of the kk group, and a window of rows inside the index for every case
    assert {c.law for n, c in G.CASES.items() if "/kk/" in n} == set(G.LAWS)
    assert all(1 <= G.self_window(c)[1] and sum(G.self_window(c)) <= c.n_ref and G.self_window(c)[0] > 0 for c in G.CASES.values())


def test_lds_boundary_is_derived():
    """The largest kk that fits 150 KiB and the first that does not, from the layout: expanded calls (12 queries a pass)
    stop at 34 / 24 / 24 for d = 1000 / 1024 / 1025 (a chunk is 1,024 columns wide, so 1,025 costs what 1,024 does); direct
    and Hamming calls (8 a pass) fit kScanMaxKK = 192 at every width."""
    got = {(f, d): S.lds_boundary(d, f) for f in G.FORMULAS for d in G.LDS_WIDTHS}
    assert [got[S.EXPANDED, d] for d in G.LDS_WIDTHS] == [(34, 35), (24, 25), (24, 25)]
    assert all(got[f, d] == (S.MAX_KK, None) for f in (S.DIRECT, S.HAMMING) for d in G.LDS_WIDTHS)
    assert all(S.fits(d, S.MAX_KK, f) for f in (S.DIRECT, S.HAMMING) for d in (1, 1024, 4096, 100_000))
    assert (S.scan_block_bytes(1000, 34, S.EXPANDED), S.scan_block_bytes(1000, 35, S.EXPANDED)) == (153_600, 153_888)
    assert (S.scan_block_bytes(1024, 24, S.EXPANDED), S.scan_block_bytes(1024, 25, S.EXPANDED)) == (153_504, 153_792)
    for (f, d), (ok, refused) in got.items():
        name = f"{S.FORMULA_NAMES[f]}/lds/d{d}-accepted"
        assert G.CASES[name].kk == ok and G.COVERAGE[name][4] == S.scan_block_bytes(d, ok, f) <= S.LDS_LIMIT
        assert refused is None or S.scan_block_bytes(d, refused, f) > S.LDS_LIMIT
    assert G.lds_refusals() == [(S.EXPANDED, 1000, 35), (S.EXPANDED, 1024, 25), (S.EXPANDED, 1025, 25)]


@functools.lru_cache(maxsize=None)
def _oracle_self(law, n_ref, d, formula, k):
    """oracle.kneighbors / oracle.kneighbors_hamming with X=None over the whole index (shared by the cases of a data set)."""
    from oracle import oracle as O

    ref, w = G.reference_rows(law, n_ref, d)
    if formula == S.HAMMING:
        return O.kneighbors_hamming(ref, None, w, k)
    return O.kneighbors(ref, None, k, S.FORMULA_NAMES[formula])


# (law, kk, X=None, deterministic) of the sliced variants on the lattice and duplicate laws that the oracle's rule replays
# whole: without the deterministic order any two equal kept values send a row on, and on these laws 32 kept rows always
# hold such a pair.  The answers of these two variants (of 28) say nothing about the merge; the other variants of the same
# cases, and their replay counts, do.
ALL_REPLAY = {("lattice", 32, True, False), ("dup", 32, False, False)}

SLICED = [n for n, c in G.CASES.items() if G.COVERAGE[n][2] > 1 or G.call_slices(c, True) > 1]


@pytest.mark.parametrize("name", SLICED)
def test_slice_merge_on_the_cpu_equals_the_oracle(record_property, name):
    """Every sliced call of the table: the slices' candidates merged as shards give oracle.kneighbors bit for bit (the
    function itself for the deterministic calls, its parts -- argkmin, drop_self -- for the others), and the replay count
    obeys the law's bounds."""
    from oracle import oracle as O

    c = G.CASES[name]
    ref, w = G.reference_rows(c.law, c.n_ref, c.d)
    for self_rows, det in G.variants(c):
        if G.call_slices(c, self_rows) <= 1:
            continue
        md, mi, n_replay = G.merged(c, self_rows, det)
        record_property(f"replays (X=None {self_rows}, deterministic {det})", n_replay)
        wd, wi = G.want(c, self_rows, det)
        np.testing.assert_array_equal(mi, wi)
        np.testing.assert_array_equal(md, wd)
        off, rows = G.self_window(c) if self_rows else (G.ROW_OFFSET, c.rows)
        if det:  # (the composition in want() is the oracle's own function)
            if self_rows:
                od, oi = _oracle_self(c.law, c.n_ref, c.d, c.formula, c.kk - 1)
                od, oi = od[off:off + rows], oi[off:off + rows]
            elif c.formula == S.HAMMING:
                od, oi = O.kneighbors_hamming(ref, G.query_rows(c.law, c.n_ref, c.d, c.rows), w, c.kk, row_offset=off)
            else:
                od, oi = O.kneighbors(ref, G.query_rows(c.law, c.n_ref, c.d, c.rows), c.kk, S.FORMULA_NAMES[c.formula], row_offset=off)
            np.testing.assert_array_equal(wi, oi)
            np.testing.assert_array_equal(wd, od)
        if c.formula != S.EXPANDED:
            assert n_replay == 0  # (distance, index) order: the union of the slices' lists is always the answer
        elif c.kk == 1:
            assert n_replay == rows  # the slice that holds the nearest row is full and ends at it: see the module docstring
        elif c.law == "smooth":
            # no ties: the one clause that fires is "a full slice ends at the k-th value", that is, all kk nearest rows
            # (the row itself included for X=None) lie in one slice -- never with many slices and kk = 32
            _, ni = G._argkmin(c.law, c.n_ref, c.d, c.rows, c.formula, c.kk, G.self_window(c) if self_rows else None)
            starts = [lo for lo, _ in S.slice_bounds(c.n_ref, G.call_slices(c, self_rows))]
            sid = np.searchsorted(starts, ni, side="right")
            assert n_replay == int((sid == sid[:, :1]).all(axis=1).sum()), (self_rows, det, n_replay)
            if c.kk == S.SLICE_MAX_KK and G.call_slices(c, self_rows) >= 10:
                assert n_replay == 0
        elif (c.law, c.kk, self_rows, det) in ALL_REPLAY:
            assert n_replay == rows, (n_replay, rows)
        else:  # lattice and dup, kk >= 2, every variant
            assert 0 < n_replay < rows, (self_rows, det, n_replay, rows)


def test_shard_merge_problem_has_ties_across_shards():
    """The shard-merge test's rows: under the expanded formula some rows are replayed and some are not at kk = 32; at
    kk = 1 every row is (the module docstring's finding)."""
    ref, _ = G.reference_rows("lattice", G.SHARD_ROWS, G.SHARD_D)
    q = G.query_rows("lattice", G.SHARD_ROWS, G.SHARD_D, G.SHARD_QUERIES)
    for n_shards in (2, 7, 64):
        for kk in (1, 32):
            n = S.merge_slices(ref, q, kk, S.EXPANDED, G.shard_bounds_of(n_shards), True, row_offset=G.ROW_OFFSET)[2]
            assert (n == G.SHARD_QUERIES) if kk == 1 else (0 < n < G.SHARD_QUERIES), (n_shards, kk, n)
