"""The plan a search call works out before its first launch (plan_search in sknnr_amd/csrc/sknnr_hip.hip, through
sknnr_debug_search_plan: no handle, no device) against the Python restatements of the dispatch rules that the GPU instance
tests rely on: tests/_prefilter_dispatch.py (which pre-filter, which lists), tests/_finalize_record.py (the record path)
and tests/_hamming_dispatch.py (the envelope of the integer Hamming pre-filter).

One sweep, shared by the tests: a few thousand ctypes calls.
"""

from __future__ import annotations

import numpy as np
import pytest

import _finalize_record as R
import _hamming_dispatch as H
import _prefilter_dispatch as P

DIMS = (8, 16, 32, 48, 64, 80, 128, 129)
KKS = range(1, 34)
DEPTHS = (0, 3)
NQ = 1000


def n_refs(d: int) -> tuple[int, ...]:
    lo = P.min_coarse2_n_ref(P.ks_of(d))
    return (1000, lo - 1, lo, 50_000, 1 << 20)


@pytest.fixture(scope="module")
def native():
    from sknnr_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="module")
def sweep(native):
    """{(n_ref, d, kk, depth): plan} over the whole grid, Euclidean calls on given rows."""
    return {(n_ref, d, kk, depth): native.debug_search_plan(n_ref, d, kk, NQ, cell_depth=depth)
            for d in DIMS for n_ref in n_refs(d) for kk in KKS for depth in DEPTHS}


def test_grid_is_the_one_asked_for(sweep):
    assert len(sweep) == 5 * len(DIMS) * 33 * 2
    assert all(P.use_coarse2(n_refs(d)[2], d, 6) and not P.use_coarse2(n_refs(d)[1], d, 6) for d in DIMS if d <= 64)


def test_plan_matches_the_restated_prefilter_dispatch(sweep):
    for (n_ref, d, kk, depth), plan in sweep.items():
        want = P.expected_launch(n_ref, d, kk, NQ, depth=depth)
        got = {f: plan[f] for f in ("generation", "m_list", "rank_extra", "cell_depth")}
        assert got == {f: want[f] for f in got}, (n_ref, d, kk, depth)
        assert plan["kk"] == kk and plan["ks"] == want["ks"]


def test_plan_reaches_exactly_the_reachable_instances(sweep):
    reached = {(p["ks"], p["m_list"], p["rank_extra"]) for p in sweep.values() if p["generation"] == 2}
    assert sorted(reached) == P.reachable_instances()


def test_record_path_matches_its_restatement(native, sweep):
    for (n_ref, d, kk, depth), plan in sweep.items():
        launch = P.expected_launch(n_ref, d, kk, NQ, depth=depth)
        assert bool(plan["record"]) == R.uses_record(launch, kk), (n_ref, d, kk, depth)
    # shard candidates (raw) never take it
    for (n_ref, d, kk, depth) in list(sweep)[:: 7]:
        assert native.debug_search_plan(n_ref, d, kk, NQ, cell_depth=depth, raw=True)["record"] == 0


def test_integer_hamming_envelope_matches_its_restatement(native):
    ok_ids, bad_ids = np.zeros((4, 3)), np.full((4, 3), 0.5)
    assert H.h16_ok(ok_ids) and not H.h16_ok(bad_ids)
    for kk in KKS:
        for ids in (ok_ids, bad_ids):
            plan = native.debug_search_plan(1000, 3, kk, NQ, formula=native.FORMULA_HAMMING, h16_ok=H.h16_ok(ids))
            assert plan["generation"] == 0, "no Euclidean pre-filter on a Hamming call"
            assert bool(plan["ham_int"]) == H.ham_int(ids, kk), kk
    # ... and never on a Euclidean call
    assert native.debug_search_plan(1000, 3, 5, NQ, h16_ok=True)["ham_int"] == 0
