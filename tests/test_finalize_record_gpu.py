"""finalize_record_kernel (8 lanes per query on the merged candidate record that coarse2_kernel's epilogue files) pinned
bit for bit to the oracle, and the dispatch around it.

Every call names the pre-filter launch it expects (tests/_prefilter_dispatch.py) and whether the finaliser must have run
on records (tests/_finalize_record.py, uses_record); ``Index.debug_last_finalize()`` must report exactly that.  Indices
and float64 distances are compared with ``oracle.kneighbors`` with assert_array_equal.  The share of rows handed to the
exact scan on the synthetic law is held to the bound the existing instance tests use for lists with sentinels
(tests/test_prefilter_instances_gpu.py, FALLBACK_MAX).

4,500 reference rows (enough for the second-generation kernel at every width here); thin-only calls have 6,144 rows,
the bulk + thin call 270,000 (264 workgroups of 16 waves: 256 bulk, 8 thin).  Cells forced on (SKNNR_CELLS=6: bucketed
order) and off (SKNNR_CELLS=0: plain order).
"""

from __future__ import annotations

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _finalize_record as R
import _prefilter_dispatch as P

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REF = 4_500
NQ_THIN = 6_144
NQ_BOTH = 270_000
ROW_OFFSET = 1_000
FALLBACK_MAX = 0.05
WIDTHS = (8, 16, 32, 64)


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def handles(N):
    made = {}

    def get(key, ref, **env):
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                for name, value in env.items():
                    mp.setenv(name, str(value))
                made[key] = N.Index(ref)
        return made[key]

    yield get
    for ix in made.values():
        ix.close()


@functools.lru_cache(maxsize=4)
def _problem(d, nq=NQ_THIN, n_ref=N_REF):
    from sknnr_amd import synth

    x_ref, _, x_q = synth.make_problem(n_ref, nq, d, t=1, n_dup_refs=24, n_dup_queries=16)
    return x_ref, x_q


def _call(ix, q, k, formula=0, nq=None, row_offset=None):
    """(dist, idx, pre-filter record, finaliser record, rows sent to the exact scan) of one call on fresh statistics."""
    exclude_self = q is None
    if row_offset is None:
        row_offset = 0 if exclude_self else ROW_OFFSET
    ix.reset_stats()
    dist, idx = ix.kneighbors_host(q, ix.make_opts(k, exclude_self=exclude_self, row_offset=row_offset, formula=formula), nq=nq)
    st = ix.stats()
    assert st["queries"] == len(idx) and st["exact_only_queries"] == 0, st
    return dist, idx, ix.debug_last_prefilter(), ix.debug_last_finalize(), st["exact_fallbacks"]


def _expect_finalize(launch, kk, raw=False):
    rec = R.uses_record(launch, kk, raw)
    lanes = R.RECORD_LEN if rec else (16 if launch["m_list"] <= 8 else (32 if launch["m_list"] <= 16 else 64))
    return rec, lanes


def _check(got, want, launch, kk, what, fallback_max=FALLBACK_MAX):
    dist, idx, pre, fin, fallbacks = got
    od, oi = want
    assert pre == launch, f"{what}: launched {pre}, dispatch says {launch}"
    rec, lanes = _expect_finalize(launch, kk)
    assert (fin["record"], fin["lanes_per_query"]) == (int(rec), lanes), f"{what}: finaliser {fin}"
    assert fin["truncated_rows"] <= fallbacks and (rec or fin["truncated_rows"] == 0), f"{what}: {fin}, {fallbacks} fall-backs"
    np.testing.assert_array_equal(idx, oi, err_msg=what)
    np.testing.assert_array_equal(dist, od, err_msg=what)
    if fallback_max is not None:
        share = fallbacks / len(idx)
        print(f"{what}: fall-back share {share:.4%}, truncated {fin['truncated_rows']}")
        assert share <= fallback_max, f"{what}: {share:.2%} of the rows went to the exact scan"
    return fin


@gpu
@pytest.mark.parametrize("cells", (6, 0))
@pytest.mark.parametrize("formula", ("expanded", "direct"))
@pytest.mark.parametrize("d", WIDTHS)
def test_thin_calls_k1_to_6(N, O, handles, d, formula, cells):
    """k = 1 .. 6, X given and X=None, thin-only calls: up to 32 features every call that searches at most 5 neighbours runs
    on records (lists of 2 and 6; 6 and 7 neighbours are on lists of 8); 64 features (four K-steps) keep the lists."""
    ref, q = _problem(d)
    ix = handles((d, cells), ref, SKNNR_CELLS=cells)
    code = {"expanded": N.FORMULA_EXPANDED, "direct": N.FORMULA_DIRECT}[formula]
    served = 0
    for k in range(1, 7):
        launch = P.expected_launch(N_REF, d, k, NQ_THIN, cells_env=cells)
        fin = _check(_call(ix, q, k, code), O.kneighbors(ref, q, k, formula, row_offset=ROW_OFFSET), launch, k,
                     f"d={d} {formula} cells={cells} k={k}")
        served += fin["record"]
        launch = P.expected_launch(N_REF, d, k + 1, N_REF, cells_env=cells)
        fin = _check(_call(ix, None, k, code, nq=N_REF), O.kneighbors(ref, None, k, formula), launch, k + 1,
                     f"d={d} {formula} cells={cells} k={k} X=None")
        served += fin["record"]
    assert served == (9 if d <= 32 else 0)  # (of 12 calls: k <= 5 on given rows, k <= 4 for X=None)


@gpu
@pytest.mark.parametrize("cells,k", ((6, 5), (0, 3)))
def test_bulk_and_thin_launch(N, O, handles, cells, k):
    """One call whose rows are split between the 16-wave bulk launch (finalised on the side stream) and the thin launch."""
    d = 32
    ref, q = _problem(d, NQ_BOTH)
    ix = handles((d, cells), _problem(d)[0], SKNNR_CELLS=cells)
    launch = P.expected_launch(N_REF, d, k, NQ_BOTH, cells_env=cells)
    assert launch["bulk_rows"] > 0 and launch["thin_rows"] > 0
    fin = _check(_call(ix, q, k), O.kneighbors(ref, q, k, "expanded", row_offset=ROW_OFFSET), launch, k, f"bulk + thin cells={cells}")
    assert fin["record"] == 1


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
from sknnr_amd import _native as N, synth
ref, _, q = synth.make_problem({n_ref}, {nq}, 32, t=1, n_dup_refs=24, n_dup_queries=16)
ix = N.Index(ref)
dist, idx = ix.kneighbors_host(q, ix.make_opts(5, row_offset=0))
fin = ix.debug_last_finalize(); pre = ix.debug_last_prefilter()
np.savez(sys.argv[1], dist=dist, idx=idx, record=fin["record"], rows=pre["bulk_rows"] + pre["thin_rows"])
ix.close()
"""


@gpu
@pytest.mark.parametrize("cells", (6, 0))
def test_two_chunks(N, O, tmp_path, cells):
    """SKNNR_CHUNK_ROWS is read once per process: a child runs 10,000 rows in chunks of 6,144 (the record workspace is
    reused by the second chunk, whose rows start at call row 6,144)."""
    nq = 10_000
    out = tmp_path / "two_chunks.npz"
    env = dict(os.environ, SKNNR_CHUNK_ROWS="6144", SKNNR_CELLS=str(cells))
    run = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, n_ref=N_REF, nq=nq), str(out)], env=env,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)
    assert int(got["record"]) == 1 and int(got["rows"]) < nq  # (the record describes the LAST chunk: fewer rows than the call)
    ref, q = _problem(32, nq)
    od, oi = O.kneighbors(ref, q, 5, "expanded")
    np.testing.assert_array_equal(got["idx"], oi)
    np.testing.assert_array_equal(got["dist"], od)


@gpu
def test_row_offset_and_out(N, O):
    """X=None on a window of the reference rows (row_offset) and the engine's out= / row_offset on device tensors."""
    import torch

    from sknnr_amd._engine import KNNEngine

    ref, q = _problem(32)
    ix = N.Index(ref)
    k, lo, n = 4, 1_500, 2_000
    dist, idx, _, fin, _ = _call(ix, None, k, nq=n, row_offset=lo)
    od, oi = O.kneighbors(ref, None, k, "expanded")
    assert fin["record"] == 1 and fin["lanes_per_query"] == 8
    np.testing.assert_array_equal(idx, oi[lo:lo + n])
    np.testing.assert_array_equal(dist, od[lo:lo + n])
    ix.close()
    eng = KNNEngine(ref)
    xq = torch.as_tensor(q, device="cuda")
    big_d = torch.full((3 * NQ_THIN, k), -1.0, dtype=torch.float64, device="cuda")
    big_i = torch.full((3 * NQ_THIN, k), -1, dtype=torch.int64, device="cuda")
    eng.kneighbors(xq, k, row_offset=700, out=(big_d[NQ_THIN:2 * NQ_THIN], big_i[NQ_THIN:2 * NQ_THIN]))
    fin = eng._index.debug_last_finalize()
    assert fin["record"] == 1 and fin["lanes_per_query"] == 8
    od, oi = O.kneighbors(ref, q, k, "expanded", row_offset=700)
    np.testing.assert_array_equal(big_i[NQ_THIN:2 * NQ_THIN].cpu().numpy(), oi)
    np.testing.assert_array_equal(big_d[NQ_THIN:2 * NQ_THIN].cpu().numpy(), od)
    assert (big_i[:NQ_THIN] == -1).all() and (big_i[2 * NQ_THIN:] == -1).all()
    eng.close()


@gpu
@pytest.mark.parametrize("cells", (6, 0))
def test_ties_and_duplicates_reach_the_exact_scan(N, O, cells, monkeypatch):
    """An integer lattice (many exactly tied pre-filter values: the record's last entry lies inside the window, so the
    truncation rule must be SEEN to fire) and reference rows repeated twelve times (more hits in one unit than a lane's
    queue holds: poisoned queries, whose bound is NaN, must be seen to reach the exact scan).  Answers stay bit for bit."""
    monkeypatch.setenv("SKNNR_CELLS", str(cells))
    rng = np.random.default_rng(5)
    d = 16
    ref = rng.integers(0, 3, size=(N_REF, d)).astype(np.float64)
    q = rng.integers(0, 3, size=(NQ_THIN, d)).astype(np.float64)
    ix = N.Index(ref)
    for k in (1, 5):
        launch = P.expected_launch(N_REF, d, k, NQ_THIN, cells_env=cells)
        got = _call(ix, q, k)
        fin = _check(got, O.kneighbors(ref, q, k, "expanded", row_offset=ROW_OFFSET), launch, k, f"lattice k={k}", fallback_max=None)
        assert fin["record"] == 1
        if k == 5:
            assert fin["truncated_rows"] > 0, "the truncation rule never fired on a lattice"
    ix.close()
    ref, q = (a.copy() for a in _problem(32))
    ref[600:1200] = np.repeat(ref[:50], 12, axis=0)
    q[:600] = ref[600:1200] + 1e-9
    ix = N.Index(ref)
    for k in (1, 5):
        launch = P.expected_launch(N_REF, 32, k, NQ_THIN, cells_env=cells)
        got = _call(ix, q, k)
        fin = _check(got, O.kneighbors(ref, q, k, "expanded", row_offset=ROW_OFFSET), launch, k, f"duplicates k={k}", fallback_max=None)
        assert fin["record"] == 1 and got[4] > 0, "no duplicated row reached the exact scan"
    ix.close()


@gpu
def test_other_calls_keep_the_lists(N, O):
    """k = 10 (pooled rank), raw shard candidates and a reference set too small for the second-generation kernel keep the
    two lists and finalize_kernel."""
    ref, q = _problem(32)
    ix = N.Index(ref)
    got = _call(ix, q, 10)
    launch = P.expected_launch(N_REF, 32, 10, NQ_THIN, depth=got[2]["cell_depth"])  # (default order: the index build's choice)
    assert launch["rank_extra"] > 0
    fin = _check(got, O.kneighbors(ref, q, 10, "expanded", row_offset=ROW_OFFSET), launch, 10, "k=10", fallback_max=None)
    assert (fin["record"], fin["lanes_per_query"]) == (0, 16)
    # the same handle serves k = 5 on records and a shard call of 5 candidates on the lists
    got = _call(ix, q, 5)
    assert got[3]["record"] == 1
    val, sidx = ix.shard_candidates_host(q, ix.make_opts(5), index_offset=7)
    fin = ix.debug_last_finalize()
    assert (fin["record"], fin["lanes_per_query"], fin["truncated_rows"]) == (0, 16, 0)
    ov, oi = O.shard_candidates(ref, q, 5, "expanded", index_offset=7)
    np.testing.assert_array_equal(sidx, oi)
    np.testing.assert_array_equal(val, ov)
    ix.close()
    small = 3_000
    ref, q = _problem(32, NQ_THIN, small)
    ix = N.Index(ref)
    launch = P.expected_launch(small, 32, 5, NQ_THIN)
    assert launch["generation"] == 1
    fin = _check(_call(ix, q, 5), O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET), launch, 5, "3,000 reference rows")
    assert (fin["record"], fin["lanes_per_query"]) == (0, 16)
    ix.close()
