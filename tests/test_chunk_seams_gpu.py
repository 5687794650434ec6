"""Device-chunk seams of one search call: what the host code in sknnr_amd/csrc/sknnr_hip.hip re-bases at ``c0``, the first
row of a chunk, pinned to the oracle on calls that cross a seam.

Every stage is pinned at kernel level elsewhere; a wrong offset in the loops that cut a call into chunks gives wrong
neighbours only behind the first seam, on calls larger than any other test makes.  ``SKNNR_CHUNK_ROWS`` is read once per
process, so the calls run in three child processes (this file, run as a script), one after the other; each writes one
``.npz`` and the parent compares every ``idx`` and ``dist`` with ``oracle/oracle.py`` by assert_array_equal.  A child that
exits non-zero fails its test with the end of its stderr; nothing is retried.

Child A (``SKNNR_CHUNK_ROWS=6144``, ``SKNNR_CELLS=0``) and child B (the same with ``SKNNR_CELLS=6``: bucketed order,
``finalize_rows`` by positions, ``qperm`` per chunk) use one handle of 14,000 x 32 reference rows
(``synth.make_problem`` with duplicated rows, 600 rows replaced by twelve copies each of 50 rows) that also carries an
affine map 24 -> 32 with a centre, a scale and a projection.  Child C (default environment) queries a forest-mapped
handle: 5 trees of depth <= 6 on 4 features, 200 reference rows, 2^18 + 37 raw rows.

Where the cases differ from their first description, and why (read from the code, nothing here is a tolerance):

- Bulk AND thin launches in a 6,144-row chunk do not exist.  ``launch_coarse2`` gives a chunk a bulk launch only from
  257 workgroups on (16 waves: 263,168 rows); a 6,144-row chunk is 6 workgroups and all of it goes to the 4-wave thin
  launch (``_prefilter_dispatch.coarse2_split``).  The fork's join is therefore not reachable under this chunk size;
  what is asserted instead, for every row count of case 1, is that the LAST chunk launched exactly what
  ``expected_launch`` predicts for its live rows (1 row: one thin workgroup of 256).
- d = 160 with an affine map is refused by the library (``run_device``: "outside the HIP envelope"), and so are narrow
  rows at d > 128 (``validate_call``).  Both refusals are asserted.  The loop's ``prep_chunk``-only branch (``to_xt``
  without a coarse image pass) is reached with k = 32 on the affine handle instead: more than 31 neighbours take no
  pre-filter, the preparation kernel writes the transformed rows chunk by chunk and the exact scan answers every row.
- Node ids that the integer Hamming pass cannot hold cannot come out of a forest map (they are node numbers of the
  installed trees); the rows at 2^18 - 1, 2^18 and the last row hold raw values far outside the training range
  (+-8e37, +-0) instead, which end in the outermost leaves.
- With ``row_offset`` 1000 and 200 reference rows the order of tied neighbours does not depend on a row's position
  (every row lies behind every index), so a forest chunk that lost its ``c0`` would answer the same.  Child C makes one
  more call at ``row_offset`` 100, and the parent first shows on the CPU that the oracle's order behind the seam changes
  when the seam's 2^18 is left out of the base.
- ``debug_last_rescue`` is call-wide (the device words count over the chunks of a call), so its identities are asserted
  on the whole call.
- Child B builds four handles, not three: the merge runs on the main handle, the three shards need one each.

Wall time of the children on an MI355X, from ``subprocess.run`` to its return: A 3.8 s, B 4.2 s, C 3.7 s (1.6, 1.9 and
1.5 s of them in handles and calls, the rest imports); each test with the parent's oracle runs: 8.2, 8.8 and 7.5 s.

Teeth, measured on an MI355X with scratch builds of sknnr_hip.hip (never committed): ``oc.row_offset = o->row_offset``
in ``run_forest`` fails test_forest_map_across_a_seam (the call at row_offset 100, 19 indices behind the seam), and the
transformed rows of ``merge_shards_device`` written at ``xt`` without ``c0 * d`` fail test_bucketed_order_across_seams
(1,693 of 40,000 merged indices).  ``ra.row0 = 0`` was not run: the rescue kernel would then read the query image and
``qnc`` of chunk rows 6,144 .. 9,999 in buffers that hold 6,144 rows.
"""

from __future__ import annotations

import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

gpu = pytest.mark.gpu
CHUNK = 6_144                # SKNNR_CHUNK_ROWS of children A and B: kRowQuantum, the smallest chunk
N_REF, D, D_IN = 14_000, 32, 24
ROW_OFFSET = 1_000
COUNTS = (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)
NQ = 10_000
SELF_LO, SELF_NQ = 1_500, 2 * CHUNK + 1
TIE_ROWS = np.r_[100:150, 6_100:6_144, 6_144:6_200, 9_950:10_000]  # rows 6,143, 6,144 and 9,999 among them
NQ_XT, K_XT = 7_000, 32
NARROW = ("float64", "float32", "int16", "uint8")
N_SHARDS, K_SHARD = 3, 4
FOREST_CHUNK = 1 << 18
FOREST_NQ = FOREST_CHUNK + 37
FOREST_K = 4
FOREST_OFFSET_LOW = 100
NAN_MESSAGE = "Input X contains NaN"


# ---------------------------------------------------------------------------------------------------------------------
# inputs, built the same way by the parent and by the children
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _rows():
    """(reference rows, 12,289 query rows): make_problem's correlated features with its duplicated rows; reference rows
    600 .. 1,199 are twelve copies each of rows 0 .. 49 (exact ties across the k-th neighbour for the queries beside them)."""
    from sknnr_amd import synth

    ref, _, q = synth.make_problem(N_REF, 2 * CHUNK + 1, D, t=1, n_dup_refs=24, n_dup_queries=16)
    ref = ref.copy()
    ref[600:1200] = np.repeat(ref[:50], 12, axis=0)
    for a in (ref, q):
        a.setflags(write=False)
    return ref, q


@functools.lru_cache(maxsize=1)
def _tie_queries():
    """10,000 query rows; those of TIE_ROWS sit 1e-9 beside a reference row that exists at least thirteen times."""
    ref, q = _rows()
    q = q[:NQ].copy()
    q[TIE_ROWS] = ref[600:600 + len(TIE_ROWS)] + 1e-9
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=1)
def _affine():
    """(centre, scale, projection, raw rows): 10,000 x 24 integers in 0 .. 200, which float64, float32, int16 and uint8
    all hold exactly."""
    rng = np.random.default_rng(7)
    center = 100.0 + 10.0 * rng.standard_normal(D_IN)
    scale = 58.0 * rng.uniform(0.5, 2.0, D_IN)
    proj = rng.standard_normal((D_IN, D)) / np.sqrt(D_IN)
    raw = rng.integers(0, 201, (NQ, D_IN))
    return center, scale, proj, raw


@functools.lru_cache(maxsize=1)
def _wide():
    """300 x 160 reference rows and a projection 24 -> 160: outside the envelope of the preparation kernel."""
    rng = np.random.default_rng(8)
    return rng.standard_normal((300, 160)), rng.standard_normal((D_IN, 160)) / np.sqrt(D_IN)


def _forest_chunk_rows(n_trees):
    """forest_chunk_rows (sknnr_hip.hip): 2^18 rows or what 4 GiB of node ids hold, a multiple of kFtRows = 256."""
    return max(256, min(1 << 18, (4 << 30) // (8 * max(n_trees, 1))) // 256 * 256)


@functools.lru_cache(maxsize=1)
def _forest():
    """(fitted transformer, its 200 x 4 training rows, 1-D y, 2^18 + 37 raw float32 rows, tree weights)."""
    from sknnr_amd.transformers import RFNodeTransformer

    rng = np.random.default_rng(21)
    x = rng.normal(size=(200, 4))
    y = x @ np.array([1.0, -2.0, 0.5, 0.25]) + 0.3 * rng.normal(size=200)
    t = RFNodeTransformer(n_estimators=5, max_depth=6, random_state=0).fit(x, y)
    q = rng.normal(size=(FOREST_NQ, 4)).astype(np.float32)
    q[FOREST_CHUNK - 1] = 8e37
    q[FOREST_CHUNK] = -8e37
    q[FOREST_NQ - 1] = (0.0, -0.0, 8e37, -8e37)
    w = rng.random(5) + 0.05
    q.setflags(write=False)
    return t, x, y, q, w


# ---------------------------------------------------------------------------------------------------------------------
# the children
# ---------------------------------------------------------------------------------------------------------------------
def _refusal(call):
    """[code, message] of the library error ``call`` raises, [0, ""] when it raises none."""
    from sknnr_amd import _native as N

    try:
        call()
    except N.HipBackendError as e:
        return json.dumps([e.code, e.message])
    return json.dumps([0, ""])


def _child_euclid(out, plain_order):
    """Children A (``plain_order``: every case) and B (cases 1, 2, 4 and the shard round trip) on one handle."""
    from sknnr_amd import _native as N

    t0 = time.perf_counter()
    ref, q = _rows()
    center, scale, proj, raw = _affine()
    res = {}
    ix = N.Index(ref)
    ix.set_affine(D_IN, center, scale, proj)
    consts = ix.debug_image_constants()
    res["s"], res["mu"] = np.float64(consts["s"]), np.asarray(consts["mu"], dtype=np.float64)

    def call(name, rows, k, nq=None, **kw):
        ix.reset_stats()
        dist, idx = ix.kneighbors_host(rows, ix.make_opts(k, **kw), nq=nq)
        res[name + "_dist"], res[name + "_idx"] = dist, idx
        res[name + "_rec"] = json.dumps(dict(stats=ix.stats(), pre=ix.debug_last_prefilter(), prep=ix.debug_last_prep(),
                                             rescue=ix.debug_last_rescue(), scan=ix.debug_last_scan()))

    for n in COUNTS:
        call(f"counts{n}", q[:n], 5, row_offset=ROW_OFFSET)
    for formula, code in (("expanded", N.FORMULA_EXPANDED), ("direct", N.FORMULA_DIRECT)):
        call(f"self_{formula}", None, 4, nq=SELF_NQ, exclude_self=True, row_offset=SELF_LO, formula=code)
    call("ties", _tie_queries(), 5, row_offset=ROW_OFFSET)
    if plain_order:
        for name in NARROW:
            call(f"affine_{name}", raw.astype(name), 5, apply_affine=True, row_offset=ROW_OFFSET,
                 query_dtype=N.dtype_code(name))
        clean = q[:NQ]
        for name, cells in (("first", ((3, 5, np.nan),)), ("seam", ((CHUNK, 5, np.nan),)),
                            ("last", ((NQ - 1, 5, np.nan), (NQ - 1, 9, np.inf)))):
            bad = clean.copy()
            for r, c, v in cells:
                bad[r, c] = v
            res[f"nonfinite_{name}"] = _refusal(
                lambda: ix.kneighbors_host(bad, ix.make_opts(5, row_offset=ROW_OFFSET, check_finite=True)))
        call("after_nonfinite", clean, 5, row_offset=ROW_OFFSET, check_finite=True)
        call("xt_only", raw[:NQ_XT].astype(np.float32), K_XT, apply_affine=True, row_offset=ROW_OFFSET,
             query_dtype=N.dtype_code(np.float32))
        ref160, proj160 = _wide()
        wide = N.Index(ref160)
        wide.set_affine(D_IN, center, scale, proj160)
        res["wide_affine"] = _refusal(lambda: wide.kneighbors_host(
            raw[:NQ_XT].astype(np.float64), wide.make_opts(3, apply_affine=True)))
        res["wide_float32"] = _refusal(lambda: wide.kneighbors_host(
            ref160[:50].astype(np.float32), wide.make_opts(3, query_dtype=N.dtype_code(np.float32))))
        wide.close()
    else:
        from sknnr_amd.distributed import shard_bounds

        rows = raw.astype(np.float64)
        vals, idxs = [], []
        for g in range(N_SHARDS):
            a, b = shard_bounds(N_REF, N_SHARDS, g)
            shard = N.Index(ref[a:b])
            shard.set_affine(D_IN, center, scale, proj)
            v, i = shard.shard_candidates_host(rows, shard.make_opts(K_SHARD, deterministic=False, apply_affine=True),
                                               index_offset=a)
            shard.close()
            vals.append(v)
            idxs.append(i)
        res["shard_val"], res["shard_idx"] = np.stack(vals), np.stack(idxs)
        res["merge_dist"], res["merge_idx"] = ix.merge_shards_host(
            rows, ix.make_opts(K_SHARD, apply_affine=True, row_offset=ROW_OFFSET), res["shard_val"], res["shard_idx"])
    ix.close()
    res["wall"] = np.float64(time.perf_counter() - t0)
    np.savez(out, **res)


def _child_forest(out):
    """Child C: raw rows through the forest map, two forest chunks."""
    from sknnr_amd import _native as N

    t0 = time.perf_counter()
    t, x, y, q, w = _forest()
    image = t.forest_image()
    ix = N.Index(t.transform(x).astype(np.float64), y)
    ix.set_hamming_weights(w)
    ix.set_forest(image["d_in"], image["tree_offset"], image["threshold"], image["feature"], image["left"], image["right"])
    res = {}

    def opts(dtype, row_offset=ROW_OFFSET):
        return ix.make_opts(FOREST_K, formula=N.FORMULA_HAMMING, apply_affine=True, row_offset=row_offset,
                            check_finite=True, query_dtype=N.dtype_code(dtype))

    pred, res["f32_dist"], res["f32_idx"] = ix.predict_host(q, opts(np.float32), return_neighbors=True)
    res["f32_pred"] = pred
    res["hamming"] = json.dumps(ix.debug_last_hamming())
    res["f64_dist"], res["f64_idx"] = ix.kneighbors_host(q.astype(np.float64), opts(np.float64))
    res["low_dist"], res["low_idx"] = ix.kneighbors_host(q, opts(np.float32, FOREST_OFFSET_LOW))
    bad = q.copy()
    bad[FOREST_CHUNK + 1, 2] = np.nan
    res["nonfinite"] = _refusal(lambda: ix.kneighbors_host(bad, opts(np.float32)))
    res["after_dist"], res["after_idx"] = ix.kneighbors_host(q[:300], opts(np.float32))
    ix.close()
    res["wall"] = np.float64(time.perf_counter() - t0)
    np.savez(out, **res)


def _run_child(which, tmp_path, **env_set):
    out = tmp_path / f"seams_{which}.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("SKNNR_CHUNK_ROWS", "SKNNR_CELLS")}
    env.update(env_set)
    t0 = time.perf_counter()
    run = subprocess.run([sys.executable, os.path.abspath(__file__), which, str(out)], env=env, capture_output=True,
                         text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)
    print(f"child {which}: {wall:.1f} s, {float(got['wall']):.1f} s of them handles and calls")
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the parent's checks, one per case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def _equal(got, name, want, what=None):
    od, oi = want
    np.testing.assert_array_equal(got[name + "_idx"], oi, err_msg=what or name)
    np.testing.assert_array_equal(got[name + "_dist"], od, err_msg=what or name)


def _rec(got, name):
    return json.loads(str(got[name + "_rec"]))


@functools.lru_cache(maxsize=1)
def _want_counts():
    from oracle import oracle

    ref, q = _rows()
    return oracle.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET)


def _check_counts(got, cells):
    """Case 1, 6,144 / 6,145 / 12,288 / 12,289 given float64 rows, k = 5, row_offset 1000.  Pins ``pad_rows`` on the
    remainder (a last chunk of one row is padded by 6,143; one and two full chunks have no remainder), ``select_window``
    at ``c0`` (outputs at ``out + c0 * k``, the reorder's row at ``row_offset + c0``) and ``finalize_args``' ``fail_base``;
    bucketed (child B) also ``finalize_rows`` by positions on each chunk's own ``qperm``.  The last chunk's launch record
    must be what ``expected_launch`` says of its live rows: thin rows only (the module docstring says why)."""
    import _prefilter_dispatch as P

    od, oi = _want_counts()
    for n in COUNTS:
        _equal(got, f"counts{n}", (od[:n], oi[:n]))
        rest = n - (n - 1) // CHUNK * CHUNK
        rec = _rec(got, f"counts{n}")
        launch = P.expected_launch(N_REF, D, 5, rest, cells_env=cells)
        assert launch["generation"] == 2 and launch["bulk_rows"] == 0 and launch["thin_rows"] > 0, launch
        assert rec["pre"] == launch, f"{n} rows: the last chunk launched {rec['pre']}, dispatch says {launch}"
        assert (rec["prep"]["nq"], rec["prep"]["nq_pad"]) == (rest, CHUNK), rec["prep"]
        assert rec["stats"]["queries"] == n and rec["stats"]["exact_only_queries"] == 0, rec["stats"]
    first = got[f"counts{CHUNK}_idx"].tobytes(), got[f"counts{CHUNK}_dist"].tobytes()
    for n in COUNTS[1:]:
        assert (got[f"counts{n}_idx"][:CHUNK].tobytes(), got[f"counts{n}_dist"][:CHUNK].tobytes()) == first, n


def _check_self_rows(got, O):
    """Case 2, X=None on reference rows 1,500 .. 13,788 (two seams), k = 4, both formulas.  Pins the row's own index
    ``row_offset + c0 + r`` of exclude_self (``select_window``) and ``prep_chunk``'s ``call.xq + c0 * d`` on the handle's own
    rows."""
    ref, _ = _rows()
    own = np.arange(SELF_LO, SELF_LO + SELF_NQ)[:, None]
    for formula in ("expanded", "direct"):
        od, oi = O.kneighbors(ref, None, 4, formula)
        assert not (got[f"self_{formula}_idx"] == own).any(), f"{formula}: a row names itself"
        _equal(got, f"self_{formula}", (od[SELF_LO:SELF_LO + SELF_NQ], oi[SELF_LO:SELF_LO + SELF_NQ]))


def _check_narrow_affine(got, O, N):
    """Case 3, the same 10,000 raw rows as float64, float32, int16 and uint8 through the affine map (centre, scale and
    projection: all three prep bits), 24 -> 32.  Pins ``prep_chunk``'s stride ``c0 * d_x * dtype_bytes(x_dtype)`` on
    ``const void* xdev`` and its ``xt + c0 * d``."""
    ref, _ = _rows()
    center, scale, proj, raw = _affine()
    want = O.kneighbors(ref, O.affine(raw.astype(np.float64), center, scale, proj), 5, "expanded", row_offset=ROW_OFFSET)
    for name in NARROW:
        _equal(got, f"affine_{name}", want)
        prep = _rec(got, f"affine_{name}")["prep"]
        assert (prep["affine_bits"], prep["x_dtype"], prep["nq"], prep["xt_written"]) == (
            7, N.dtype_code(name), NQ - CHUNK, 1), prep
        np.testing.assert_array_equal(got[f"affine_{name}_idx"], got["affine_float64_idx"])
        np.testing.assert_array_equal(got[f"affine_{name}_dist"], got["affine_float64_dist"])


def _check_ties(got, O):
    """Case 4, rows that fail the certificate on both sides of the seam (rows 6,143, 6,144 and 9,999 among them).  Pins
    ``rescue_args``' ``row0 = c0`` (the list names call rows, the workspace holds chunk rows), the finaliser's switch to
    call-relative rows there, and ``fail_base``.

    The condition, on the CPU: each chosen row has an exact tie between its 5th and 6th nearest reference row, and by the
    restated certificate (tests/_rescue.py) even the largest ``t_min`` a sound pre-filter can report for it -- that of an
    outside row at the tied distance -- leaves the bound at or below tau, so the finaliser lists the row.  The rescue's
    record is call-wide: it ran, it was offered every row the finalisers listed, and it handed on at least the tied rows,
    which the exact scan consumed."""
    import _rescue as R

    ref, _ = _rows()
    q = _tie_queries()
    assert (TIE_ROWS < CHUNK).any() and (TIE_ROWS >= CHUNK).any() and {CHUNK - 1, CHUNK, NQ - 1} <= set(TIE_ROWS.tolist())
    v, _ = O.argkmin(q[TIE_ROWS], ref, 6, "expanded", squared=True)
    assert (v[:, 4] == v[:, 5]).all(), "a chosen row has no exact tie across its 5th neighbour"
    s, mu = float(got["s"]), got["mu"][:D]
    rb, qb = s * (ref - mu), s * (q[TIE_ROWS] - mu)
    ymax, qn = np.sqrt((rb * rb).sum(axis=1).max()), (qb * qb).sum(axis=1)
    eps, noise = R.certificate_terms(qn, ymax, s, D, (D + 15) // 16, 2.0 * np.linalg.norm(mu))
    tau = v[:, 4]
    assert (R.bound(qn, s * s * tau + eps - qn, eps, noise, 1.0 / (s * s)) <= tau).all()

    _equal(got, "ties", O.kneighbors(ref, q, 5, "expanded", row_offset=ROW_OFFSET))
    rec = _rec(got, "ties")
    resc, st = rec["rescue"], rec["stats"]
    assert resc["launched"] == 1 and resc["offered"] == st["exact_fallbacks"], rec
    assert len(TIE_ROWS) <= resc["handed_on"] <= resc["offered"] and rec["scan"]["rows"] == resc["handed_on"], rec


def _check_status(got, N):
    """Case 6, ``check_finite`` with a NaN in row 3 only, in row 6,144 only, and in the last row only (an infinity beside
    it).  Pins that the status word a chunk's ``launch_prep`` raises is seen by ``poll_status`` whichever chunk raised it,
    and that the failing call clears it: the clean call that follows is exact."""
    for name in ("first", "seam", "last"):
        code, message = json.loads(str(got[f"nonfinite_{name}"]))
        assert code == N.ERR_NONFINITE and NAN_MESSAGE in message, (name, code, message)
    od, oi = _want_counts()
    _equal(got, "after_nonfinite", (od[:NQ], oi[:NQ]))


def _check_xt_only(got, O, N):
    """Case 7, the loop's ``prep_chunk``-only branch: 7,000 float32 rows through the affine map, k = 32.  Pins ``xt + c0 * d``
    where no pre-filter runs and the exact scan reads every transformed row of the call.  d = 160 (no coarse image) is
    refused with an affine map and with narrow rows."""
    ref, _ = _rows()
    center, scale, proj, raw = _affine()
    xt = O.affine(raw[:NQ_XT].astype(np.float64), center, scale, proj)
    _equal(got, "xt_only", O.kneighbors(ref, xt, K_XT, "expanded", row_offset=ROW_OFFSET))
    rec = _rec(got, "xt_only")
    assert rec["pre"]["generation"] == 0 and rec["stats"]["exact_only_queries"] == NQ_XT, rec
    assert (rec["prep"]["kernel"] > 0, rec["prep"]["nq"], rec["prep"]["xt_written"]) == (True, NQ_XT - CHUNK, 1), rec["prep"]
    for name, text in (("wide_affine", "outside the HIP envelope"), ("wide_float32", "needs d <= 128")):
        code, message = json.loads(str(got[name]))
        assert code == N.ERR_UNSUPPORTED and text in message, (name, code, message)


def _check_shards(got, O):
    """The shard round trip of child B: three shards' candidates of 10,000 raw rows (``run_device`` in raw mode across the
    seam), merged with ``apply_affine``.  Pins ``merge_shards_device``'s prep loop, ``xdev + c0 * d_in`` -> ``xt + c0 * d``: the
    merge reads the transformed rows only for the rows it replays, and the oracle's merge must replay some behind the
    seam."""
    from sknnr_amd.distributed import shard_bounds

    ref, _ = _rows()
    center, scale, proj, raw = _affine()
    xt = O.affine(raw.astype(np.float64), center, scale, proj)
    sv, si = got["shard_val"], got["shard_idx"]
    for g in range(N_SHARDS):
        a, b = shard_bounds(N_REF, N_SHARDS, g)
        ov, oi = O.shard_candidates(ref[a:b], xt, K_SHARD, "expanded", index_offset=a)
        np.testing.assert_array_equal(si[g], oi, err_msg=f"shard {g}")
        np.testing.assert_array_equal(sv[g], ov, err_msg=f"shard {g}")
    *_, behind = O.merge_shards(ref, xt[CHUNK:], sv[:, CHUNK:], si[:, CHUNK:], K_SHARD, "expanded",
                                row_offset=ROW_OFFSET + CHUNK)
    assert behind > 0, "no row behind the seam is replayed: the merge would not read its transformed rows"
    md, mi, _ = O.merge_shards(ref, xt, sv, si, K_SHARD, "expanded", row_offset=ROW_OFFSET)
    _equal(got, "merge", (md, mi))
    _equal(got, "merge", O.kneighbors(ref, xt, K_SHARD, "expanded", row_offset=ROW_OFFSET), "merge against one heap")


# ---------------------------------------------------------------------------------------------------------------------
# the three tests
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_plain_order_across_seams(N, O, tmp_path):
    """Child A: chunks of 6,144 rows in the caller's order -- row counts at the quantum, X=None over two seams, narrow
    rows through the affine map, rescue on both sides of a seam, the status word, the prep-only loop."""
    got = _run_child("A", tmp_path, SKNNR_CHUNK_ROWS=str(CHUNK), SKNNR_CELLS="0")
    _check_counts(got, 0)
    _check_self_rows(got, O)
    _check_narrow_affine(got, O, N)
    _check_ties(got, O)
    _check_status(got, N)
    _check_xt_only(got, O, N)


@gpu
def test_bucketed_order_across_seams(N, O, tmp_path):
    """Child B: the same chunks with the rows of each chunk bucketed by cell -- cases 1, 2 and 4 again, and a shard round
    trip whose merge prepares its rows in two chunks."""
    got = _run_child("B", tmp_path, SKNNR_CHUNK_ROWS=str(CHUNK), SKNNR_CELLS="6")
    _check_counts(got, 6)
    _check_self_rows(got, O)
    _check_ties(got, O)
    _check_shards(got, O)


@gpu
def test_forest_map_across_a_seam(N, O, tmp_path):
    """Child C: 2^18 + 37 raw rows through the forest map, k = 4.  Pins ``run_forest``: the input stepped by
    ``c0 * f_d_in * dtype_bytes(query_dtype)`` (float32 and float64 rows), the chunk handed on with ``row_offset + c0`` and
    ``out + c0 * k``, the prediction of the same call at ``out + c0 * t``, and the status word of the second chunk.

    Expected values: node ids by the host traversal (TreeNodeTransformer.transform), then the oracle's weighted-Hamming
    neighbours of every row, and numpy's mean of the 1-D y over them."""
    assert _forest_chunk_rows(5) == FOREST_CHUNK
    t, x, y, q, w = _forest()
    ids_ref, ids_q = t.transform(x), t.transform(q)
    np.testing.assert_array_equal(ids_q, t.transform(q.astype(np.float64)))
    d0, i0 = O.argkmin_hamming(ids_q, ids_ref, w, FOREST_K)
    od, oi = O.deterministic_reorder(d0, i0, 10, ROW_OFFSET)
    ld, li = O.deterministic_reorder(d0, i0, 10, FOREST_OFFSET_LOW)
    # the low row_offset has power: without the seam's 2^18 in their base, rows behind the seam come out in another order
    _, lost = O.deterministic_reorder(d0[FOREST_CHUNK:], i0[FOREST_CHUNK:], 10, FOREST_OFFSET_LOW)
    assert (lost != li[FOREST_CHUNK:]).any()

    got = _run_child("C", tmp_path)
    assert json.loads(str(got["hamming"]))["ran"] == 1
    _equal(got, "f32", (od, oi))
    _equal(got, "f64", (od, oi))
    _equal(got, "low", (ld, li))
    np.testing.assert_array_equal(got["f32_pred"][:, 0], O.predict(y, od, oi))
    code, message = json.loads(str(got["nonfinite"]))
    assert code == N.ERR_NONFINITE and NAN_MESSAGE in message, (code, message)
    _equal(got, "after", (od[:300], oi[:300]))


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    {"A": lambda out: _child_euclid(out, True), "B": lambda out: _child_euclid(out, False), "C": _child_forest}[sys.argv[1]](
        sys.argv[2])
