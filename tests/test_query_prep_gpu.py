"""Every query preparation and bucketing launch, pinned bit for bit to the host restatement (tests/_query_prep.py).

The launches: prep_queries_direct_kernel<1..4>, prep_queries_kernel<256 / 128 / 64> (exact.hip.h), cell_assign_kernel and
the counting sort cell_count_kernel / cell_scatter_kernel (bucket.hip.h).  Every case makes one ``kneighbors`` call of a
single device chunk, asserts that ``Index.debug_last_prep()`` equals the restated dispatch, and compares every buffer the
call fills (``Index.debug_query_prep``): the f16 hi / lo image as raw bytes, ``qnc``, the float64 transformed rows and the
cells bit for bit, the permutation by everything the counting sort promises (``_query_prep.check_bucketing``: the order
inside a cell is not deterministic).  The answers of the calls are not checked here; other modules own that.

Teeth (scratch builds, never committed): of the 79 cases of this module, measured on an MI355X, fail
- 78 with the two K halves of every lo piece swapped (both kernels; all but the refusal of 300 columns),
- 78 with the qnc chain stopped one K-step early (both kernels),
- 22 with the padding rows of the image left unwritten (both kernels): every case whose call follows a larger one on its
  handle, test_row_counts by construction,
- 11 with `>=` turned to `>` in cell_of: every cell case that holds a row on a split value,
- 4 with dc of the LDS kernel's walk one short where d_in exceeds the rows per block (d_in 131 / 149 / 150 / 299),
- 2 with int32 rows widened through float32 (test_element_types[int32], both kernels).
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import _prefilter_dispatch as P
import _query_prep as Q

gpu = pytest.mark.gpu
pytestmark = gpu

N_SMALL = 300      # reference rows of the image cases (first-generation pre-filter, plain order)
N_CELLS = 4_500    # reference rows of the cell cases: SKNNR_CELLS=6 gives depth 3, as in test_prefilter_instances_gpu.py
K = 3


# ---------------------------------------------------------------------------------------------------------------------
# shared state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


@pytest.fixture(scope="module")
def handles(N):
    """handles(key, make, **env): one (index, image constants, affine map) per key; ``make()`` returns the reference rows
    and the affine map (None, or a dict of d_in / center / scale / proj); created under the environment variables given
    (read at index creation) and kept for the module."""
    made = {}

    def get(key, make, **env):
        if key not in made:
            ref, affine = make()
            with pytest.MonkeyPatch.context() as mp:
                for name, value in env.items():
                    mp.setenv(name, str(value))
                ix = N.Index(ref)
            if affine is not None:
                ix.set_affine(affine["d_in"], affine["center"], affine["scale"], affine["proj"])
            made[key] = (ix, ix.debug_image_constants(), affine, ref)
        return made[key]

    yield get
    for ix, *_ in made.values():
        ix.close()


def _affine_map(rng, d_in, d, parts, lo=-3.0, hi=3.0):
    """An affine map with the parts named in ``parts`` (c, s, p) for raw values in [lo, hi]."""
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    return dict(d_in=d_in,
                center=mid + 0.1 * half * rng.standard_normal(d_in) if "c" in parts else None,
                scale=half * rng.uniform(0.5, 2.0, d_in) if "s" in parts else None,
                proj=rng.standard_normal((d_in, d)) / np.sqrt(d_in) if "p" in parts else None)


def _plain(d, seed, n_ref=N_SMALL, scale=1.0, offset=0.0):
    def make():
        rng = np.random.default_rng([seed, d])
        return rng.standard_normal((n_ref, d)) * scale + offset, None
    return make


def _with_map(d_in, d, parts, seed, lo=-3.0, hi=3.0, n_ref=N_SMALL):
    """Reference rows that are the image of raw rows uniform in [lo, hi] under a random affine map."""
    def make():
        from oracle import oracle

        rng = np.random.default_rng([seed, d_in, d])
        a = _affine_map(rng, d_in, d, parts, lo, hi)
        raw = rng.uniform(lo, hi, (n_ref, d_in))
        return oracle.affine(raw, a["center"], a["scale"], a["proj"]), a
    return make


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(N, handle, x, k=K, *, apply_affine=False, prep_lds=False, device=False, check_finite=False, what=""):
    """One call on the rows ``x`` (None: X=None on the index's own rows), then the launch record against the restated
    dispatch and every buffer the call filled against the restatement.  Returns (record, buffers read back, restatement)."""
    ix, consts, affine, ref = handle
    self_rows = x is None
    rows = ref if self_rows else np.ascontiguousarray(x)
    nq, code = len(rows), 0 if self_rows else N.dtype_code(rows.dtype)
    amap = affine if apply_affine else None
    opts = ix.make_opts(k, exclude_self=self_rows, apply_affine=apply_affine, query_dtype=code, check_finite=check_finite)
    with pytest.MonkeyPatch.context() as mp:
        if prep_lds:
            mp.setenv("SKNNR_PREP_LDS", "1")
        else:
            mp.delenv("SKNNR_PREP_LDS", raising=False)
        if device:
            import torch

            xq = torch.as_tensor(rows, device="cuda")
            dist = torch.empty((nq, k), dtype=torch.float64, device="cuda")
            idx = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ix.kneighbors_device(xq.data_ptr(), nq, opts, dist.data_ptr(), idx.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        else:
            ix.kneighbors_host(None if self_rows else rows, opts, nq=nq)
    kk = k + (1 if self_rows else 0)
    bucketed = P.expected_launch(ix.n_ref, ix.d, kk, nq, depth=consts["cell_depth"])["cell_depth"] > 0
    expect = Q.expected_prep(ix.d, nq, d_in=amap["d_in"] if amap else None, center=bool(amap) and amap["center"] is not None,
                             scale=bool(amap) and amap["scale"] is not None, proj=bool(amap) and amap["proj"] is not None,
                             x_dtype=code, prep_lds=prep_lds, bucketed=bucketed)
    rec = ix.debug_last_prep()
    assert rec == expect, f"{what}: launched {rec}, dispatch says {expect}"
    record = bool(ix.debug_last_finalize()["record"])
    names = ["qimg", "qnc"] + (["xt"] if expect["xt_written"] else []) + (["cell", "perm"] if bucketed else []) + (
        ["qnc_pos"] if bucketed and record else [])
    got = ix.debug_query_prep(expect["nq_pad"], want=names)
    for missing in {"xt", "cell", "qnc_pos"} - set(names):  # a buffer the call did not fill is refused, not read stale
        with pytest.raises(N.HipBackendError) as e:
            ix.debug_query_prep(1, want=(missing,))
        assert e.value.code == N.ERR_INVALID
    want = Q.restate(rows, consts, bucketed=bucketed, **({k_: amap[k_] for k_ in ("center", "scale", "proj")} if amap else {}))
    if "xt" in names:
        np.testing.assert_array_equal(_bits(got["xt"]), _bits(want["xt"]), err_msg=f"{what}: xt")
    bad = np.flatnonzero((got["qimg"] != want["qimg"]).any(axis=1))
    assert bad.size == 0, f"{what}: image rows {bad[:8]} of {bad.size} differ (live rows: {nq}); first: got " \
                          f"{got['qimg'][bad[0]].view(np.float16)}, want {want['qimg'][bad[0]].view(np.float16)}"
    np.testing.assert_array_equal(_bits(got["qnc"]), _bits(want["qnc"]), err_msg=f"{what}: qnc")
    if bucketed:
        np.testing.assert_array_equal(got["cell"], want["cell"], err_msg=f"{what}: cell")
        Q.check_bucketing(got["perm"], got["cell"], nq, consts["cell_depth"], got["qnc"], got.get("qnc_pos"))
    return rec, got, want


# ---------------------------------------------------------------------------------------------------------------------
# rows: the edges of a wave (64), a block (256) and the row quantum (6144)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _row_queries():
    return np.random.default_rng(21).uniform(-3.0, 3.0, (6145, 9))


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257, 6143, 6144, 6145])
def test_row_counts(N, handles, nq):
    """Direct kernel, cells off, xt on through an affine map (9 -> 13 columns): the tail rows of a wave and of a block, and
    the padding rows up to the row quantum (all of the second one at 6145 rows) are zero in the image and in qnc, also
    where the workspace held the live rows of a larger call before."""
    h = handles("rows", _with_map(9, 13, "csp", 20))
    h[0].kneighbors_host(_row_queries(), h[0].make_opts(K, apply_affine=True))
    rec, got, _ = _run(N, h, _row_queries()[:nq], apply_affine=True, what=f"{nq} rows")
    assert rec["kernel"] == Q.KERNEL_DIRECT and rec["nq_pad"] == (12288 if nq > 6144 else 6144)
    assert not got["qimg"][nq:].any() and not got["qnc"][nq:].any()


# ---------------------------------------------------------------------------------------------------------------------
# direct kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 7, 13, 16, 17, 32, 33, 48, 49, 64])
def test_direct_kernel_widths(N, handles, d):
    """prep_queries_direct_kernel<1..4> at full and partly padded last K-steps: float64 rows (image and qnc only), and
    float32 rows (which also writes xt)."""
    h = handles(("plain", d), _plain(d, 30, scale=2.0, offset=0.5))
    q = np.random.default_rng([31, d]).standard_normal((333, d)) * 2.0 + 0.5
    rec, *_ = _run(N, h, q, what=f"d {d}, float64")
    assert (rec["kernel"], rec["xt_written"]) == (Q.KERNEL_DIRECT, 0)
    _run(N, h, q.astype(np.float32), what=f"d {d}, float32")


@pytest.mark.parametrize("parts, d_in, d", [("csp", 8, 13), ("csp", 21, 13), ("p", 9, 13), ("p", 20, 13), ("cp", 20, 13),
                                            ("sp", 9, 13), ("cs", 13, 13), ("cs", 16, 16), ("c", 16, 16), ("s", 13, 13),
                                            ("csp", 40, 64), ("csp", 75, 33)])
def test_direct_kernel_affine_map(N, handles, parts, d_in, d):
    """center / scale / proj each on and off, d_in odd and even (the scalar and the 16-byte load path of float64 rows),
    d_in below and above d; float32 rows take the scalar path at every d_in."""
    h = handles(("map", parts, d_in, d), _with_map(d_in, d, parts, 40))
    q = np.random.default_rng([41, d_in]).uniform(-3.0, 3.0, (333, d_in))
    rec, *_ = _run(N, h, q, apply_affine=True, what=f"{parts} {d_in} -> {d}, float64")
    assert (rec["kernel"], rec["xt_written"]) == (Q.KERNEL_DIRECT, 1)
    _run(N, h, q.astype(np.float32), apply_affine=True, what=f"{parts} {d_in} -> {d}, float32")


@pytest.mark.parametrize("d", [13, 64])
def test_direct_kernel_self_rows(N, handles, d):
    """X=None: the index's own float64 rows, no xt."""
    h = handles(("plain", d), _plain(d, 30, scale=2.0, offset=0.5))
    rec, *_ = _run(N, h, None, what=f"X=None, d {d}")
    assert (rec["nq"], rec["xt_written"]) == (N_SMALL, 0)


# ---------------------------------------------------------------------------------------------------------------------
# LDS kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [65, 80, 100, 128])
def test_lds_kernel_default_dispatch(N, handles, d):
    """prep_queries_kernel as default dispatch reaches it (five to eight K-steps; 256 rows per block up to 75 columns, 128
    beyond): plain float64 and float32 rows, and raw rows through an affine map of d + 3 columns."""
    q = np.random.default_rng([51, d]).standard_normal((333, d)) * 2.0 + 0.5
    h = handles(("plain", d), _plain(d, 50, scale=2.0, offset=0.5))
    rec, *_ = _run(N, h, q, what=f"d {d}, float64")
    assert (rec["kernel"], rec["rows_per_block"]) == (Q.KERNEL_LDS, 256 if d == 65 else 128)
    _run(N, h, q.astype(np.float32), what=f"d {d}, float32")
    h = handles(("map", "csp", d + 3, d), _with_map(d + 3, d, "csp", 52))
    raw = np.random.default_rng([53, d]).uniform(-3.0, 3.0, (333, d + 3))
    _run(N, h, raw, apply_affine=True, what=f"{d + 3} -> {d}")


@pytest.mark.parametrize("d_in, rows_per_block", [(75, 256), (76, 128), (149, 128), (150, 64), (299, 64)])
def test_lds_kernel_rows_per_block(N, handles, d_in, rows_per_block):
    """d = 70 with an image at every edge of the rows-per-block table (d_in above the block size from 149 on: the walk
    over the block's elements advances by less than a row per trip); 333 rows: whole blocks and a partial one."""
    h = handles(("map", "csp", d_in, 70), _with_map(d_in, 70, "csp", 60))
    raw = np.random.default_rng([61, d_in]).uniform(-3.0, 3.0, (333, d_in))
    rec, *_ = _run(N, h, raw, apply_affine=True, what=f"d_in {d_in}, float64")
    assert (rec["kernel"], rec["rows_per_block"]) == (Q.KERNEL_LDS, rows_per_block)
    _run(N, h, raw.astype(np.float32)[:130], apply_affine=True, what=f"d_in {d_in}, float32")


def test_lds_kernel_refuses_300_columns(N, handles):
    ix, *_ = h = handles(("map", "csp", 300, 70), _with_map(300, 70, "csp", 60))
    assert Q.expected_prep(70, 10, d_in=300, center=True, scale=True, proj=True) is None
    raw = np.random.default_rng(62).uniform(-3.0, 3.0, (10, 300))
    with pytest.raises(N.HipBackendError) as e:
        ix.kneighbors_host(raw, ix.make_opts(K, apply_affine=True))
    assert e.value.code == N.ERR_UNSUPPORTED and e.value.message == Q.UNSUPPORTED_MESSAGE.format(d_in=300)
    assert ix.debug_last_prep()["kernel"] == 0
    with pytest.raises(N.HipBackendError):
        ix.debug_query_prep(1, want=("qnc",))


@pytest.mark.parametrize("d", [13, 64])
def test_lds_kernel_on_narrow_spaces(N, handles, d):
    """SKNNR_PREP_LDS=1: prep_queries_kernel writes the image of one to four K-steps."""
    q = np.random.default_rng([31, d]).standard_normal((333, d)) * 2.0 + 0.5
    h = handles(("plain", d), _plain(d, 30, scale=2.0, offset=0.5))
    rec, *_ = _run(N, h, q, prep_lds=True, what=f"d {d}, float64")
    assert rec["kernel"] == Q.KERNEL_LDS
    _run(N, h, q.astype(np.float32), prep_lds=True, what=f"d {d}, float32")
    _run(N, h, None, prep_lds=True, what=f"d {d}, X=None")
    h = handles(("map", "csp", 21, d), _with_map(21, d, "csp", 40))
    raw = np.random.default_rng([41, 21]).uniform(-3.0, 3.0, (333, 21))
    _run(N, h, raw, apply_affine=True, prep_lds=True, what=f"21 -> {d}")


# ---------------------------------------------------------------------------------------------------------------------
# element types
# ---------------------------------------------------------------------------------------------------------------------
def _typed_rows(dtype, n, cols, rng):
    """Rows of ``dtype`` over its whole range, the first ones holding its extreme values."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        x = (rng.standard_normal((n, cols)) * 100.0).astype(dtype)
        fi = np.finfo(dtype)
        special = [fi.max, -fi.max, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, np.nextafter(fi.tiny, dtype.type(0)),
                   -0.0, 0.0, 1.0 + fi.eps, 16777217.0]
    else:
        ii = np.iinfo(dtype)
        x = rng.integers(ii.min, ii.max, (n, cols), dtype=dtype, endpoint=True)
        special = [ii.min, ii.max, 0, 1]
        if dtype == np.int32:
            special += [2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 31 - 2 ** 7 + 1, 123456789]
    for i, v in enumerate(special):  # alone in an otherwise tame row, and all together in one row
        x[i] = (x[i] % 7 if dtype.kind != "f" else np.sign(x[i]))
        x[i, i % cols] = v
        x[len(special), i % cols] = v
    return x


def _range_of(dtype):
    dtype = np.dtype(dtype)
    return (-300.0, 300.0) if dtype.kind == "f" else (float(np.iinfo(dtype).min), float(np.iinfo(dtype).max))


@pytest.mark.parametrize("lds", [False, True], ids=["direct", "lds"])
@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint16, np.uint8, np.int32])
def test_element_types(N, handles, dtype, lds):
    """Every narrow element type at the ends of its range (int32 beyond 2^24, float32 subnormals, -0.0 and values that
    overflow the image), widened exactly: against the restatement on the float64 values, not against a float64 call of
    the same kernel.  Direct kernel (d = 13) and LDS kernel (d = 70), without and with an affine map."""
    d = 70 if lds else 13
    name = np.dtype(dtype).name
    lo, hi = _range_of(dtype)
    rng = np.random.default_rng([70, d])
    h = handles(("typed", name, d), _plain(d, 71, scale=(hi - lo) / 8.0, offset=(hi + lo) / 2.0))
    rec, got, want = _run(N, h, _typed_rows(dtype, 200, d, rng), what=f"{name}, no map")
    assert rec["kernel"] == (Q.KERNEL_LDS if lds else Q.KERNEL_DIRECT) and rec["xt_written"] == 1
    if np.dtype(dtype).kind == "f":
        assert np.isinf(want["qnc"][:200]).any(), "the law should hold rows that overflow the image"
    assert np.isfinite(want["qnc"][:200]).sum() >= 150
    h = handles(("typed map", name, d), _with_map(d + 6, d, "csp", 72, lo, hi))
    _run(N, h, _typed_rows(dtype, 200, d + 6, rng), apply_affine=True, what=f"{name}, map")


# ---------------------------------------------------------------------------------------------------------------------
# image edges
# ---------------------------------------------------------------------------------------------------------------------
EDGE_B = [np.nextafter(32768.0, 0.0), 32768.0, np.nextafter(32768.0, np.inf), -32768.0, -np.nextafter(32768.0, 0.0), 40000.0,
          1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -30, -(1.0 + 2.0 ** -11), 2.0 ** -24, 2.0 ** -25,
          1.5 * 2.0 ** -25, 2.0 ** -26, -(2.0 ** -25), 0.0, 65504.0, 1.0 + 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25]


@pytest.mark.parametrize("lds", [False, True], ids=["direct", "lds"])
@pytest.mark.parametrize("d", [13, 32])
def test_image_edges(N, handles, d, lds):
    """Scaled values b placed just below, at and above 32768 (qnc finite / +inf), at float16 rounding ties (also one that
    only rounding through float32 first makes a tie), below the smallest float16 subnormal, at the largest float16 and at
    exactly mu (b = 0); each alone in a row, in the first, the last and a middle column, the first and the last live
    row among them.  The reference rows are integers symmetric about zero, so that mu = 0 and b = s x exactly."""
    def make():
        a = np.random.default_rng([80, d]).integers(-40, 41, (N_SMALL // 2, d)).astype(np.float64)
        return np.concatenate([a, -a]), None

    h = handles(("edges", d), make)
    consts = h[1]
    s = consts["s"]
    assert not consts["mu"].any() and np.log2(s) == np.round(np.log2(s))
    cols = [0, d // 2, d - 1]
    q = np.random.default_rng([81, d]).integers(-40, 41, (len(EDGE_B) * len(cols), d)).astype(np.float64)
    placed = []
    for i, bv in enumerate(EDGE_B):
        for j, c in enumerate(cols):
            q[i * len(cols) + j, c] = bv / s
            placed.append((i * len(cols) + j, c, bv))
    b = Q.scaled_rows(q, consts["mu"], s, len(q))
    for r, c, bv in placed:
        assert b[r, c] == bv, "the law does not hold"
    rec, got, want = _run(N, h, q, prep_lds=lds, what=f"edges, d {d}")
    assert rec["kernel"] == (Q.KERNEL_LDS if lds else Q.KERNEL_DIRECT)
    n_over = sum(1 for bv in EDGE_B if not abs(bv) < 32768.0) * len(cols)
    assert np.isinf(want["qnc"]).sum() == n_over and n_over == 5 * len(cols)


# ---------------------------------------------------------------------------------------------------------------------
# cells and the counting sort
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _cell_problem(d):
    from sknnr_amd import synth

    x_ref, _, x_q = synth.make_problem(N_CELLS, 6145, d, t=1, n_dup_refs=24, n_dup_queries=16)
    return x_ref, x_q


def _on_split_rows(ref, consts):
    """For every node of the tree, one reference row whose coordinate IS the node's split value (build_cell_tree takes the
    split from its rows): raising that split by one float32 step moves the row to the other side."""
    from oracle import oracle

    base = oracle.cell_assign(ref, consts["axes"], consts["centre"], consts["thr"])
    rows = []
    for node in range(len(consts["thr"])):
        thr = consts["thr"].copy()
        thr[node] = np.nextafter(thr[node], np.float32(np.inf))
        moved = np.flatnonzero(oracle.cell_assign(ref, consts["axes"], consts["centre"], thr) != base)
        assert moved.size >= 1, f"no reference row on the split of node {node}"
        rows.append(int(moved[0]))
    return rows


def _root_coordinate_is(x, consts, t):
    """Whether the float32 coordinate of row x along the first axis equals t exactly."""
    from oracle import oracle

    def side(thr):
        return oracle.cell_assign(x[None, :], consts["axes"][:1], consts["centre"], np.array([thr], dtype=np.float32))[0]

    return side(t) == 1 and side(np.nextafter(np.float32(t), np.float32(np.inf))) == 0


def _one_step_rows(row, consts):
    """Copies of a row that lies on the root split, its last three coordinates nudged by a few float32 steps each (a
    seeded random search) until the row's float32 coordinate along the first axis is exactly one step below / above the
    split value.  Candidates are found with a float64 emulation of the chain and kept only if the C fmaf chain confirms
    them."""
    t = np.float32(consts["thr"][0])
    axis, centre = consts["axes"][0], consts["centre"]
    row32 = row.astype(np.float32)
    tail = np.arange(len(row) - 3, len(row))
    nudges = np.random.default_rng(5).integers(-64, 65, (200_000, 3))
    x = np.repeat(row[None, :], len(nudges), axis=0)
    x[:, tail] = row32[tail].astype(np.float64) + nudges * np.spacing(np.abs(row32[tail])).astype(np.float64)
    v = x.astype(np.float32) - centre
    z = np.zeros(len(x), dtype=np.float32)
    for c in range(len(row)):
        z = (v[:, c].astype(np.float64) * np.float64(axis[c]) + z.astype(np.float64)).astype(np.float32)
    out = []
    for target in (np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))):
        hits = [i for i in np.flatnonzero(z == target)[:8] if _root_coordinate_is(x[i], consts, target)]
        assert hits, "no row one float32 step from the root split found"
        out.append(x[hits[0]])
    return out


_CELL_QUERIES = {}


def _cell_queries(d, ref, consts):
    """6145 query rows: row 0 ordinary; then, for every node, a copy of a reference row lying exactly on its split, and
    two rows one float32 step either side of the root split; the rest from the synthetic law."""
    if d not in _CELL_QUERIES:
        q = _cell_problem(d)[1].copy()
        on = _on_split_rows(ref, consts)
        special = [ref[r] for r in on] + _one_step_rows(ref[on[0]], consts)
        q[1:1 + len(special)] = special
        _CELL_QUERIES[d] = (q, len(special))
    return _CELL_QUERIES[d]


@pytest.mark.parametrize("prep_lds", [False, True], ids=["direct", "cell_assign"])
@pytest.mark.parametrize("nq", [1, 1000, 6145])
@pytest.mark.parametrize("d", [13, 64])
def test_cells(N, handles, d, nq, prep_lds):
    """Depth-3 cells named by prep_queries_direct_kernel and, behind the LDS kernel, by cell_assign_kernel (both equal the
    restatement, hence each other), then the counting sort; k = 5 files candidate records at d = 13 (qnc_pos is written),
    k = 20 and d = 64 do not."""
    h = handles(("cells", d), lambda: (_cell_problem(d)[0], None), SKNNR_CELLS=6)
    ix, consts, _, ref = h
    assert consts["cell_depth"] == 3
    q, n_special = _cell_queries(d, ref, consts)
    for k in (5, 20):
        rec, got, want = _run(N, h, q[:nq], k, prep_lds=prep_lds, what=f"d {d}, {nq} rows, k {k}")
        assert rec["cells_by"] == (Q.CELLS_BY_ASSIGN if prep_lds else Q.CELLS_BY_PREP)
        assert ("qnc_pos" in got) == (k == 5 and d == 13)
        if nq >= 1000:
            # rows on a split value fall right of it (>=); the two rows around the root split fall on either side
            on = want["cell"][1:1 + n_special - 2]
            assert [(int(on[node]) >> (2 - lvl)) & 1 for lvl in range(3) for node in range((1 << lvl) - 1, (2 << lvl) - 1)] == [1] * 7
            below, above = want["cell"][n_special - 1], want["cell"][n_special]
            assert (below >> 2, above >> 2) == (0, 1)
            assert len(np.unique(want["cell"][:nq])) == 8


@pytest.mark.parametrize("prep_lds", [False, True], ids=["direct", "cell_assign"])
def test_cells_all_rows_in_one_cell(N, handles, prep_lds):
    d = 13
    h = handles(("cells", d), lambda: (_cell_problem(d)[0], None), SKNNR_CELLS=6)
    q, _ = _cell_queries(d, h[3], h[1])
    cell = Q.cells(q, h[1], len(q))
    for c in (0, 7, 3):  # the first, the last (the padding rows' own) and a middle cell
        rows = q[cell == c]
        assert len(rows) > 300
        _, got, _ = _run(N, h, rows, 5, prep_lds=prep_lds, what=f"one cell ({c})")
        assert (got["cell"][:len(rows)] == c).all()


def test_cells_self_rows(N, handles):
    """X=None on the bucketed index: 4,500 float64 rows, kk = k + 1."""
    h = handles(("cells", 13), lambda: (_cell_problem(13)[0], None), SKNNR_CELLS=6)
    rec, got, _ = _run(N, h, None, 4, what="X=None, cells")
    assert rec["cells_by"] == Q.CELLS_BY_PREP and "qnc_pos" in got


# ---------------------------------------------------------------------------------------------------------------------
# entry paths, non-finite input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_entry_point(N, handles, dtype):
    """kneighbors_device on a torch tensor: the rows are read where they are."""
    h = handles("rows", _with_map(9, 13, "csp", 20))
    _run(N, h, _row_queries()[:257].astype(dtype), apply_affine=True, device=True, what="device tensor")


@pytest.mark.parametrize("lds", [False, True], ids=["direct", "lds"])
def test_nonfinite_input(N, handles, lds):
    """A NaN or an infinity alone in the first row, the last live row and the last column: the call fails with the
    reference's message, and the next clean call on the handle succeeds and prepares its rows as ever."""
    d = 70 if lds else 13
    h = handles(("map", "csp", d + 3, d), _with_map(d + 3, d, "csp", 52 if lds else 40))
    ix = h[0]
    raw = np.random.default_rng([90, d]).uniform(-3.0, 3.0, (321, d + 3))
    inf_msg = "Input X contains infinity or a value too large for dtype('float64')."
    for (r, c), bad, msg in (((0, 0), np.nan, "Input X contains NaN."), ((320, 1), np.inf, inf_msg),
                             ((200, d + 2), -np.inf, inf_msg), ((320, d + 2), np.nan, "Input X contains NaN.")):
        x = raw.copy()
        x[r, c] = bad
        with pytest.raises(N.HipBackendError) as e:
            ix.kneighbors_host(x, ix.make_opts(K, apply_affine=True, check_finite=True))
        assert e.value.code == N.ERR_NONFINITE and e.value.message == msg, (r, c)
        rec, *_ = _run(N, h, raw, apply_affine=True, check_finite=True, what=f"clean call after {bad} at {(r, c)}")
        assert rec["kernel"] == (Q.KERNEL_LDS if lds else Q.KERNEL_DIRECT)
