"""Nodata rows of streamed raster tiles, masked on the device (sknnr_amd/csrc/mask.hip.h, the masked entry points of
include/sknnr_hip.h, ``kneighbors_chunks`` / ``predict_chunks`` with ``nodata=``).

The yardstick is always the existing unmasked path on ``X[valid]`` with ``assert_array_equal``: valid rows must get exactly
its indices, distances and predictions, masked rows the fills (``fill_index``, NaN, NaN).  No row is exempted.  The
reference rows are an integer lattice (500 rows, k = 3): distances tie after the reorder's rounding, so its second key --
the row's position in the call -- decides the order, which proves that positions count valid rows only.  The mask itself
is compared with the host restatement (tests/_nodata.py).
"""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import _nodata as ND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REF, K = 500, 3
SENTINEL = {np.dtype(np.uint8): 255, np.dtype(np.int16): -32768, np.dtype(np.float32): -9999.0,
            np.dtype(np.float64): -9999.0}


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


def lattice(n, d, seed, hi=6):
    return np.random.default_rng(seed).integers(0, hi, size=(n, d))


@pytest.fixture(scope="module")
def raw():
    """raw(d, weights): a RawKNNRegressor on a 500-row integer lattice of d columns with t = 2 targets, one per key."""
    import sknnr_amd

    made = {}

    def get(d, weights="uniform"):
        if (d, weights) not in made:
            x = lattice(N_REF, d, 100 + d).astype(np.float64)
            y = np.random.default_rng(7).standard_normal((N_REF, 2))
            made[d, weights] = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights).fit(x, y)
        return made[d, weights]

    return get


def queries(nq, d, dtype, masked, seed=0):
    """Lattice query rows of ``dtype``; the rows named by ``masked`` get the dtype's sentinel in one column."""
    rng = np.random.default_rng(seed)
    x = lattice(nq, d, 1000 + seed).astype(dtype)
    rows = np.flatnonzero(masked)
    x[rows, rng.integers(0, d, size=rows.size)] = SENTINEL[np.dtype(dtype)]
    return x


def check_against_yardstick(est, x, valid, dist, idx, fill_index=-1):
    valid = np.asarray(valid, dtype=bool)
    assert idx.shape == (x.shape[0], K) and idx.dtype == np.int64
    if valid.any():
        yd, yi = est.kneighbors(x[valid])
        np.testing.assert_array_equal(idx[valid], yi)
        if dist is not None:
            np.testing.assert_array_equal(dist[valid], yd)
    assert (idx[~valid] == fill_index).all()
    if dist is not None:
        assert np.isnan(dist[~valid]).all() and not np.isnan(dist[valid]).any()


# ---------------------------------------------------------------------------------------------------------------------
# the mask alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
@pytest.mark.parametrize("d_in", [1, 7, 32])
def test_mask_rows_equals_the_restatement(N, dtype, d_in):
    import torch

    rng = np.random.default_rng(d_in)
    nq = 1000  # four blocks, the last one partial
    x = rng.integers(0, 5, size=(nq, d_in)).astype(dtype)
    per_column = rng.integers(0, 5, size=d_in).astype(np.float64)
    cases = {"scalar": np.full(d_in, 3.0), "per_column": per_column}
    if np.dtype(dtype).kind == "f":
        x[rng.random(x.shape) < 0.02] = np.nan
        nan_nd = per_column.copy()
        nan_nd[::2] = np.nan  # NaN is nodata in the even columns only: NaN elsewhere leaves a row valid
        cases["nan"] = nan_nd
        cases["all_nan"] = np.full(d_in, np.nan)
    for name, nodata in cases.items():
        want = ND.row_mask(x, nodata)
        valid, n_valid = N.mask_rows_host(x, nodata)
        np.testing.assert_array_equal(valid, want, err_msg=f"host memory, {name}")
        assert n_valid == int(want.sum()), name
        xt = torch.as_tensor(x, device="cuda")
        vt = torch.zeros(nq, dtype=torch.uint8, device="cuda")
        nv = N.mask_rows_device(xt.data_ptr(), nq, d_in, N.dtype_code(x.dtype), nodata, vt.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(vt.cpu().numpy(), want, err_msg=f"device memory, {name}")
        assert nv == int(want.sum()), name
    assert 0 < ND.row_mask(x, cases["per_column"]).sum() or d_in == 32


# ---------------------------------------------------------------------------------------------------------------------
# compaction edge cases: one masked call of one tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1025, 5000])
@pytest.mark.parametrize("kind", ND.MASK_KINDS)
def test_compaction_edge_cases(raw, nq, kind):
    d = 7  # rows of 7 int16: 14 bytes, no 4-byte alignment of a row
    est = raw(d)
    eng = est.engine_
    masked = ND.make_mask(kind, nq, seed=nq)
    x = queries(nq, d, np.int16, masked, seed=nq)
    nodata = np.full(d, float(SENTINEL[np.dtype(np.int16)]))
    valid = ND.row_mask(x, nodata).astype(bool)
    np.testing.assert_array_equal(valid, ~masked)
    before = eng.stats()["queries"]
    qdt = eng.query_dtype_code(x, est._formula(), False)
    opts = eng._opts(K, exclude_self=False, deterministic=True, decimals=est.DISTANCE_PRECISION_DECIMALS,
                     formula=est._formula(), apply_affine=False, check_finite=True, query_dtype=qdt)
    dist, idx, n_valid = eng._index.kneighbors_masked_host(x, opts, nodata, fill_index=-7)
    rec = eng._index.debug_last_mask()
    grew = eng.stats()["queries"] - before
    assert n_valid == valid.sum()
    assert rec["ran"] == 1 and rec["rows"] == nq and rec["valid_rows"] == n_valid and rec["valid_total"] == n_valid
    assert rec["path"] == ND.expected_path(valid) and rec["mask_blocks"] == ND.mask_blocks(nq) and rec["row_bytes"] == 2 * d
    if kind == "none":
        assert rec["path"] == ND.PATH_IN_PLACE
    if kind == "all":
        assert rec["path"] == ND.PATH_ALL_MASKED
    assert grew == n_valid, "masked rows must cost no search work"
    check_against_yardstick(est, x, valid, dist, idx, fill_index=-7)
    # the public streamed call, the tile cut in two
    cut = nq // 3
    tiles = [x[:cut], x[cut:]] if cut else [x]
    d2, i2 = est.kneighbors_chunks(tiles, nodata=SENTINEL[np.dtype(np.int16)], fill_index=-7)
    np.testing.assert_array_equal(i2, idx)
    np.testing.assert_array_equal(d2, dist)
    # an unmasked call zeroes the record
    est.kneighbors(x[:1].astype(np.float64))
    assert eng._index.debug_last_mask()["ran"] == 0


def test_one_call_crossing_a_device_chunk(raw):
    d, nq = 4, (1 << 18) + 100
    est = raw(d)
    masked = ND.blob_mask(nq, 0.3, seed=3)
    x = queries(nq, d, np.uint8, masked, seed=3)
    valid = ~masked
    dist, idx = est.kneighbors_chunks([x], nodata=255)
    rec = est.engine_._index.debug_last_mask()  # (before the yardstick's unmasked call zeroes the record)
    assert rec["ran"] == 1 and rec["valid_total"] == valid.sum() and rec["row_bytes"] == 4
    check_against_yardstick(est, x, valid, dist, idx)


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
def stream_tiles(d, dtype):
    """Three tiles of unequal size: mixed, fully masked, fully valid."""
    sizes = (1000, 300, 700)
    masks = [ND.make_mask("random30", sizes[0], seed=5), ND.make_mask("all", sizes[1]), ND.make_mask("none", sizes[2])]
    tiles = [queries(n, d, dtype, m, seed=20 + i) for i, (n, m) in enumerate(zip(sizes, masks))]
    return tiles, ~np.concatenate(masks)


def test_stream_equals_one_masked_call_and_the_yardstick(raw, N):
    d = 7
    est = raw(d)
    eng = est.engine_
    tiles, valid = stream_tiles(d, np.int16)
    x = np.concatenate(tiles)
    nodata = -32768
    dist, idx = est.kneighbors_chunks(iter(tiles), nodata=nodata)
    check_against_yardstick(est, x, valid, dist, idx)
    d1, i1 = eng.kneighbors(x, K, formula=est._formula(), nodata=np.full(d, float(nodata)))
    np.testing.assert_array_equal(i1, idx)
    np.testing.assert_array_equal(d1, dist)
    # indices only, and per-column nodata that masks the same rows
    i_only = est.kneighbors_chunks(iter(tiles), return_distance=False, nodata=[nodata] * d, fill_index=-5)
    np.testing.assert_array_equal(i_only[valid], idx[valid])
    assert (i_only[~valid] == -5).all()
    # out= arrays receive the fills
    out_d = np.full((x.shape[0] + 10, K), 123.0)
    out_i = np.full((x.shape[0] + 10, K), 123, dtype=np.int64)
    d2, i2 = est.kneighbors_chunks(iter(tiles), out=(out_d, out_i), nodata=nodata)
    assert np.shares_memory(d2, out_d) and np.shares_memory(i2, out_i)
    np.testing.assert_array_equal(out_i[:x.shape[0]], idx)
    np.testing.assert_array_equal(out_d[:x.shape[0]], dist)
    assert (out_i[x.shape[0]:] == 123).all()
    # the native stream: the running count of valid rows, and set_nodata after a push
    qdt = eng.query_dtype_code(x, est._formula(), False)
    stream = eng.open_stream(K, formula=est._formula(), query_dtype=qdt, nodata=np.full(d, float(nodata)))
    seen = 0
    for tile, n_valid in zip(tiles, (valid[:1000].sum(), 0, 700)):
        stream.push(tile)
        seen += n_valid
        assert stream.valid_rows() == seen
    with pytest.raises(N.HipBackendError) as err:
        stream.set_nodata(np.zeros(d))
    assert err.value.code == N.ERR_INVALID and "before the first push" in err.value.message
    assert stream.close() == x.shape[0]  # rows_pushed stays the pushed rows
    # nodata=None is the unmasked call
    d3, i3 = est.kneighbors_chunks(iter(tiles), nodata=None)
    yd, yi = est.kneighbors(x)
    np.testing.assert_array_equal(i3, yi)
    np.testing.assert_array_equal(d3, yd)


# ---------------------------------------------------------------------------------------------------------------------
# more tiles than the host pipeline has slots (kHostSlots = 4): the per-slot mask buffers are reused while other tiles
# are in flight, and regrown by a larger tile
# ---------------------------------------------------------------------------------------------------------------------
LONG_SIZES = (300, 1000, 1, 257, 2000, 64, 700, 256, 1500, 5)
LONG_KINDS = ("random30", "none", "all", "alternating", "block_run", "all", "first", "none", "random30", "last")


def long_stream_tiles(d, dtype):
    masks = [ND.make_mask(kind, n, seed=40 + i) for i, (n, kind) in enumerate(zip(LONG_SIZES, LONG_KINDS))]
    tiles = [queries(n, d, dtype, m, seed=60 + i) for i, (n, m) in enumerate(zip(LONG_SIZES, masks))]
    return tiles, masks


def test_long_stream_reuses_and_regrows_the_slots(raw):
    d = 7
    est = raw(d, "distance")
    eng = est.engine_
    tiles, masks = long_stream_tiles(d, np.int16)
    assert len(tiles) > 2 * 4 and max(LONG_SIZES[4:]) > max(LONG_SIZES[:4])  # every slot reused twice, and regrown
    x = np.concatenate(tiles)
    valid = ~np.concatenate(masks)
    nodata = np.full(d, -32768.0)
    # kneighbors_chunks
    dist, idx = est.kneighbors_chunks(iter(tiles), nodata=-32768, fill_index=-7)
    check_against_yardstick(est, x, valid, dist, idx, fill_index=-7)
    d1, i1 = eng.kneighbors(x, K, formula=est._formula(), nodata=nodata, fill_index=-7)
    np.testing.assert_array_equal(i1, idx)
    np.testing.assert_array_equal(d1, dist)
    # predict_chunks
    pred = est.predict_chunks(iter(tiles), nodata=-32768)
    assert pred.shape == (x.shape[0], 2)
    np.testing.assert_array_equal(pred[valid], est.predict(x[valid]))
    assert np.isnan(pred[~valid]).all() and not np.isnan(pred[valid]).any()
    p1 = eng.predict(x, K, "distance", formula=est._formula(), nodata=nodata)
    np.testing.assert_array_equal(p1, pred)
    # the native stream, neighbours and predictions at once; valid_rows() after every push
    qdt = eng.query_dtype_code(x, est._formula(), False)
    stream = eng.open_stream(K, weights="distance", formula=est._formula(), query_dtype=qdt, nodata=nodata, fill_index=-7)
    outs, seen = [], 0
    for tile, m in zip(tiles, masks):
        outs.append(stream.push(tile))
        seen += int((~m).sum())
        assert stream.valid_rows() == seen
    assert stream.close() == x.shape[0]
    np.testing.assert_array_equal(np.concatenate([o[0] for o in outs]), idx)
    np.testing.assert_array_equal(np.concatenate([o[1] for o in outs]), dist)
    np.testing.assert_array_equal(np.concatenate([o[2] for o in outs]), pred)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import _nodata as ND
import sknnr_amd
K, d, nq = 3, 7, {nq}
rng = np.random.default_rng(107)
ref = rng.integers(0, 6, size=(500, d)).astype(np.float64)
y = np.random.default_rng(7).standard_normal((500, 2))
est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(ref, y)
eng = est.engine_
masked = ND.blob_mask(nq, 0.3, seed=5, mean_len=600)
masked[3000:8000] = True    # whole tiles without a valid row ...
masked[10000:15000] = False  # ... and whole tiles without a masked one
x = rng.integers(0, 6, size=(nq, d)).astype(np.int16)
rows = np.flatnonzero(masked)
x[rows, rng.integers(0, d, size=rows.size)] = -32768
nodata = np.full(d, -32768.0)
valid = ND.row_mask(x, nodata).astype(bool)
assert (valid == ~masked).all()
qdt = eng.query_dtype_code(x, est._formula(), False)
kw = dict(exclude_self=False, deterministic=True, decimals=est.DISTANCE_PRECISION_DECIMALS, formula=est._formula(),
          apply_affine=False, check_finite=True, query_dtype=qdt)
dist, idx, n_valid = eng._index.kneighbors_masked_host(x, eng._opts(K, **kw), nodata, fill_index=-7)
rec = eng._index.debug_last_mask()
assert n_valid == valid.sum() and rec["ran"] == 1 and rec["valid_total"] == n_valid, (n_valid, rec)
assert rec["rows"] <= 2048 < nq, rec  # the record describes the LAST tile: the call was cut into tiles
pred, pd, pi, nv2 = eng._index.predict_masked_host(x, eng._opts(K, weight_mode=eng.weight_mode("distance"), **kw), nodata,
                                                   fill_index=-7, return_neighbors=True)
assert nv2 == n_valid
yd, yi = est.kneighbors(x[valid])
np.testing.assert_array_equal(idx[valid], yi)
np.testing.assert_array_equal(dist[valid], yd)
assert (idx[~valid] == -7).all() and np.isnan(dist[~valid]).all() and not np.isnan(dist[valid]).any()
np.testing.assert_array_equal(pi, idx)
np.testing.assert_array_equal(pd, dist)
np.testing.assert_array_equal(pred[valid], est.predict(x[valid]))
assert np.isnan(pred[~valid]).all() and not np.isnan(pred[valid]).any()
print("ok", nq, int(n_valid), rec["rows"])
"""


@pytest.mark.parametrize("ramp", [True, False])
def test_one_host_call_spanning_the_pipeline_slots(ramp):
    """SKNNR_HOST_CHUNK_ROWS is read once per process: a child answers 20,000 rows in one masked host call with tiles of
    at most 2,048 rows -- ten or more tiles through the four slots, once ramping up (256, 512, 1,024, then 2,048: every
    slot's mask buffers regrown) and once without -- and compares with the yardstick itself."""
    env = dict(os.environ, SKNNR_HOST_CHUNK_ROWS="2048")
    env.pop("SKNNR_PIPE_NO_RAMP", None)
    if not ramp:
        env["SKNNR_PIPE_NO_RAMP"] = "1"
    run = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), nq=20_000)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1].startswith("ok 20000 "), run.stdout[-500:]


def test_dataframe_index_of_masked_rows_is_the_fill(raw):
    import pandas as pd
    import sknnr_amd

    d = 4
    x_ref = pd.DataFrame(lattice(N_REF, d, 104).astype(np.float64), index=np.arange(N_REF) * 10 + 1000,
                         columns=[f"b{i}" for i in range(d)])
    y = np.random.default_rng(7).standard_normal((N_REF, 2))
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K).fit(x_ref, y)
    masked = ND.make_mask("random30", 600, seed=9)
    x = pd.DataFrame(queries(600, d, np.float64, masked, seed=9), columns=x_ref.columns)
    ids = est.kneighbors_chunks([x.iloc[:250], x.iloc[250:]], return_distance=False, return_dataframe_index=True,
                                nodata=-9999.0, fill_index=-1)
    want = est.kneighbors(x[~masked], return_distance=False, return_dataframe_index=True)
    np.testing.assert_array_equal(ids[~masked], want)
    assert (ids[masked] == -1).all() and (ids[~masked] >= 1000).all()  # never table[-1]
    ids0 = est.kneighbors_chunks([x], return_distance=False, return_dataframe_index=True, nodata=-9999.0, fill_index=0)
    assert (ids0[masked] == 0).all()
    np.testing.assert_array_equal(ids0[~masked], want)


# ---------------------------------------------------------------------------------------------------------------------
# predictions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_predict_chunks(raw, weights):
    d = 7
    est = raw(d, weights)
    tiles, valid = stream_tiles(d, np.int16)
    x = np.concatenate(tiles)
    pred = est.predict_chunks(iter(tiles), nodata=-32768)
    assert pred.shape == (x.shape[0], 2)
    np.testing.assert_array_equal(pred[valid], est.predict(x[valid]))
    assert np.isnan(pred[~valid]).all() and not np.isnan(pred[valid]).any()
    out = np.full((x.shape[0], 2), 5.0)
    est.predict_chunks(iter(tiles), out=out, nodata=-32768)
    np.testing.assert_array_equal(out, pred)
    p1 = est.engine_.predict(x, K, weights, formula=est._formula(), nodata=np.full(d, -32768.0))
    np.testing.assert_array_equal(p1, pred)


# ---------------------------------------------------------------------------------------------------------------------
# finiteness
# ---------------------------------------------------------------------------------------------------------------------
def test_finiteness_is_tested_on_valid_rows_only(raw):
    d = 7
    est = raw(d)
    masked = ND.make_mask("random30", 900, seed=2)
    masked[[10, 500]] = True
    masked[[11, 501]] = False
    x = queries(900, d, np.float64, masked, seed=2)
    keep = np.flatnonzero(x[10] != -9999.0)[0]
    ok = x.copy()
    ok[10, keep] = np.inf   # infinity and NaN in masked rows: not tested
    ok[500, np.flatnonzero(x[500] != -9999.0)[0]] = np.nan
    dist, idx = est.kneighbors_chunks([ok[:400], ok[400:]], nodata=-9999.0)
    check_against_yardstick(est, x, ~masked, dist, idx)
    bad = x.copy()
    bad[11, 2] = np.inf
    with pytest.raises(ValueError, match="Input X contains infinity"):
        est.kneighbors_chunks([bad[:400], bad[400:]], nodata=-9999.0)
    bad = x.copy()
    bad[501, 3] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN"):
        est.kneighbors_chunks([bad[:400], bad[400:]], nodata=-9999.0)
    # ... unless NaN is that column's nodata: then the row is masked
    nodata = np.full(d, -9999.0)
    nodata[3] = np.nan
    d2, i2 = est.kneighbors_chunks([bad[:400], bad[400:]], nodata=nodata)
    valid2 = ND.row_mask(bad, nodata).astype(bool)
    assert not valid2[501]  # (rows whose only sentinel sat in column 3 are valid now, and searched with it)
    yd, yi = est.kneighbors(bad[valid2])
    np.testing.assert_array_equal(i2[valid2], yi)
    np.testing.assert_array_equal(d2[valid2], yd)
    assert (i2[~valid2] == -1).all() and np.isnan(d2[~valid2]).all()


# ---------------------------------------------------------------------------------------------------------------------
# other estimators: the affine map and the forest map
# ---------------------------------------------------------------------------------------------------------------------
def test_transformed_estimator_affine_map(moscow):
    import sknnr_amd

    est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=K).fit(moscow["X_train"], moscow["y_train"])
    x = np.ascontiguousarray(np.concatenate([moscow["X_test"], moscow["X_train"]]), dtype=np.float64)
    masked = ND.make_mask("random30", x.shape[0], seed=4)
    rng = np.random.default_rng(4)
    rows = np.flatnonzero(masked)
    x[rows, rng.integers(0, x.shape[1], size=rows.size)] = -9999.0
    dist, idx = est.kneighbors_chunks([x[:50], x[50:]], nodata=-9999.0)
    yd, yi = est.kneighbors(x[~masked])
    np.testing.assert_array_equal(idx[~masked], yi)
    np.testing.assert_array_equal(dist[~masked], yd)
    assert (idx[masked] == -1).all() and np.isnan(dist[masked]).all()
    pred = est.predict_chunks([x[:50], x[50:]], nodata=-9999.0)
    np.testing.assert_array_equal(pred[~masked], est.predict(x[~masked]))
    assert np.isnan(pred[masked]).all()
    with pytest.raises(ValueError, match="expected"):
        est.kneighbors_chunks([x], nodata=[0.0, 1.0])


def test_forest_estimator_forest_map():
    import sknnr_amd

    rng = np.random.default_rng(11)
    x_ref = rng.standard_normal((N_REF, 6))
    y = x_ref[:, :2] + 0.1 * rng.standard_normal((N_REF, 2))
    est = sknnr_amd.RFNNRegressor(n_estimators=3, n_neighbors=K, random_state=0).fit(x_ref, y)
    assert est._map_on_device()
    x = rng.standard_normal((1200, 6)).astype(np.float32)
    masked = ND.make_mask("random30", 1200, seed=6)
    rows = np.flatnonzero(masked)
    x[rows, rng.integers(0, 6, size=rows.size)] = -9999.0
    dist, idx = est.kneighbors_chunks([x[:500], x[500:]], nodata=-9999.0)
    yd, yi = est.kneighbors(x[~masked])
    np.testing.assert_array_equal(idx[~masked], yi)
    np.testing.assert_array_equal(dist[~masked], yd)
    assert (idx[masked] == -1).all() and np.isnan(dist[masked]).all()
    pred = est.predict_chunks([x[:500], x[500:]], nodata=-9999.0)
    np.testing.assert_array_equal(pred[~masked], est.predict(x[~masked]))
    assert np.isnan(pred[masked]).all()


# ---------------------------------------------------------------------------------------------------------------------
# CUDA tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_cuda_tensors_through_the_masked_engine_call(raw):
    import torch

    d = 7
    est = raw(d, "distance")
    eng = est.engine_
    masked = ND.make_mask("random30", 3000, seed=8)
    x = queries(3000, d, np.int16, masked, seed=8)
    nodata = np.full(d, -32768.0)
    xt = torch.as_tensor(x, device="cuda")
    dist, idx = eng.kneighbors(xt, K, formula=est._formula(), nodata=nodata, check_finite=True)
    assert dist.is_cuda and idx.is_cuda
    check_against_yardstick(est, x, ~masked, dist.cpu().numpy(), idx.cpu().numpy())
    assert eng._index.debug_last_mask()["path"] == ND.PATH_COMPACTED
    out_d = torch.zeros((3000, K), dtype=torch.float64, device="cuda")
    out_i = torch.zeros((3000, K), dtype=torch.int64, device="cuda")
    eng.kneighbors(xt, K, formula=est._formula(), nodata=nodata, fill_index=-9, out=(out_d, out_i))
    check_against_yardstick(est, x, ~masked, out_d.cpu().numpy(), out_i.cpu().numpy(), fill_index=-9)
    pred = eng.predict(xt, K, "distance", formula=est._formula(), nodata=nodata)
    assert pred.is_cuda
    pred = pred.cpu().numpy()
    np.testing.assert_array_equal(pred[~masked], est.predict(x[~masked]))
    assert np.isnan(pred[masked]).all()
    # fully valid and fully masked tensors
    clean = torch.as_tensor(x[~masked], device="cuda")
    d1, i1 = eng.kneighbors(clean, K, formula=est._formula(), nodata=nodata)
    assert eng._index.debug_last_mask()["path"] == ND.PATH_IN_PLACE
    yd, yi = est.kneighbors(x[~masked])
    np.testing.assert_array_equal(i1.cpu().numpy(), yi)
    np.testing.assert_array_equal(d1.cpu().numpy(), yd)
    gone = torch.as_tensor(x[masked], device="cuda")
    d0, i0 = eng.kneighbors(gone, K, formula=est._formula(), nodata=nodata)
    assert eng._index.debug_last_mask()["path"] == ND.PATH_ALL_MASKED
    assert (i0.cpu().numpy() == -1).all() and np.isnan(d0.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# settings that answer tile by tile on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_settings_raise(raw):
    import sknnr_amd

    est = raw(4)
    x = lattice(50, 4, 1).astype(np.float64)
    with sknnr_amd.tree_tie_policy("tree"), pytest.raises(NotImplementedError, match="tree_tie_policy"):
        est.kneighbors_chunks([x], nodata=-1.0)
    with sknnr_amd.tree_tie_policy("tree"), pytest.raises(NotImplementedError, match="tree_tie_policy"):
        est.predict_chunks([x], nodata=-1.0)
    rng = np.random.default_rng(12)
    x_ref = rng.standard_normal((N_REF, 5))
    rf = sknnr_amd.RFNNRegressor(n_estimators=3, n_neighbors=K, random_state=0).fit(x_ref, x_ref[:, :2])
    with sknnr_amd.hamming_tie_policy("numpy"), pytest.raises(NotImplementedError, match="hamming_tie_policy"):
        rf.kneighbors_chunks([x_ref[:40]], nodata=-1.0)
    call = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=lambda dd: 1.0 / (1.0 + dd)).fit(
        lattice(N_REF, 4, 2).astype(np.float64), rng.standard_normal((N_REF, 2)))
    with pytest.raises(NotImplementedError, match="callable weights"):
        call.predict_chunks([x], nodata=-1.0)
    call.predict_chunks([x])  # (without nodata the callable still runs tile by tile)
    with pytest.raises(ValueError, match="column 0 is NaN"):
        est.kneighbors_chunks([x.astype(np.int16)], nodata=np.nan)
