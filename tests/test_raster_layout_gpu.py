"""Band-first raster tiles end to end (``kneighbors_chunks`` / ``predict_chunks`` with ``layout="bands"``, the stream's
``push_planes``): both transpositions run on the device (sknnr_amd/csrc/planes.hip.h).

The yardstick is always today's row call on the ``np.moveaxis`` tiles, transposed, with ``assert_array_equal``: the value
at ``[j, p]`` must be the value at ``[p, j]``, bit for bit.  The raw-space references are an integer lattice (500 rows of
7 uint8 columns, k = 3, two targets): distances tie after the reorder's rounding, so its second key -- the row's position
in the whole call -- decides the order, which proves that positions run on across band-first tiles.  After each bands
call ``sknnr_debug_last_planes`` must show that the device transposed the last tile in both directions.
"""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import _planes as PL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REF, D, K = 500, 7, 3
SIZES = (1, 300, 1024, 2500, 77)  # pixels per tile; 2500 is given as (7, 50, 50), 300 as a list of seven arrays


def lattice(n, d, seed, hi=6):
    return np.random.default_rng(seed).integers(0, hi, size=(n, d))


def band_tiles(dtype=np.uint8, d=D, seed=0, sizes=SIZES):
    """The five tiles, band-first in the forms a caller may use, and the same pixels as row tiles."""
    bands, rows = [], []
    for i, n in enumerate(sizes):
        x = lattice(n, d, 1000 + seed + i).astype(dtype)  # (n, d) rows
        cube = np.ascontiguousarray(x.T)                   # (d, n)
        if n == 2500:
            cube = cube.reshape(d, 50, 50)
        tile = [cube[j].copy() for j in range(d)] if n == 300 else cube
        bands.append(tile)
        rows.append(np.ascontiguousarray(np.moveaxis(np.asarray(cube), 0, -1).reshape(-1, d)))
    return bands, rows


@pytest.fixture(scope="module")
def raw():
    """raw(weights, y_1d): a RawKNNRegressor on the uint8 lattice with a dataframe index and two targets (or a 1-D y)."""
    import pandas as pd
    import sknnr_amd

    made = {}

    def get(weights="uniform", y_1d=False):
        if (weights, y_1d) not in made:
            x = pd.DataFrame(lattice(N_REF, D, 107).astype(np.uint8), index=np.arange(N_REF) * 10 + 1000)
            y = np.random.default_rng(7).standard_normal((N_REF, 2))
            made[weights, y_1d] = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights).fit(x, y[:, 0] if y_1d else y)
        return made[weights, y_1d]

    return get


def assert_device_path(index, n, d, esz, out_planes):
    rec = index.debug_last_planes()
    # (chunk_cols: the kernel's own column chunk -- the kernel tests choose their edge columns by tests/_planes.py's)
    assert rec == {"planes_in": 1, "rows": n, "cols": d, "elem_bytes": esz, "planes_out": 1, "out_planes": out_planes,
                   "chunk_cols": PL.chunk_cols(esz)}, rec


# ---------------------------------------------------------------------------------------------------------------------
# raw space
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("with_out", [False, True])
def test_kneighbors_chunks(raw, ids, with_out):
    est = raw()
    bands, rows = band_tiles()
    total = sum(SIZES)
    want_d, want_i = est.kneighbors_chunks(iter(rows), return_dataframe_index=ids)
    out = (np.full((K, total), -1.0), np.full((K, total), -5, dtype=np.int64)) if with_out else None
    dist, idx = est.kneighbors_chunks(iter(bands), return_dataframe_index=ids, out=out, layout="bands")
    assert_device_path(est.engine_._index, SIZES[-1], D, 1, 2 * K)
    assert dist.shape == (K, total) and idx.shape == (K, total) and idx.dtype == np.int64
    np.testing.assert_array_equal(idx, want_i.T)
    np.testing.assert_array_equal(dist, want_d.T)
    if with_out:
        np.testing.assert_array_equal(out[1], idx)
        np.testing.assert_array_equal(out[0], dist)
    if ids:
        assert (idx >= 1000).all()
    only = est.kneighbors_chunks(iter(bands), return_distance=False, return_dataframe_index=ids, layout="bands")
    assert_device_path(est.engine_._index, SIZES[-1], D, 1, K)
    np.testing.assert_array_equal(only, want_i.T)


@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("with_out", [False, True])
def test_predict_chunks(raw, weights, with_out):
    est = raw(weights)
    bands, rows = band_tiles(seed=3)
    total = sum(SIZES)
    want = est.predict_chunks(iter(rows))
    out = np.full((2, total), 5.0) if with_out else None
    pred = est.predict_chunks(iter(bands), out=out, layout="bands")
    assert_device_path(est.engine_._index, SIZES[-1], D, 1, 2)
    assert pred.shape == (2, total) and pred.dtype == want.dtype
    np.testing.assert_array_equal(pred, want.T)
    if with_out:
        np.testing.assert_array_equal(out, want.T)
    # an output raster: (targets, h, w) memory, handed over as (targets, h * w)
    raster = np.zeros((2, 2, 1951), dtype=np.float64)
    assert 2 * 1951 == total
    est.predict_chunks(iter(bands), out=raster.reshape(2, total), layout="bands")
    np.testing.assert_array_equal(raster.reshape(2, total), want.T)


def test_one_dimensional_y(raw):
    est = raw(y_1d=True)
    bands, rows = band_tiles(seed=4)
    total = sum(SIZES)
    want = est.predict_chunks(iter(rows))
    assert want.shape == (total,)
    pred = est.predict_chunks(iter(bands), layout="bands")
    assert_device_path(est.engine_._index, SIZES[-1], D, 1, 1)
    assert pred.shape == (total,)
    np.testing.assert_array_equal(pred, want)
    out = np.full(total, 5.0)
    est.predict_chunks(iter(bands), out=out, layout="bands")
    np.testing.assert_array_equal(out, want)


def test_nodata_and_fill_index(raw):
    """A per-band nodata: tile 0 (one pixel) and tile 2 are fully masked, tile 3 fully valid, the others mixed."""
    est = raw()
    bands, rows = band_tiles(seed=5)
    nodata = np.array([255, 254, 255, 253, 255, 255, 250], dtype=np.float64)
    rng = np.random.default_rng(5)
    for i, r in enumerate(rows):
        n = r.shape[0]
        masked = {0: np.ones(n, bool), 2: np.ones(n, bool), 3: np.zeros(n, bool)}.get(i, rng.random(n) < 0.3)
        col = rng.integers(0, D, size=n)
        r[masked, col[masked]] = nodata[col[masked]].astype(np.uint8)
        cube = np.ascontiguousarray(r.T)
        bands[i] = [cube[j].copy() for j in range(D)] if n == 300 else (cube.reshape(D, 50, 50) if n == 2500 else cube)
    for ids in (False, True):
        want_d, want_i = est.kneighbors_chunks(iter(rows), nodata=nodata, fill_index=-7, return_dataframe_index=ids)
        dist, idx = est.kneighbors_chunks(iter(bands), nodata=nodata, fill_index=-7, return_dataframe_index=ids, layout="bands")
        assert_device_path(est.engine_._index, SIZES[-1], D, 1, 2 * K)
        assert est.engine_._index.debug_last_mask()["ran"] == 1
        np.testing.assert_array_equal(idx, want_i.T)
        np.testing.assert_array_equal(dist, want_d.T)
        assert (idx[:, :1] == -7).all() and np.isnan(dist[:, 301:1325]).all() and not np.isnan(dist[:, 1325:3825]).any()
    want = est.predict_chunks(iter(rows), nodata=nodata)
    pred = est.predict_chunks(iter(bands), nodata=nodata, layout="bands")
    np.testing.assert_array_equal(pred, want.T)
    assert np.isnan(pred[:, 0]).all()


def test_use_deterministic_ordering_off(raw):
    est = raw()
    bands, rows = band_tiles(seed=6)
    want_d, want_i = est.kneighbors_chunks(iter(rows), use_deterministic_ordering=False)
    dist, idx = est.kneighbors_chunks(iter(bands), use_deterministic_ordering=False, layout="bands")
    np.testing.assert_array_equal(idx, want_i.T)
    np.testing.assert_array_equal(dist, want_d.T)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16, np.uint16, np.int32, np.int64])
def test_every_query_dtype(raw, dtype):
    """(int64 is no device dtype: its bands are converted to float64 band by band, as the row call converts its rows)"""
    est = raw()
    bands, rows = band_tiles(dtype=dtype, seed=8, sizes=(300, 1024, 77))
    want_d, want_i = est.kneighbors_chunks(iter(rows))
    dist, idx = est.kneighbors_chunks(iter(bands), layout="bands")
    esz = 8 if dtype == np.int64 else np.dtype(dtype).itemsize
    assert_device_path(est.engine_._index, 77, D, esz, 2 * K)
    np.testing.assert_array_equal(idx, want_i.T)
    np.testing.assert_array_equal(dist, want_d.T)


# ---------------------------------------------------------------------------------------------------------------------
# affine and forest spaces
# ---------------------------------------------------------------------------------------------------------------------
def test_affine_space_float32_bands_with_nan_nodata(moscow):
    import sknnr_amd

    est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=K).fit(moscow["X_train"], moscow["y_train"])
    x = np.ascontiguousarray(np.concatenate([moscow["X_test"], moscow["X_train"]]), dtype=np.float32)
    rng = np.random.default_rng(4)
    masked = rng.random(x.shape[0]) < 0.3
    rows_m = np.flatnonzero(masked)
    x[rows_m, rng.integers(0, x.shape[1], size=rows_m.size)] = np.nan
    rows = [x[:50], x[50:]]
    bands = [np.ascontiguousarray(r.T) for r in rows]
    bands[1] = bands[1].reshape(x.shape[1], 5, -1)
    want_d, want_i = est.kneighbors_chunks(iter(rows), nodata=np.nan)
    dist, idx = est.kneighbors_chunks(iter(bands), nodata=np.nan, layout="bands")
    assert_device_path(est.regressor_.engine_._index, rows[1].shape[0], x.shape[1], 4, 2 * K)
    np.testing.assert_array_equal(idx, want_i.T)
    np.testing.assert_array_equal(dist, want_d.T)
    assert np.isnan(dist[:, masked]).all() and not np.isnan(dist[:, ~masked]).any()
    want = est.predict_chunks(iter(rows), nodata=np.nan)
    pred = est.predict_chunks(iter(bands), nodata=np.nan, layout="bands")
    np.testing.assert_array_equal(pred, want.T)


def test_forest_space_int16_bands():
    import sknnr_amd

    rng = np.random.default_rng(11)
    x_ref = rng.integers(-300, 300, size=(N_REF, 6)).astype(np.float64)
    y = x_ref[:, :2] + 0.1 * rng.standard_normal((N_REF, 2))
    est = sknnr_amd.RFNNRegressor(n_estimators=3, n_neighbors=K, random_state=0).fit(x_ref, y)
    assert est._map_on_device()
    x = rng.integers(-300, 300, size=(1200, 6)).astype(np.int16)
    rows = [x[:500], x[500:]]
    bands = [np.ascontiguousarray(r.T) for r in rows]
    want_d, want_i = est.kneighbors_chunks(iter(rows))
    dist, idx = est.kneighbors_chunks(iter(bands), layout="bands")
    assert_device_path(est.regressor_.engine_._index, 700, 6, 2, 2 * K)
    np.testing.assert_array_equal(idx, want_i.T)
    np.testing.assert_array_equal(dist, want_d.T)
    want = est.predict_chunks(iter(rows))
    pred = est.predict_chunks(iter(bands), layout="bands")
    np.testing.assert_array_equal(pred, want.T)
    # 64-bit integer bands reach float32 in one rounding, as the row call's validation does
    big = [r.astype(np.int64) for r in rows]
    w64 = est.kneighbors_chunks(iter(big), return_distance=False)
    i64 = est.kneighbors_chunks(iter([np.ascontiguousarray(r.T) for r in big]), return_distance=False, layout="bands")
    assert_device_path(est.regressor_.engine_._index, 700, 6, 4, K)
    np.testing.assert_array_equal(i64, w64.T)


# ---------------------------------------------------------------------------------------------------------------------
# the native stream: both kinds of push in one stream
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_pushes_in_one_stream(raw):
    est = raw("distance")
    eng = est.engine_
    bands, rows = band_tiles(seed=9)
    want_d, want_i = est.kneighbors_chunks(iter(rows))
    want_p = est.predict_chunks(iter(rows))
    code = eng.query_dtype_code(rows[0], est._formula(), False)
    stream = eng.open_stream(K, weights="distance", want_dist=True, decimals=est.DISTANCE_PRECISION_DECIMALS,
                             formula=est._formula(), check_finite=True, query_dtype=code)
    got, row = [], 0
    for i, (b, r) in enumerate(zip(bands, rows)):
        n = r.shape[0]
        if i % 2:
            got.append((False, row, n) + stream.push(r))
            assert eng._index.debug_last_planes()["planes_in"] == 0
        else:
            flat = [np.asarray(b[j]).reshape(-1) for j in range(D)]
            got.append((True, row, n) + stream.push_planes(flat))
            assert_device_path(eng._index, n, D, 1, 2 * K + 2)
        row += n
    assert stream.close() == row
    for planes, r0, n, idx, dist, pred in got:
        fix = (lambda a: a.T) if planes else (lambda a: a)
        np.testing.assert_array_equal(fix(idx), want_i[r0:r0 + n])
        np.testing.assert_array_equal(fix(dist), want_d[r0:r0 + n])
        np.testing.assert_array_equal(fix(pred), want_p[r0:r0 + n])


_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import pandas as pd
import sknnr_amd
import test_raster_layout_gpu as T
x = pd.DataFrame(T.lattice(T.N_REF, T.D, 107).astype(np.uint8), index=np.arange(T.N_REF) * 10 + 1000)
y = np.random.default_rng(7).standard_normal((T.N_REF, 2))
est = sknnr_amd.RawKNNRegressor(n_neighbors=T.K, weights="distance").fit(x, y)
sizes = (1, 300, 1024, 2500, 7000)  # (7,000 pixels: seven tiles of at most 1,024 through the four slots)
bands, rows = T.band_tiles(seed=10, sizes=sizes)
want_d, want_i = est.kneighbors_chunks(iter(rows))
dist, idx = est.kneighbors_chunks(iter(bands), layout="bands")
rec = est.engine_._index.debug_last_planes()
assert rec["planes_in"] == 1 and rec["planes_out"] == 1 and rec["rows"] <= 1024 < 7000 and rec["out_planes"] == 2 * T.K, rec
np.testing.assert_array_equal(idx, want_i.T)
np.testing.assert_array_equal(dist, want_d.T)
# the largest tile first: an idle pipeline ramps up (unless SKNNR_PIPE_NO_RAMP is set)
want_d, want_i = est.kneighbors_chunks(iter(rows[::-1]))
dist, idx = est.kneighbors_chunks(iter(bands[::-1]), layout="bands")
np.testing.assert_array_equal(idx, want_i.T)
np.testing.assert_array_equal(dist, want_d.T)
nodata = 5
want = est.predict_chunks(iter(rows), nodata=nodata)
out = np.zeros((2, sum(sizes)))
est.predict_chunks(iter(bands), nodata=nodata, out=out, layout="bands")
np.testing.assert_array_equal(out, want.T)
assert np.isnan(out).any() and not np.isnan(out).all()
print("ok", sum(sizes), rec["rows"])
"""


@pytest.mark.parametrize("ramp", [True, False])
def test_small_tiles_reuse_the_slots_with_plane_buffers_live(ramp):
    """SKNNR_HOST_CHUNK_ROWS is read once per process: a child runs the tiles with at most 1,024 pixels per pipeline tile
    -- pushes are split into more tiles than the four slots, once ramping up (128, 256, 512, then 1,024: every slot's
    plane buffers regrown) and once without -- and compares with the row call itself."""
    env = dict(os.environ, SKNNR_HOST_CHUNK_ROWS="1024")
    env.pop("SKNNR_PIPE_NO_RAMP", None)
    if not ramp:
        env["SKNNR_PIPE_NO_RAMP"] = "1"
    run = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1].startswith("ok 10825 "), run.stdout[-500:]


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(raw, moscow):
    import sknnr_amd
    import torch

    est = raw()
    bands, rows = band_tiles(seed=12, sizes=(50,))
    with pytest.raises(ValueError, match="layout must be 'rows' or 'bands'"):
        est.kneighbors_chunks(iter(bands), layout="planes")
    with pytest.raises(ValueError, match=r"X has 6 features, but RawKNNRegressor is expecting 7 features as input\."):
        est.kneighbors_chunks([bands[0][:6]], layout="bands")
    with pytest.raises(TypeError, match="streamed tiles are host arrays"):
        est.kneighbors_chunks([torch.as_tensor(bands[0], device="cuda")], layout="bands")
    with pytest.raises(ValueError, match="out arrays must be C-contiguous"):
        est.kneighbors_chunks(iter(bands), out=(None, np.zeros((50, K), dtype=np.int64)), layout="bands")
    with pytest.raises(ValueError, match="out arrays must share one number of columns"):  # (before any tile is written)
        est.kneighbors_chunks(iter(bands), out=(np.zeros((K, 50)), np.zeros((K, 55), dtype=np.int64)), layout="bands")
    with sknnr_amd.tree_tie_policy("tree"), pytest.raises(NotImplementedError, match="layout='bands'.*tree_tie_policy"):
        est.kneighbors_chunks(iter(bands), layout="bands")
    with sknnr_amd.tree_tie_policy("tree"), pytest.raises(NotImplementedError, match="layout='bands'.*tree_tie_policy"):
        est.predict_chunks(iter(bands), layout="bands")
    rng = np.random.default_rng(12)
    x_ref = rng.standard_normal((N_REF, 5))
    rf = sknnr_amd.RFNNRegressor(n_estimators=3, n_neighbors=K, random_state=0).fit(x_ref, x_ref[:, :2])
    with sknnr_amd.hamming_tie_policy("numpy"), pytest.raises(NotImplementedError, match="layout='bands'.*hamming_tie_policy"):
        rf.kneighbors_chunks([np.ascontiguousarray(x_ref[:40].T)], layout="bands")
    call = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=lambda dd: 1.0 / (1.0 + dd)).fit(
        lattice(N_REF, D, 2).astype(np.float64), rng.standard_normal((N_REF, 2)))
    with pytest.raises(NotImplementedError, match="layout='bands'.*callable weights"):
        call.predict_chunks(iter(bands), layout="bands")
    # a transformer that runs on the host never sees band-first tiles
    host = sknnr_amd.EuclideanKNNRegressor(n_neighbors=K).fit(moscow["X_train"], moscow["y_train"])
    host._device_affine = False
    xt = np.ascontiguousarray(np.asarray(moscow["X_test"], dtype=np.float64).T)
    with pytest.raises(NotImplementedError, match="layout='bands'.*transformer runs on the host"):
        host.kneighbors_chunks([xt], layout="bands")
    with pytest.raises(NotImplementedError, match="layout='bands'.*transformer runs on the host"):
        host.predict_chunks([xt], layout="bands")
    # a non-finite band still raises the reference's sentence
    f_bands = [np.ascontiguousarray(rows[0].T).astype(np.float32)]
    f_bands[0][3, 17] = np.inf
    with pytest.raises(ValueError, match="Input X contains infinity"):
        est.kneighbors_chunks(iter(f_bands), layout="bands")
    f_bands[0][3, 17] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN"):
        est.predict_chunks(iter(f_bands), layout="bands")
    # ... and the handle answers the next call as if nothing had happened
    want = est.kneighbors_chunks(iter(rows), return_distance=False)
    np.testing.assert_array_equal(est.kneighbors_chunks(iter(bands), return_distance=False, layout="bands"), want.T)
