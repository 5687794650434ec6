"""Typed raster outputs end to end: ``predict_chunks(out_dtype=..., scale=..., offset=..., out_nodata=...)`` and
``kneighbors_chunks(index_dtype=..., distance_dtype=...)``, the stream's ``set_output``.  The device converts each tile
(sknnr_amd/csrc/narrow.hip.h) and only the narrow bytes are copied out.

The yardstick is always the SAME call without the new arguments: every typed result must equal the numpy restatement
(tests/_narrow.py) applied to the float64 / int64 result, exactly (``assert_array_equal``).  300 reference rows of 6
integer-valued features, k = 3, t = 3 and 17 targets; five tiles of 1, 255, 256, 257 and 700 rows -- one below, at and
one above the conversion kernels' 256-row workgroup -- as float64 and as int16, as rows and band-first, with and without a
nodata value (about a quarter of the rows, a fully masked 1-row tile among them), with and without ``out``.  After each
typed call ``sknnr_debug_last_narrow`` must show that the conversion ran on the device and that the last tile's
device-to-host copies moved ``n * cols * sizeof(type)`` bytes.

Without the feature every test here fails with ``TypeError`` (unexpected keyword) / ``AttributeError``.

Measured on an MI355X: the 98 cases of this module take 4.7 s, of which 3.4 s are the first case's device set-up; no other
case takes more than 0.25 s.
"""

from __future__ import annotations

import numpy as np
import pytest

import _narrow as NR

pytestmark = pytest.mark.gpu

N_REF, D, K = 300, 6, 3
SIZES = (1, 255, 256, 257, 700)
NODATA = -9999
OUT_DTYPES = [np.float32, np.int16, np.uint16, np.uint8, np.int32]
CODE = {np.dtype(np.float64): 0, np.dtype(np.int64): 0, np.dtype(np.float32): 1, np.dtype(np.int16): 2,
        np.dtype(np.uint16): 3, np.dtype(np.uint8): 4, np.dtype(np.int32): 5}


def make_tiles(dtype, masked, seed=0):
    """The five row tiles (n_i, D); with ``masked`` a quarter of the rows hold the nodata value in some column, and the
    1-row tile is masked."""
    rng = np.random.default_rng(100 + seed)
    tiles = []
    for n in SIZES:
        x = rng.integers(-40, 40, size=(n, D)).astype(np.int16)
        if masked:
            rows = np.flatnonzero(rng.random(n) < 0.25) if n > 1 else np.array([0])
            x[rows, rng.integers(0, D, size=rows.size)] = NODATA
        tiles.append(np.ascontiguousarray(x.astype(dtype)))
    return tiles


def as_bands(tiles):
    return [np.ascontiguousarray(t.T) for t in tiles]


@pytest.fixture(scope="module")
def E():
    """E(t, weights, y_dtype): a RawKNNRegressor on 300 integer-valued rows with a dataframe index; targets spread over
    [-100, 400) so that uint8 and, scaled, int16 clamp at both ends."""
    import pandas as pd
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    made = {}

    def get(t=3, weights="uniform", y_dtype=np.float64):
        key = (t, weights, np.dtype(y_dtype))
        if key not in made:
            rng = np.random.default_rng(7)
            x = pd.DataFrame(rng.integers(-40, 40, size=(N_REF, D)).astype(np.float64), index=np.arange(N_REF) * 7 + 5000)
            y = (rng.random((N_REF, t)) * 500.0 - 100.0).astype(y_dtype)
            made[key] = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights).fit(x, y)
        return made[key]

    return get


_REFS = {}


def reference(key, compute):
    """The untyped result of a call, computed once per module and left unchanged."""
    if key not in _REFS:
        r = compute()
        for a in (r if isinstance(r, tuple) else (r,)):
            a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def scaling(kind, t):
    if kind == "none":
        return None, None
    if kind == "scalar":
        return 100.0, -3.0
    return np.linspace(0.1, 90.0, t), np.linspace(-50.0, 50.0, t)


def restate_pred(ref, dtype, scale, offset, fill, bands, t):
    rows = ref.T if bands else ref
    s = None if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), (t,))
    o = None if scale is None else np.broadcast_to(np.asarray(offset, dtype=np.float64), (t,))
    got = NR.narrow_values(rows, dtype, s, o, fill)
    return got.T if bands else got


def assert_record(est, ran, n_last, idx_dt, dist_dt, pred_dt, cols_bytes):
    rec = est.engine_._index.debug_last_narrow()
    assert rec["ran"] == ran and rec["rows"] == n_last, rec
    assert (rec["idx_dtype"], rec["dist_dtype"], rec["pred_dtype"]) == (idx_dt, dist_dt, pred_dt), rec
    assert rec["d2h_bytes"] == n_last * cols_bytes, rec
    return rec


@pytest.mark.parametrize("layout", ["rows", "bands"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("scale_kind", ["none", "scalar", "per_target"])
@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
def test_predict_chunks_every_type(E, out_dtype, scale_kind, masked, layout):
    bands = layout == "bands"
    dt = np.dtype(out_dtype)
    t = 17 if (OUT_DTYPES.index(out_dtype) + (scale_kind == "scalar") + masked) % 2 else 3
    est = E(t)
    scale, offset = scaling(scale_kind, t)
    total = sum(SIZES)
    for in_dtype in (np.float64, np.int16):
        tiles = make_tiles(in_dtype, masked)
        feed = as_bands(tiles) if bands else tiles
        kw = dict(layout=layout, nodata=NODATA if masked else None)
        ref = reference(("pred", t, np.dtype(in_dtype), masked, layout), lambda: est.predict_chunks(iter(feed), **kw))
        assert ref.dtype == np.float64 and ref.shape == ((t, total) if bands else (total, t))
        assert bool(np.isnan(ref).any()) == masked
        fill = None
        if masked:
            fill = {np.dtype(np.float32): None, np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535}.get(dt, -32768)
        want = restate_pred(ref, dt, scale, offset, fill, bands, t)
        typed = dict(out_dtype=dt, scale=scale, offset=offset, out_nodata=fill)
        got = est.predict_chunks(iter(feed), **kw, **typed)
        assert got.dtype == dt and got.shape == ref.shape
        np.testing.assert_array_equal(got, want)
        rec = assert_record(est, 1, SIZES[-1], 0, 0, CODE[dt], t * dt.itemsize)
        # the last tile (700 rows, a 16-byte aligned slot buffer): packed rows take the wide path; planes 700 apart too
        assert rec["wide_mask"] == 4, rec
        out = np.full(ref.shape, 77, dtype=dt)
        ret = est.predict_chunks(iter(feed), out=out, **kw, **typed)
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(ret, want)
        with pytest.raises(ValueError, match="out arrays must be C-contiguous"):  # (a float64 out is the wrong type now)
            est.predict_chunks(iter(feed), out=np.zeros(ref.shape), **kw, **typed)


def test_float32_fill_and_default_nan(E):
    est = E(3)
    tiles = make_tiles(np.int16, True)
    ref = reference(("pred", 3, np.dtype(np.int16), True, "rows"), lambda: est.predict_chunks(iter(tiles), nodata=NODATA))
    got = est.predict_chunks(iter(tiles), nodata=NODATA, out_dtype=np.float32)
    np.testing.assert_array_equal(got, ref.astype(np.float32))  # (NaN stays NaN)
    assert np.isnan(got).any()
    got = est.predict_chunks(iter(tiles), nodata=NODATA, out_dtype=np.float32, out_nodata=-9999.0, scale=0.5)
    np.testing.assert_array_equal(got, NR.narrow_values(ref, np.float32, np.full(3, 0.5), np.zeros(3), -9999.0))
    assert not np.isnan(got).any() and (got == -9999.0).any()


@pytest.mark.parametrize("weights, y_dtype, t", [("distance", np.float64, 3), ("distance", np.float64, 17),
                                                 ("uniform", np.float32, 3), ("distance", np.float32, 17)])
@pytest.mark.parametrize("layout", ["rows", "bands"])
def test_distance_weights_and_float32_targets(E, weights, y_dtype, t, layout):
    est = E(t, weights, y_dtype)
    bands = layout == "bands"
    tiles = make_tiles(np.int16, True, seed=1)
    feed = as_bands(tiles) if bands else tiles
    ref64 = np.empty((t, sum(SIZES)) if bands else (sum(SIZES), t))  # (into a float64 out: float32 targets held exactly)
    est.predict_chunks(iter(feed), out=ref64, nodata=NODATA, layout=layout)
    for dt, fill in ((np.dtype(np.int16), -1), (np.dtype(np.float32), None), (np.dtype(np.uint8), 0)):
        got = est.predict_chunks(iter(feed), nodata=NODATA, layout=layout, out_dtype=dt, scale=10.0, offset=0.5,
                                 out_nodata=fill)
        np.testing.assert_array_equal(got, restate_pred(ref64, dt, 10.0, 0.5, fill, bands, t))
        assert_record(est, 1, SIZES[-1], 0, 0, CODE[dt], t * dt.itemsize)


def test_one_dimensional_y(E):
    import sknnr_amd

    rng = np.random.default_rng(3)
    x = rng.integers(-40, 40, size=(N_REF, D)).astype(np.float64)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K).fit(x, rng.random(N_REF) * 300.0)
    tiles = make_tiles(np.int16, False, seed=2)
    ref = est.predict_chunks(iter(tiles))
    assert ref.shape == (sum(SIZES),)
    for layout, feed in (("rows", tiles), ("bands", as_bands(tiles))):
        got = est.predict_chunks(iter(feed), layout=layout, out_dtype=np.uint8, scale=[0.5])
        assert got.shape == ref.shape and got.dtype == np.uint8
        np.testing.assert_array_equal(got, NR.narrow_values(ref[:, None], np.uint8, [0.5], [0.0])[:, 0])
        out = np.zeros(sum(SIZES), dtype=np.uint8)
        est.predict_chunks(iter(feed), layout=layout, out_dtype=np.uint8, scale=[0.5], out=out)
        np.testing.assert_array_equal(out, got)


@pytest.mark.parametrize("layout", ["rows", "bands"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("index_dtype, distance_dtype", [(np.int32, np.float32), (np.int32, None), (None, np.float32)])
def test_kneighbors_chunks_typed(E, index_dtype, distance_dtype, ids, masked, layout):
    est = E(3)
    bands = layout == "bands"
    total = sum(SIZES)
    idt = np.dtype(np.int64 if index_dtype is None else index_dtype)
    ddt = np.dtype(np.float64 if distance_dtype is None else distance_dtype)
    for in_dtype in (np.float64, np.int16):
        tiles = make_tiles(in_dtype, masked, seed=4)
        feed = as_bands(tiles) if bands else tiles
        kw = dict(layout=layout, return_dataframe_index=ids)
        if masked:
            kw.update(nodata=NODATA, fill_index=-7)
        ref_d, ref_i = reference(("nbr", np.dtype(in_dtype), ids, masked, layout),
                                 lambda: est.kneighbors_chunks(iter(feed), **kw))
        assert ref_i.dtype == np.int64 and ref_d.dtype == np.float64
        if masked:
            assert (ref_i == -7).any() and np.isnan(ref_d).any()
        if ids:
            assert ((ref_i >= 5000) | (ref_i == -7)).all()
        typed = dict(index_dtype=index_dtype, distance_dtype=distance_dtype)
        dist, idx = est.kneighbors_chunks(iter(feed), **kw, **typed)
        assert idx.dtype == idt and dist.dtype == ddt and idx.shape == ref_i.shape
        np.testing.assert_array_equal(idx, ref_i.astype(idt))
        with np.errstate(over="ignore"):
            np.testing.assert_array_equal(dist, ref_d.astype(ddt))
        assert_record(est, 1, SIZES[-1], CODE[idt], CODE[ddt], 0, K * (idt.itemsize + ddt.itemsize))
        shape = (K, total) if bands else (total, K)
        out = (np.full(shape, -1.0, dtype=ddt), np.full(shape, -5, dtype=idt))
        est.kneighbors_chunks(iter(feed), out=out, **kw, **typed)
        np.testing.assert_array_equal(out[1], ref_i.astype(idt))
        np.testing.assert_array_equal(out[0], ref_d.astype(ddt))
        only = est.kneighbors_chunks(iter(feed), return_distance=False, **kw, **typed)
        np.testing.assert_array_equal(only, ref_i.astype(idt))
        if index_dtype is not None:
            assert_record(est, 1, SIZES[-1], CODE[idt], 0, 0, K * idt.itemsize)


def test_forest_estimator():
    import sknnr_amd

    rng = np.random.default_rng(11)
    x_ref = rng.integers(-300, 300, size=(N_REF, 6)).astype(np.float64)
    y = np.abs(x_ref[:, :2]) + 0.1 * rng.standard_normal((N_REF, 2))
    est = sknnr_amd.RFNNRegressor(n_estimators=3, n_neighbors=K, random_state=0).fit(x_ref, y)
    assert est._map_on_device()
    x = rng.integers(-300, 300, size=(957, 6)).astype(np.int16)
    x[::5, 2] = NODATA
    rows = [x[:257], x[257:]]
    for layout, feed in (("rows", rows), ("bands", as_bands(rows))):
        ref = est.predict_chunks(iter(feed), nodata=NODATA, layout=layout)
        got = est.predict_chunks(iter(feed), nodata=NODATA, layout=layout, out_dtype=np.uint16, scale=100.0, out_nodata=65535)
        np.testing.assert_array_equal(got, restate_pred(ref, np.uint16, 100.0, 0.0, 65535, layout == "bands", 2))
        assert_record(est.regressor_, 1, 700, 0, 0, 3, 2 * 2)
        ref_d, ref_i = est.kneighbors_chunks(iter(feed), nodata=NODATA, fill_index=-1, layout=layout)
        dist, idx = est.kneighbors_chunks(iter(feed), nodata=NODATA, fill_index=-1, layout=layout, index_dtype=np.int32,
                                          distance_dtype=np.float32)
        np.testing.assert_array_equal(idx, ref_i.astype(np.int32))
        np.testing.assert_array_equal(dist, ref_d.astype(np.float32))


def test_transformed_estimator(moscow):
    import sknnr_amd

    est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=K).fit(moscow["X_train"], moscow["y_train"])
    x = np.ascontiguousarray(np.concatenate([moscow["X_test"], moscow["X_train"]]), dtype=np.float32)
    x[::4, 1] = np.nan
    rows = [x[:50], x[50:]]
    t = np.asarray(moscow["y_train"]).shape[1]
    scale = np.linspace(1.0, 20.0, t)
    for layout, feed in (("rows", rows), ("bands", as_bands(rows))):
        ref = est.predict_chunks(iter(feed), nodata=np.nan, layout=layout)
        assert np.isnan(ref).any()
        got = est.predict_chunks(iter(feed), nodata=np.nan, layout=layout, out_dtype=np.int16, scale=scale, offset=1.0,
                                 out_nodata=-32768)
        np.testing.assert_array_equal(got, restate_pred(ref, np.int16, scale, np.full(t, 1.0), -32768, layout == "bands", t))
        assert_record(est.regressor_, 1, x.shape[0] - 50, 0, 0, 2, t * 2)
        ref_d, ref_i = est.kneighbors_chunks(iter(feed), layout=layout, nodata=np.nan)
        dist, idx = est.kneighbors_chunks(iter(feed), layout=layout, nodata=np.nan, index_dtype="int32",
                                          distance_dtype="float32")
        np.testing.assert_array_equal(idx, ref_i.astype(np.int32))
        np.testing.assert_array_equal(dist, ref_d.astype(np.float32))


def test_query_stream_set_output(E):
    """The native stream alone: typed pushes, mixed layouts, and the refusals of ``set_output``."""
    from sknnr_amd import _native

    est = E(3)
    eng = est.engine_
    tiles = make_tiles(np.float64, False, seed=6)
    ref = est.predict_chunks(iter([tiles[4], tiles[3]]))  # (the same tiles at the same row positions)
    stream = eng.open_stream(K, weights="uniform", want_dist=False,
                             output=dict(pred_dtype=np.int16, scale=np.full(3, 2.0), offset=np.zeros(3), fill=-1))
    with stream:
        assert stream.pred_dtype == np.int16 and stream.idx_dtype == np.int64
        a = stream.push(tiles[4], need_idx=False)[2]
        b = stream.push_planes(list(np.ascontiguousarray(tiles[3].T)), need_idx=False)[2]
        with pytest.raises(_native.HipBackendError, match="only before the first push"):
            stream.set_output(pred_dtype=np.uint8)
        stream.flush()
    assert a.dtype == np.int16 and a.shape == (700, 3) and b.dtype == np.int16 and b.shape == (3, 257)
    np.testing.assert_array_equal(a, NR.narrow_values(ref[:700], np.int16, np.full(3, 2.0), np.zeros(3), -1))
    np.testing.assert_array_equal(b, NR.narrow_values(ref[700:], np.int16, np.full(3, 2.0), np.zeros(3), -1).T)
    stream = eng.open_stream(K, weights=None, want_dist=True)
    with stream:
        with pytest.raises(_native.HipBackendError, match="opened without predictions"):
            stream.set_output(pred_dtype=np.int16)
        with pytest.raises(ValueError, match="no narrow output type"):
            stream.set_output(index_dtype=np.float64)
        with pytest.raises(_native.HipBackendError, match="idx_dtype"):
            stream.set_output(index_dtype=np.int16)
        with pytest.raises(_native.HipBackendError, match="dist_dtype"):
            stream.set_output(distance_dtype=np.int32)


def test_parent_path_is_untouched(E):
    """A call without the new arguments: no conversion kernel, the same copies, the same results."""
    est = E(3)
    tiles = make_tiles(np.int16, True, seed=5)
    typed = est.predict_chunks(iter(tiles), nodata=NODATA, out_dtype=np.int16, out_nodata=-1)
    assert est.engine_._index.debug_last_narrow()["ran"] == 1
    pred = est.predict_chunks(iter(tiles), nodata=NODATA)
    rec = est.engine_._index.debug_last_narrow()
    assert rec == {"ran": 0, "rows": SIZES[-1], "idx_dtype": 0, "dist_dtype": 0, "pred_dtype": 0,
                   "d2h_bytes": SIZES[-1] * 3 * 8, "wide_mask": 0, "reserved": 0}, rec
    assert pred.dtype == np.float64
    np.testing.assert_array_equal(typed, NR.narrow_values(pred, np.int16, fill=-1))
    # what the call returned before: the one-shot predict of the valid rows, NaN elsewhere
    x = np.concatenate(tiles)
    valid = ~(x == NODATA).any(axis=1)
    np.testing.assert_array_equal(pred[valid], est.predict(x[valid].astype(np.float64)))
    assert np.isnan(pred[~valid]).all()
    dist, idx = est.kneighbors_chunks(iter(tiles), nodata=NODATA)
    rec = est.engine_._index.debug_last_narrow()
    assert rec["ran"] == 0 and rec["d2h_bytes"] == SIZES[-1] * K * 16 and idx.dtype == np.int64 and dist.dtype == np.float64
    want_d, want_i = est.kneighbors(x[valid].astype(np.float64))
    np.testing.assert_array_equal(idx[valid], want_i)
    np.testing.assert_array_equal(dist[valid], want_d)


_ALL_LANES_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
import sknnr_amd
import _narrow as NR
import test_raster_layout_gpu as RL
K, T, D, N_REF, NODATA = 5, 3, 7, 400, 5
rng = np.random.default_rng(21)
y = np.stack([rng.standard_normal(N_REF) * 50.0 + 100.0, rng.integers(0, 5, size=N_REF) * 40.0 + 3.0,
              rng.random(N_REF) * 200.0], axis=1)
est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(RL.lattice(N_REF, D, 107).astype(np.uint8), y)
sizes = (1, 300, 1024, 2500, 7000)  # (7,000 pixels: seven tiles of at most 1,024 through the four slots)
bands, rows = RL.band_tiles(seed=30, sizes=sizes)
total = sum(sizes)
X = np.concatenate(rows).astype(np.float64)
valid = ~(X == NODATA).any(axis=1)
ends = np.cumsum(sizes)
partly = [0 < valid[e - n:e].sum() < n for n, e in zip(sizes, ends)]
assert sum(partly) >= 3 and not all(partly), partly
# the yardsticks: untiled float64 calls on device tensors (they do not pass through the host pipeline)
dev = lambda a: torch.as_tensor(a, device="cuda")
host = lambda a: a.cpu().numpy()
stat = ["mean", "mode", "max"]
d_v, i_v = (host(a) for a in est.kneighbors(dev(X[valid])))
want_d, want_i, want_s = np.full((total, K), np.nan), np.full((total, K), -7, dtype=np.int64), np.full((total, T), np.nan)
want_d[valid], want_i[valid], want_s[valid] = d_v, i_v, host(est.summarize(dev(X[valid]), stat))
all_d, all_i = (host(a) for a in est.kneighbors(dev(X)))
all_p = host(est.predict(dev(X)))
index = est.engine_._index

# (a) neighbours: band-first, masked, int32 / float32, into the caller's arrays
row_d, row_i = est.kneighbors_chunks(iter([r.astype(np.float64) for r in rows]), nodata=NODATA, fill_index=-7)
np.testing.assert_array_equal(row_i, want_i)
np.testing.assert_array_equal(row_d, want_d)
out_d, out_i = np.full((K, total), 9, dtype=np.float32), np.full((K, total), 9, dtype=np.int32)
est.kneighbors_chunks(iter(bands), layout="bands", nodata=NODATA, fill_index=-7, index_dtype=np.int32,
                      distance_dtype=np.float32, out=(out_d, out_i))
np.testing.assert_array_equal(out_i, NR.narrow_indices(want_i).T)
np.testing.assert_array_equal(out_d, NR.narrow_values(want_d, np.float32).T)
assert (out_i[:, ~valid] == -7).all() and np.isnan(out_d[:, ~valid]).all() and not np.isnan(out_d[:, valid]).any()
rec = index.debug_last_narrow()
assert rec["ran"] == 1 and rec["rows"] <= 1024 and (rec["idx_dtype"], rec["dist_dtype"], rec["pred_dtype"]) == (5, 1, 0), rec
assert rec["d2h_bytes"] == rec["rows"] * K * (4 + 4), rec

# (b) summaries: band-first, masked, int16 with a scale and an offset per target
scale, offset = np.array([10.0, 1.0, 0.25]), np.array([0.5, -3.0, 100.0])
out_p = np.zeros((T, total), dtype=np.int16)
est.predict_chunks(iter(bands), layout="bands", nodata=NODATA, out=out_p, out_dtype=np.int16, scale=scale, offset=offset,
                   out_nodata=-32768, statistic=stat)
np.testing.assert_array_equal(out_p, NR.narrow_values(want_s, np.int16, scale, offset, -32768).T)
assert (out_p[:, ~valid] == -32768).all()
rec = index.debug_last_narrow()
assert (rec["idx_dtype"], rec["dist_dtype"], rec["pred_dtype"]) == (0, 0, 2) and rec["d2h_bytes"] == rec["rows"] * T * 2, rec

# (c) one stream, three typed outputs of three shapes and three widths, rows and planes in turn
scale, offset = np.array([1.0, 0.5, 0.75]), np.array([0.0, 10.0, -5.0])
eng = est.engine_
stream = eng.open_stream(K, weights="distance", want_dist=True, decimals=est.DISTANCE_PRECISION_DECIMALS,
                         formula=est._formula(), check_finite=True, query_dtype=eng.query_dtype_code(rows[0], est._formula(), False),
                         output=dict(index_dtype=np.int32, distance_dtype=np.float32, pred_dtype=np.uint8, scale=scale,
                                     offset=offset))
got, row = [], 0
for i, (b, r) in enumerate(zip(bands, rows)):
    n = r.shape[0]
    if i % 2:
        got.append((False, row, n) + stream.push(r))
    else:
        got.append((True, row, n) + stream.push_planes([np.asarray(b[j]).reshape(-1) for j in range(D)]))
    row += n
rec = index.debug_last_narrow()
assert (rec["idx_dtype"], rec["dist_dtype"], rec["pred_dtype"]) == (5, 1, 4) and rec["rows"] <= 1024, rec
assert stream.close() == total
assert index.debug_last_narrow()["d2h_bytes"] == rec["rows"] * (K * 4 + K * 4 + T * 1)
for planes, r0, n, idx, dist, pred in got:
    fix = (lambda a: a.T) if planes else (lambda a: a)
    assert (idx.dtype, dist.dtype, pred.dtype) == (np.int32, np.float32, np.uint8)
    assert idx.shape == dist.shape == ((K, n) if planes else (n, K)) and pred.shape == ((T, n) if planes else (n, T))
    np.testing.assert_array_equal(fix(idx), NR.narrow_indices(all_i[r0:r0 + n]))
    np.testing.assert_array_equal(fix(dist), NR.narrow_values(all_d[r0:r0 + n], np.float32))
    np.testing.assert_array_equal(fix(pred), NR.narrow_values(all_p[r0:r0 + n], np.uint8, scale, offset))
print("ok", total, int(valid.sum()))
"""


def test_all_lanes_differ():
    """The three outputs differ in everything at once -- k = 5 against t = 3 columns, 4 / 4 / 1 and 4 / 4 / 2 bytes per
    element -- band-first, masked and with per-target statistics, through more pipeline tiles than slots
    (SKNNR_HOST_CHUNK_ROWS=1024, read once per process: a child runs it).  Every expectation is an untiled float64 call
    on device tensors, narrowed by tests/_narrow.py."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SKNNR_HOST_CHUNK_ROWS="1024")
    env.pop("SKNNR_PIPE_NO_RAMP", None)
    run = subprocess.run([sys.executable, "-c", _ALL_LANES_CHILD.format(root=root, tests=os.path.join(root, "tests"))],
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1].startswith("ok 10825 "), run.stdout[-500:]
