"""Streamed calls end to end: dataframe ids looked up on the device (``kneighbors_chunks(return_dataframe_index=True)``)
and neighbours beside predictions from one stream (``predict_chunks(return_neighbors=True)``).

300 reference rows of 6 integer-valued features, t = 3, k of 1 and 5, a dataframe index of shuffled int64 ids (some
beyond 2^31 for the int64 outputs, all inside int32 for the int32 ones), tiles of 1, 257, 0, 1000 and 300 rows as int16,
for ``RawKNNRegressor``, ``EuclideanKNNRegressor`` and ``RFNNRegressor``; both layouts, ``index_dtype`` None and int32,
``out`` given or not; with ``nodata`` the 300-row tile is fully valid, the 1-row tile fully masked, the others about
30 % masked, ``fill_index`` -1 and 0.

The expectation is always the host flow restated here: the SAME call with ``return_dataframe_index=False``, then
tests/_id_table.py; ``predict_chunks(return_neighbors=True)`` is compared with separate ``kneighbors_chunks`` and
``predict_chunks`` calls.  Everything is ``assert_array_equal``.  After each call with ids
``sknnr_debug_last_narrow`` out[7] (the field ``reserved`` of ``debug_last_narrow()``) must be 1, and 0 after a call
without.

Without the feature every test here fails: ``predict_chunks`` has no ``return_neighbors``, and out[7] stays 0.

Measured on an MI355X: the 66 cases of this module take 8.4 s, of which 3.5 s are the first case's device set-up and 3.8 s
the child process; no other case takes more than 0.05 s.
"""

from __future__ import annotations

import numpy as np
import pytest

import _id_table as IT

pytestmark = pytest.mark.gpu

N_REF, D, T = 300, 6, 3
SIZES = (1, 257, 0, 1000, 300)
TOTAL = sum(SIZES)
NODATA = -9999
ESTIMATORS = ("raw", "euclidean", "rfnn")


def make_ids(small):
    """Shuffled int64 ids, one per reference row; ``small``: inside int32, else some beyond 2^31 and some negative."""
    rng = np.random.default_rng(3)
    ids = rng.permutation(N_REF).astype(np.int64) * 7 + 1000
    if not small:
        ids[::3] += 2**33
        ids[1::5] *= -1
    return ids


def make_tiles(masked):
    rng = np.random.default_rng(50)
    tiles = []
    for n in SIZES:
        x = rng.integers(-300, 300, size=(n, D)).astype(np.int16)
        if masked and n not in (0, 300):  # (the 300-row tile stays fully valid)
            rows = np.flatnonzero(rng.random(n) < 0.3) if n > 1 else np.array([0])
            x[rows, rng.integers(0, D, size=rows.size)] = NODATA
        tiles.append(x)
    return tiles


def feed_of(tiles, bands):
    return [np.ascontiguousarray(t.T) for t in tiles] if bands else tiles


_MADE = {}


def estimator(name, k, ids_kind="big"):
    """One fitted estimator per (class, k, kind of dataframe index), made once per module."""
    import pandas as pd
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    key = (name, k, ids_kind)
    if key not in _MADE:
        rng = np.random.default_rng(11)
        x_ref = rng.integers(-300, 300, size=(N_REF, D)).astype(np.float64)
        y = np.stack([np.abs(x_ref[:, 0]) + 0.1 * rng.standard_normal(N_REF), rng.random(N_REF) * 500.0 - 100.0,
                      rng.integers(0, 5, size=N_REF) * 40.0 + 3.0], axis=1)
        index = {"big": make_ids(False), "small": make_ids(True), "int32": make_ids(True).astype(np.int32),
                 "str": np.array([f"plot{i:04d}" for i in make_ids(True)])}[ids_kind]
        frame = pd.DataFrame(x_ref, index=index)
        if name == "raw":
            est = sknnr_amd.RawKNNRegressor(n_neighbors=k).fit(frame, y)
        elif name == "euclidean":
            est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=k).fit(frame, y)
        else:
            est = sknnr_amd.RFNNRegressor(n_estimators=3, n_neighbors=k, random_state=0).fit(frame, y)
        if name != "raw":
            assert est._map_on_device()
        _MADE[key] = est
    return _MADE[key]


def regressor(est):
    return getattr(est, "regressor_", est)


def record(est):
    return regressor(est).engine_._index.debug_last_narrow()


def shaped(n_cols, bands, dtype, value, extra=0):
    return np.full((n_cols, TOTAL + extra) if bands else (TOTAL + extra, n_cols), value, dtype=dtype)


@pytest.mark.parametrize("fill", [None, -1, 0])  # (None: no nodata mask)
@pytest.mark.parametrize("layout", ["rows", "bands"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name", ESTIMATORS)
def test_kneighbors_chunks_ids_on_the_device(name, k, layout, fill):
    bands = layout == "bands"
    masked = fill is not None
    feed = feed_of(make_tiles(masked), bands)
    kw = dict(n_neighbors=k, layout=layout)
    if masked:
        kw.update(nodata=NODATA, fill_index=fill)
    for index_dtype in (None, np.int32):
        est = estimator(name, 5, "big" if index_dtype is None else "small")
        table = regressor(est).dataframe_index_in_
        assert table.dtype == np.int64
        # today's host flow: the row indices of the same call (masked rows -1), then the restated lookup
        raw_kw = dict(kw, fill_index=-1) if masked else kw
        ref_d, ref_i = est.kneighbors_chunks(iter(feed), **raw_kw)
        assert record(est)["reserved"] == 0
        odt = np.dtype(np.int64 if index_dtype is None else index_dtype)
        want = IT.lookup(ref_i, table, -1 if fill is None else fill, odt)
        if masked:
            assert (ref_i < 0).any() and (ref_i[..., -300:] if bands else ref_i[-300:]).min() >= 0
        typed = {} if index_dtype is None else dict(index_dtype=index_dtype)
        dist, idx = est.kneighbors_chunks(iter(feed), return_dataframe_index=True, **kw, **typed)
        rec = record(est)
        assert rec["reserved"] == 1 and rec["ran"] == 1 and rec["rows"] == 300, rec
        assert rec["idx_dtype"] == (0 if index_dtype is None else 5) and rec["d2h_bytes"] == 300 * k * (odt.itemsize + 8), rec
        assert idx.dtype == odt and dist.dtype == np.float64
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(dist, ref_d)
        # into the caller's arrays, five pixels longer than the call: the tail stays as it was
        o_d, o_i = shaped(k, bands, np.float64, 7.5, 5), shaped(k, bands, odt, 77, 5)
        got_d, got_i = est.kneighbors_chunks(iter(feed), return_dataframe_index=True, out=(o_d, o_i), **kw, **typed)
        assert record(est)["reserved"] == 1
        body = (lambda a: a[:, :TOTAL]) if bands else (lambda a: a[:TOTAL])
        tail = (lambda a: a[:, TOTAL:]) if bands else (lambda a: a[TOTAL:])
        np.testing.assert_array_equal(body(o_i), want)
        np.testing.assert_array_equal(body(o_d), ref_d)
        np.testing.assert_array_equal(got_i, want)
        assert np.shares_memory(got_i, o_i) and (tail(o_i) == 77).all() and (tail(o_d) == 7.5).all()
        only = est.kneighbors_chunks(iter(feed), return_dataframe_index=True, return_distance=False, **kw, **typed)
        np.testing.assert_array_equal(only, want)


@pytest.mark.parametrize("ids_kind", ["int32", "str"])
@pytest.mark.parametrize("masked", [False, True])
def test_other_tables_give_what_they_gave(ids_kind, masked):
    """An int32-typed index takes the device lookup and its one ``astype``; string labels stay on the host."""
    est = estimator("raw", 5, ids_kind)
    table = est.dataframe_index_in_
    feed = make_tiles(masked)
    kw = dict(nodata=NODATA, fill_index=-1) if masked else {}
    _, ref_i = est.kneighbors_chunks(iter(feed), **kw)
    for fill in ((-1, 0) if masked else (None,)):
        gone = ref_i < 0
        want = table[np.where(gone, 0, ref_i)]  # (the host flow this call used to run, restated)
        if masked:
            want[gone] = fill
        call = dict(kw, fill_index=fill) if masked else kw
        _, idx = est.kneighbors_chunks(iter(feed), return_dataframe_index=True, **call)
        assert idx.dtype == table.dtype == want.dtype
        np.testing.assert_array_equal(idx, want)
        assert record(est)["reserved"] == (1 if ids_kind == "int32" else 0)
    if ids_kind == "int32":  # an int32 output of an int32 table stays int32
        _, idx = est.kneighbors_chunks(iter(feed), return_dataframe_index=True, index_dtype=np.int32, **kw)
        np.testing.assert_array_equal(idx, IT.lookup(ref_i, table, -1, np.int32))
        assert idx.dtype == np.int32


STAT = ["mean", "std", "mode"]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layout", ["rows", "bands"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name", ESTIMATORS)
def test_predict_chunks_with_neighbors_is_the_two_calls(name, k, layout, masked):
    bands = layout == "bands"
    est = estimator(name, k, "small")
    feed = feed_of(make_tiles(masked), bands)
    base = dict(layout=layout, **(dict(nodata=NODATA) if masked else {}))
    body = (lambda a: a[:, :TOTAL]) if bands else (lambda a: a[:TOTAL])
    tail = (lambda a: a[:, TOTAL:]) if bands else (lambda a: a[TOTAL:])

    # (a) nothing typed: float64 predictions, float64 distances, int64 row indices
    want_p = est.predict_chunks(iter(feed), **base)
    want_d, want_i = est.kneighbors_chunks(iter(feed), **base)
    pred, dist, idx = est.predict_chunks(iter(feed), return_neighbors=True, **base)
    assert record(est)["reserved"] == 0
    for got, want in ((pred, want_p), (dist, want_d), (idx, want_i)):
        assert got.dtype == want.dtype and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
    if masked:
        assert np.isnan(want_p).any() and (want_i == -1).any()

    # (b) everything at once: typed summaries, typed distances, int32 dataframe ids, all into the caller's arrays
    fill = dict(fill_index=0) if masked else {}
    p_kw = dict(out_dtype=np.int16, scale=100, out_nodata=-32768, statistic=STAT)
    n_kw = dict(index_dtype=np.int32, distance_dtype=np.float32, return_dataframe_index=True, **fill)
    want_p = est.predict_chunks(iter(feed), **base, **p_kw)
    want_d, want_i = est.kneighbors_chunks(iter(feed), **base, **n_kw)
    assert want_p.dtype == np.int16 and want_d.dtype == np.float32 and want_i.dtype == np.int32
    o_p, o_d, o_i = shaped(T, bands, np.int16, 99, 5), shaped(k, bands, np.float32, 7.5, 5), shaped(k, bands, np.int32, 77, 5)
    pred, dist, idx = est.predict_chunks(iter(feed), out=o_p, return_neighbors=True, neighbors_out=(o_d, o_i), **base,
                                         **p_kw, **n_kw)
    rec = record(est)
    assert rec["reserved"] == 1 and (rec["idx_dtype"], rec["dist_dtype"], rec["pred_dtype"]) == (5, 1, 2), rec
    assert rec["rows"] == 300 and rec["d2h_bytes"] == 300 * (k * 4 + k * 4 + T * 2), rec
    for got, o_, want, stays in ((pred, o_p, want_p, 99), (dist, o_d, want_d, 7.5), (idx, o_i, want_i, 77)):
        assert np.shares_memory(got, o_)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(body(o_), want)
        assert (tail(o_) == stays).all()

    # (c) without distances; and neighbors_out without a distance array: what has no array is collected (row layout --
    # the planes of a band-first tile leave with one stride, so there the arrays come all or none, as for ``out`` of
    # kneighbors_chunks)
    pred, idx = est.predict_chunks(iter(feed), return_neighbors=True, return_distance=False, **base, **p_kw, **n_kw)
    np.testing.assert_array_equal(pred, want_p)
    np.testing.assert_array_equal(idx, want_i)
    o_i[...] = 77
    if bands:
        o_p[...] = 99
        pred, idx = est.predict_chunks(iter(feed), out=o_p, return_neighbors=True, return_distance=False,
                                       neighbors_out=(None, o_i), **base, **p_kw, **n_kw)
        assert np.shares_memory(pred, o_p) and np.shares_memory(idx, o_i)
    else:
        pred, dist, idx = est.predict_chunks(iter(feed), return_neighbors=True, neighbors_out=(None, o_i), **base, **p_kw,
                                             **n_kw)
        np.testing.assert_array_equal(dist, want_d)
    np.testing.assert_array_equal(body(o_i), want_i)
    np.testing.assert_array_equal(pred, want_p)
    assert (tail(o_i) == 77).all()
    # ... and the call without return_neighbors is what it was
    np.testing.assert_array_equal(est.predict_chunks(iter(feed), **base, **p_kw), want_p)


def test_native_stream_refuses_a_late_or_wrong_table():
    from sknnr_amd import _native

    est = estimator("raw", 5, "small")
    eng = est.engine_
    tile = make_tiles(False)[1].astype(np.float64)
    table = est.dataframe_index_in_
    with eng.open_stream(5, formula=est._formula(), decimals=est.DISTANCE_PRECISION_DECIMALS) as stream:
        with pytest.raises(_native.HipBackendError, match="reference rows"):
            stream.set_id_table(table[:-1])
        idx0, _, _ = stream.push(tile)
        with pytest.raises(_native.HipBackendError, match="only before the first push"):
            stream.set_id_table(table)
        stream.flush()
    with eng.open_stream(5, formula=est._formula(), decimals=est.DISTANCE_PRECISION_DECIMALS, id_table=table) as stream:
        idx1, _, _ = stream.push(tile)
        stream.flush()
    assert (idx0 >= 0).all()
    np.testing.assert_array_equal(idx1, table[idx0])


_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import pandas as pd
import torch
import sknnr_amd
import _id_table as IT
import _narrow as NR
K, T, D, N_REF, NODATA, N = 5, 3, 7, 400, 5, 10825
rng = np.random.default_rng(21)
ids = rng.permutation(N_REF).astype(np.int64) * 11 + 90000
x_ref = pd.DataFrame(rng.integers(0, 40, size=(N_REF, D)).astype(np.float64), index=ids)
y = np.stack([rng.random(N_REF) * 250.0, rng.integers(0, 5, size=N_REF) * 40.0 + 3.0, rng.random(N_REF) * 100.0], axis=1)
est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(x_ref, y)
X = rng.integers(0, 40, size=(N, D)).astype(np.uint8)
X[rng.random(N) < 0.3, 3] = NODATA
X[2048:3072] = np.where(X[2048:3072] == NODATA, 6, X[2048:3072])  # one pipeline tile fully valid ...
X[4096:5120, 0] = NODATA                                         # ... and one fully masked
valid = ~(X == NODATA).any(axis=1)
bands = np.ascontiguousarray(X.T)
# the yardstick: untiled float64 calls on device tensors (they do not pass through the host pipeline), then the restatement
dev = lambda a: torch.as_tensor(a, device="cuda")
host = lambda a: a.cpu().numpy()
Xv = X[valid].astype(np.float64)
d_v, i_v = (host(a) for a in est.kneighbors(dev(Xv)))
want_i, want_p = np.full((N, K), -1, dtype=np.int64), np.full((N, T), np.nan)
want_i[valid], want_p[valid] = i_v, host(est.predict(dev(Xv)))
want_ids = IT.lookup(want_i, ids, 0, np.int32).T
want_u8 = NR.narrow_values(want_p, np.uint8, fill=255).T
o_p, o_i = np.full((T, N + 3), 9, dtype=np.uint8), np.full((K, N + 3), 9, dtype=np.int32)
pred, idx = est.predict_chunks([bands], layout="bands", nodata=NODATA, out=o_p, out_dtype=np.uint8, out_nodata=255,
                               return_neighbors=True, return_distance=False, return_dataframe_index=True, fill_index=0,
                               index_dtype=np.int32, neighbors_out=(None, o_i))
rec = est.engine_._index.debug_last_narrow()
assert rec["reserved"] == 1 and rec["rows"] <= 1024 and (rec["idx_dtype"], rec["pred_dtype"]) == (5, 4), rec
assert rec["d2h_bytes"] == rec["rows"] * (K * 4 + T * 1), rec
np.testing.assert_array_equal(idx, want_ids)
np.testing.assert_array_equal(pred, want_u8)
np.testing.assert_array_equal(o_i[:, :N], want_ids)
assert (o_i[:, N:] == 9).all() and (o_p[:, N:] == 9).all()
assert (idx[:, ~valid] == 0).all() and (pred[:, ~valid] == 255).all()
# the same neighbours from kneighbors_chunks, as int64 ids this time (the lookup-only kernels, more tiles than slots)
_, idx64 = est.kneighbors_chunks([bands], layout="bands", nodata=NODATA, fill_index=0, return_dataframe_index=True)
np.testing.assert_array_equal(idx64, IT.lookup(want_i, ids, 0).T)
print("ok", N, int(valid.sum()))
"""


def test_more_pipeline_tiles_than_slots_carry_the_table():
    """A 10,825-pixel push, band-first and masked, ids as int32 and predictions as uint8, through pipeline tiles of at most
    1,024 rows (SKNNR_HOST_CHUNK_ROWS=1024, read once per process: a child runs it), so that every slot is reused with
    the table in place."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SKNNR_HOST_CHUNK_ROWS="1024")
    env.pop("SKNNR_PIPE_NO_RAMP", None)
    run = subprocess.run([sys.executable, "-c", _CHILD.format(root=root, tests=os.path.join(root, "tests"))],
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1].startswith("ok 10825 "), run.stdout[-500:]
