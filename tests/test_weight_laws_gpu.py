"""Distance-weight laws on the device, end to end: the law kernel alone, one-shot ``predict`` / ``summarize``, streamed
``predict_chunks`` with every raster feature, and the refusals that remain.

The yardstick of the kernel is the law's own numpy ``__call__``.  The yardstick of every estimator call is the SAME
estimator fitted with ``weights=lambda d: law(d)`` -- a plain callable, so the host path that this feature leaves
untouched -- and, for ``predict``, scikit-learn's own reduction (tests/_predict_ref.py) on the estimator's ``kneighbors``.
Streamed calls are compared with the lambda estimator's one-shot call on the valid rows of ``np.concatenate(tiles)``,
through the typed-output restatement (tests/_narrow.py) where the output is typed, and their neighbours with
``kneighbors_chunks``.  Every comparison is ``assert_array_equal`` (NaN positions equal).

Fit set: 1,500 rows of the 4-D integer lattice of test_neighbor_summary_gpu.py (exact ties, zero distances); queries on
the lattice, a quarter of them moved half a step along one axis so that distances between the lattice's own occur.

``sknnr_debug_last_weight_law`` must show the law's code, the rows and ``ran == 1`` after a law call and ``ran == 0``
after a lambda call: the device path was taken.  Without the feature nothing here passes: there is no
``sknnr_amd.weights``.
"""

from __future__ import annotations

import numpy as np
import pytest

import _narrow as NR
from _predict_ref import crafted_neighbours, sklearn_predict

pytestmark = pytest.mark.gpu

N_REF, D, K, N_Q = 1500, 4, 5, 2000
SIZES = (1, 255, 256, 257, 1000)
TOTAL = sum(SIZES)
NODATA = -9999.0
STAT = ["mean", "std", "mode"]
TINY = np.nextafter(0.0, 1.0)


def W():
    from sknnr_amd import weights

    return weights


def all_laws():
    w = W()
    return [w.InverseDistance(1.0), w.InverseDistance(0.25), w.InverseDistance(3.7), w.InverseSquaredDistance(1.0),
            w.InverseSquaredDistance(0.5), w.InverseSquaredDistance(1e-3), w.Triangular(1.0), w.Triangular(2.5),
            w.Triangular(0.3), w.Epanechnikov(1.0), w.Epanechnikov(2.5), w.Epanechnikov(0.3)]


def plain(law):
    """The law as a plain callable: today's host path."""
    return lambda d: law(d)


def lattice(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 6, size=(N_REF, D)).astype(np.float64)
    y = np.stack([rng.standard_normal(N_REF) * 50.0 + 100.0, rng.integers(0, 5, size=N_REF) * 40.0 + 3.0,
                  rng.random(N_REF) * 200.0], axis=1)
    return x, y


def queries(n, rng, far=0.0):
    """``far``: that share of the rows lies outside the lattice's box, at least 2 from every reference row (each of
    the four coordinates at least one step beyond the box): the rows a compact law leaves without any weight."""
    q = rng.integers(0, 6, size=(n, D)).astype(np.float64)
    rows = np.flatnonzero(rng.random(n) < 0.25)
    q[rows, rng.integers(0, D, size=rows.size)] += 0.5
    if far:
        q[rng.random(n) < far] += 6.0
    return q


def make_tiles(masked=False, seed=1, far=0.0):
    """Tiles of SIZES rows; ``masked``: the 1-row tile is wholly nodata, about 25 % of the rows elsewhere."""
    rng = np.random.default_rng(seed)
    tiles = []
    for n in SIZES:
        q = queries(n, rng, far)
        if masked:
            rows = np.flatnonzero(rng.random(n) < 0.25) if n > 1 else np.array([0])
            q[rows, rng.integers(0, D, size=rows.size)] = NODATA
        tiles.append(q)
    return tiles


def as_bands(tiles):
    return [np.ascontiguousarray(t.T) for t in tiles]


_MADE = {}


def fit(weights, key, k=K, y_kind="f64x3", frame=False):
    """One fitted RawKNNRegressor per key, made once per module."""
    import pandas as pd
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    key = (key, k, y_kind, frame)
    if key not in _MADE:
        x, y = lattice()
        yy = {"f64x3": y, "f32x3": y.astype(np.float32), "f64": y[:, 0].copy()}[y_kind]
        xx = pd.DataFrame(x, index=np.random.default_rng(3).permutation(N_REF).astype(np.int64) * 7 + 1000) if frame else x
        _MADE[key] = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights).fit(xx, yy)
    return _MADE[key]


def record(est):
    return getattr(est, "regressor_", est).engine_._index.debug_last_weight_law()


def assert_law_ran(est, law, rows, k=None):
    rec = record(est)
    assert rec["law"] == law.code and rec["rows"] == rows and rec["ran"] == 1, rec
    if k is not None:
        assert rec["k"] == k, rec


def assert_no_law(est):
    rec = record(est)
    assert rec["law"] == 0 and rec["ran"] == 0, rec


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------
def kernel_distances(law, n, rng):
    p = law.params[0]
    crafted = np.array([0.0, TINY, 7 * TINY, 2.0**-1030, 1e-300, 1e308, p, np.nextafter(p, np.inf), np.nextafter(p, -np.inf),
                        0.1, 1.0 / 3.0, 1.0, 2.0, 1e155, 1.5e154])
    dist, _ = crafted_neighbours(100, n // 8 + 6, 8, rng)
    pool = np.concatenate([crafted, dist.ravel()])
    return pool[:n]


@pytest.mark.parametrize("law", all_laws(), ids=repr)
def test_kernel_alone(law):
    import torch
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    rng = np.random.default_rng(7)
    p0, p1 = law.params
    for n in (1, 255, 256, 257, 4099):
        d = kernel_distances(law, n, rng)
        assert d.shape == (n,)
        got = _native.debug_weight_law_host(law.code, p0, p1, d)
        assert got.dtype == np.float64 and got.shape == d.shape
        np.testing.assert_array_equal(got, law(d), err_msg=f"n = {n}")
    # one element at a time: each crafted value alone in a launch
    for v in kernel_distances(law, 15, rng):
        np.testing.assert_array_equal(_native.debug_weight_law_host(law.code, p0, p1, np.array([v])), law(np.array([v])))
    # device pointers, at an odd element offset; the elements outside the range stay as they were
    d = kernel_distances(law, 4099, rng)
    src = torch.as_tensor(np.concatenate([[5.0], d]), device="cuda")
    dst = torch.full((4101,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _native.debug_weight_law_device(law.code, p0, p1, src.data_ptr() + 8, 4099, dst.data_ptr() + 8)
    out = dst.cpu().numpy()
    np.testing.assert_array_equal(out[1:4100], law(d))
    assert out[0] == -7.0 and out[4100] == -7.0
    assert _native.debug_weight_law_host(law.code, p0, p1, np.empty((0, 5))).shape == (0, 5)


# ---- 2. one-shot calls -----------------------------------------------------------------------------------------------------
def one_shot(law, key, k, y_kind, far=0.0):
    import torch

    est, ref = fit(law, key, k, y_kind), fit(plain(law), key + "-plain", k, y_kind)
    X = queries(N_Q, np.random.default_rng(5), far)
    t = 1 if y_kind == "f64" else 3
    np.testing.assert_array_equal(est.independent_prediction_, ref.independent_prediction_)
    assert est.independent_prediction_.dtype == np.float64
    for kind in ("numpy", "cuda", "none"):
        Xq = {"numpy": X, "cuda": torch.as_tensor(X, device="cuda"), "none": None}[kind]
        host = (lambda a: a.cpu().numpy()) if kind == "cuda" else (lambda a: a)
        rows = N_REF if kind == "none" else N_Q
        with np.errstate(all="ignore"):
            want = host(ref.predict(Xq))
        assert_no_law(ref)
        got = est.predict(Xq)
        assert_law_ran(est, law, rows, k)
        if kind == "cuda":
            assert got.is_cuda and got.dtype == torch.float64
        got = host(got)
        assert got.dtype == np.float64 and got.shape == ((rows,) if t == 1 else (rows, t))
        np.testing.assert_array_equal(got, want, err_msg=f"predict {kind}")
        dist, idx = est.kneighbors(Xq)
        with np.errstate(all="ignore"):
            skl = sklearn_predict(est._y, host(dist), host(idx), weights=law)
        np.testing.assert_array_equal(got, skl, err_msg=f"predict {kind} against scikit-learn")
        for table in ([STAT] if t == 3 else [[s] for s in STAT]):
            with np.errstate(all="ignore"):
                want = host(ref.summarize(Xq, table))
            assert_no_law(ref)
            got = host(est.summarize(Xq, table))
            assert_law_ran(est, law, rows, k)
            assert got.dtype == np.float64
            np.testing.assert_array_equal(got, want, err_msg=f"summarize {table} {kind}")
    return est, ref, X


@pytest.mark.parametrize("y_kind", ["f64x3", "f32x3", "f64"])
@pytest.mark.parametrize("k", [1, 5, 8, 9, 24])
def test_one_shot_inverse_distance(k, y_kind):
    one_shot(W().InverseDistance(1.0), "inv1", k, y_kind)


@pytest.mark.parametrize("k, y_kind", [(5, "f64x3"), (9, "f32x3"), (24, "f64"), (8, "f64x3")])
def test_one_shot_inverse_squared(k, y_kind):
    one_shot(W().InverseSquaredDistance(0.5), "invsq.5", k, y_kind)


@pytest.mark.parametrize("k", [5, 9])
def test_one_shot_triangular_all_zero_rows(k):
    """Bandwidth 1.5, from the lattice's distance spectrum {0, 0.5, 1, sqrt(1.25), sqrt(2), 1.5, ...}: neighbours up to
    sqrt(2) have a weight, one at 1.5 (half a step and two whole ones) or beyond has none.  Every fitted row has
    another within sqrt(2) (1,500 rows in 1,296 cells), so the fit's own independent score is defined; a fifth of the
    queries lie outside the box, at least 2 from every row: their rows are all zero and they predict NaN, as
    scikit-learn does (0 / 0)."""
    law = W().Triangular(1.5)
    est, ref, X = one_shot(law, "tri1.5", k, "f64x3", far=0.2)
    assert not np.isnan(est.independent_prediction_).any()
    dist, _ = est.kneighbors(X)
    zero_rows = (law(dist) == 0.0).all(axis=1)
    assert zero_rows.any(), "the bandwidth leaves no all-zero row"
    assert zero_rows.sum() < len(X) / 2, "more than half of the rows are all zero: the comparison is mostly NaN"
    pred = est.predict(X)
    np.testing.assert_array_equal(np.isnan(pred).all(axis=1), zero_rows)
    np.testing.assert_array_equal(np.isnan(pred).any(axis=1), zero_rows)
    assert ((law(dist) > 0) & (law(dist) < 1)).any(), "weights strictly between 0 and 1 occur"
    mode = est.summarize(X, "mode")
    np.testing.assert_array_equal(np.isnan(mode).all(axis=1), zero_rows)  # (all votes zero: NaN, as `mode` defines it)


def test_one_shot_epanechnikov():
    one_shot(W().Epanechnikov(1.5), "epa1.5", 5, "f64x3")


def test_parameters_follow_the_estimator():
    """Two estimators, two laws, alternating calls: each handle holds its own parameters; a new law on one engine
    replaces the old."""
    w = W()
    a, b = fit(w.InverseDistance(1.0), "inv1"), fit(w.InverseSquaredDistance(0.5), "invsq.5")
    ra, rb = fit(plain(w.InverseDistance(1.0)), "inv1-plain"), fit(plain(w.InverseSquaredDistance(0.5)), "invsq.5-plain")
    X = queries(300, np.random.default_rng(8))
    for _ in range(2):
        np.testing.assert_array_equal(a.predict(X), ra.predict(X))
        np.testing.assert_array_equal(b.predict(X), rb.predict(X))
    eng = a.engine_
    for law in (w.InverseDistance(2.0), w.Triangular(3.0), w.InverseDistance(1.0)):
        got = eng.predict(X, K, law, formula=a._formula())
        dist, idx = a.kneighbors(X)
        np.testing.assert_array_equal(got, sklearn_predict(a._y, dist, idx, weights=law))
        assert_law_ran(a, law, len(X), K)


@pytest.mark.parametrize("kind", ["euclidean", "gnn", "rfnn"])
def test_transformed_estimators(moscow, kind):
    """The affine map (Euclidean, GNN) and the forest map with weighted-Hamming distances (RFNN) in front of the law."""
    import sknnr_amd

    law = W().InverseDistance(1.0)
    X, y = moscow["X_train"], moscow["y_train"]
    Xq = np.concatenate([moscow["X_test"], moscow["X_train"][:40]])

    def make(weights):
        if kind == "gnn":
            return sknnr_amd.GNNRegressor(n_neighbors=5, weights=weights).fit(X, y)
        if kind == "rfnn":
            return sknnr_amd.RFNNRegressor(n_neighbors=4, n_estimators=20, random_state=0, weights=weights).fit(X, y)
        return sknnr_amd.EuclideanKNNRegressor(n_neighbors=3, weights=weights).fit(X, y)

    est, ref = make(law), make(plain(law))
    t = y.shape[1]
    table = [STAT[j % 3] for j in range(t)]
    np.testing.assert_array_equal(est.independent_prediction_, ref.independent_prediction_)
    np.testing.assert_array_equal(est.predict(Xq), ref.predict(Xq))
    assert_law_ran(est, law, len(Xq))
    assert_no_law(ref)
    dist, idx = est.kneighbors(Xq)
    np.testing.assert_array_equal(est.predict(Xq), sklearn_predict(est.regressor_._y, dist, idx, weights=law))
    np.testing.assert_array_equal(est.summarize(Xq, table), ref.summarize(Xq, table))
    assert_law_ran(est, law, len(Xq))
    np.testing.assert_array_equal(est.summarize(None, table), ref.summarize(None, table))
    pieces = [Xq[:1], Xq[1:30], Xq[30:]]
    np.testing.assert_array_equal(est.predict_chunks(iter(pieces)), ref.predict(Xq))
    assert_law_ran(est, law, len(Xq) - 30)
    got = est.predict_chunks(iter(pieces), out_dtype=np.float32, statistic=table)
    np.testing.assert_array_equal(got, NR.narrow_values(ref.summarize(Xq, table), np.float32))


# ---- 3. streamed calls -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    """The streamed cases' estimators (fitted with a dataframe: ids for ``return_dataframe_index``), tiles and yardsticks."""
    law = W().InverseDistance(1.0)
    est, ref = fit(law, "inv1", frame=True), fit(plain(law), "inv1-plain", frame=True)
    tiles, mtiles = make_tiles(), make_tiles(masked=True)
    X, MX = np.concatenate(tiles), np.concatenate(mtiles)
    valid = ~(MX == NODATA).any(axis=1)
    assert 0 < valid.sum() < len(MX) and not valid[0] and 0.15 < 1 - valid.mean() < 0.35

    def masked(fn):
        out = np.full((len(MX), 3), np.nan)
        out[valid] = fn(MX[valid])
        return out

    return dict(law=law, est=est, ref=ref, tiles=tiles, mtiles=mtiles, X=X, MX=MX, valid=valid,
                pred=ref.predict(X), stat=ref.summarize(X, STAT), mpred=masked(ref.predict),
                mstat=masked(lambda x: ref.summarize(x, STAT)), last_valid=int(valid[-SIZES[-1]:].sum()))


def test_stream_is_the_one_shot_call(S):
    """The reorder key counts rows over the whole call: a law-weighted stream over tiles equals the one-shot call on the
    concatenation, so a tile boundary cannot change an answer."""
    est, law = S["est"], S["law"]
    got = est.predict_chunks(iter(S["tiles"]))
    assert_law_ran(est, law, SIZES[-1], K)
    assert got.dtype == np.float64 and got.shape == (TOTAL, 3)
    np.testing.assert_array_equal(got, est.predict(S["X"]))
    np.testing.assert_array_equal(got, S["pred"])
    again = est.predict_chunks(iter([S["X"][:700], S["X"][700:701], S["X"][701:]]))
    np.testing.assert_array_equal(again, got)
    S["ref"].predict_chunks(iter(S["tiles"][:2]))
    assert_no_law(S["ref"])


def test_stream_nodata(S):
    est = S["est"]
    got = est.predict_chunks(iter(S["mtiles"]), nodata=NODATA)
    assert_law_ran(est, S["law"], S["last_valid"], K)  # (the law sees the compacted distances: valid rows only)
    np.testing.assert_array_equal(got, S["mpred"])
    assert np.isnan(got[~S["valid"]]).all() and not np.isnan(got[S["valid"]]).any()


def test_stream_bands(S):
    got = S["est"].predict_chunks(iter(as_bands(S["tiles"])), layout="bands")
    assert_law_ran(S["est"], S["law"], SIZES[-1], K)
    np.testing.assert_array_equal(got, S["pred"].T)


def test_stream_typed(S):
    got = S["est"].predict_chunks(iter(S["tiles"]), out_dtype=np.int16, scale=100, out_nodata=-32768)
    assert_law_ran(S["est"], S["law"], SIZES[-1], K)
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, NR.narrow_values(S["pred"], np.int16, np.full(3, 100.0), np.zeros(3), -32768))


def test_stream_statistic(S):
    got = S["est"].predict_chunks(iter(S["tiles"]), statistic=STAT)
    assert_law_ran(S["est"], S["law"], SIZES[-1], K)
    np.testing.assert_array_equal(got, S["stat"])
    np.testing.assert_array_equal(got[:, 0], S["pred"][:, 0])


def test_stream_neighbors(S):
    est = S["est"]
    want_d, want_i = est.kneighbors_chunks(iter(S["tiles"]), return_dataframe_index=True, index_dtype=np.int32)
    pred, dist, idx = est.predict_chunks(iter(S["tiles"]), return_neighbors=True, return_dataframe_index=True,
                                         index_dtype=np.int32)
    assert_law_ran(est, S["law"], SIZES[-1], K)
    assert idx.dtype == np.int32 and dist.dtype == np.float64
    np.testing.assert_array_equal(pred, S["pred"])
    np.testing.assert_array_equal(dist, want_d)
    np.testing.assert_array_equal(idx, want_i)
    assert set(np.unique(idx)) <= set(est.dataframe_index_in_.tolist())


def test_stream_out_arrays(S):
    est = S["est"]
    out = np.full((TOTAL + 5, 3), 77.0)
    ret = est.predict_chunks(iter(S["tiles"]), out=out)
    np.testing.assert_array_equal(out[:TOTAL], S["pred"])
    np.testing.assert_array_equal(ret, S["pred"])
    assert np.shares_memory(ret, out) and (out[TOTAL:] == 77.0).all()
    want_d, want_i = est.kneighbors_chunks(iter(S["tiles"]))
    out = np.full((TOTAL, 3), 77.0)
    o_d, o_i = np.full((TOTAL, K), 7.5), np.full((TOTAL, K), 77, dtype=np.int64)
    pred, dist, idx = est.predict_chunks(iter(S["tiles"]), out=out, return_neighbors=True, neighbors_out=(o_d, o_i))
    assert_law_ran(est, S["law"], SIZES[-1], K)
    for got, arr, want in ((pred, out, S["pred"]), (dist, o_d, want_d), (idx, o_i, want_i)):
        np.testing.assert_array_equal(arr, want)
        np.testing.assert_array_equal(got, want)
        assert np.shares_memory(got, arr)


def test_stream_everything_together(S):
    """As the stored rasters: band-first, masked, per-target statistics, int16 with a scale and an offset, the plot ids
    (int32) and the distances from the same search, all into the caller's arrays."""
    est = S["est"]
    feed = as_bands(S["mtiles"])
    scale, offset = np.array([10.0, 1.0, 5.0]), np.array([0.5, 0.0, -3.0])
    want = NR.narrow_values(S["mstat"], np.int16, scale, offset, -32768).T
    want_d, want_i = est.kneighbors_chunks(iter(feed), nodata=NODATA, layout="bands", return_dataframe_index=True,
                                           index_dtype=np.int32)
    out = np.zeros((3, TOTAL), dtype=np.int16)
    o_d, o_i = np.zeros((K, TOTAL)), np.zeros((K, TOTAL), dtype=np.int32)
    pred, dist, idx = est.predict_chunks(iter(feed), out=out, nodata=NODATA, layout="bands", out_dtype=np.int16,
                                         scale=scale, offset=offset, out_nodata=-32768, statistic=STAT,
                                         return_neighbors=True, return_dataframe_index=True, index_dtype=np.int32,
                                         neighbors_out=(o_d, o_i))
    assert_law_ran(est, S["law"], S["last_valid"], K)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(pred, want)
    np.testing.assert_array_equal(o_d, want_d)
    np.testing.assert_array_equal(o_i, want_i)
    np.testing.assert_array_equal(dist, want_d)
    np.testing.assert_array_equal(idx, want_i)
    assert (out[:, ~S["valid"]] == -32768).all() and (o_i[:, ~S["valid"]] == -1).all() and np.isnan(o_d[:, ~S["valid"]]).all()


def test_stream_compact_law_fills_without_a_mask():
    """A law that can vanish: the NaN predictions of all-zero rows become ``out_nodata`` through the narrow kernel, with
    no nodata mask in the call."""
    law = W().Triangular(1.5)
    est, ref = fit(law, "tri1.5"), fit(plain(law), "tri1.5-plain")
    tiles = make_tiles(far=0.2)
    X = np.concatenate(tiles)
    with np.errstate(all="ignore"):
        want = ref.predict(X)
    gone = np.isnan(want).all(axis=1)
    assert gone.any() and gone.sum() < len(X) / 2 and not np.isnan(want[~gone]).any()
    with pytest.raises(ValueError, match="out_nodata is required"):
        est.predict_chunks(iter(tiles), out_dtype=np.int16, scale=100)
    got = est.predict_chunks(iter(tiles), out_dtype=np.int16, scale=100, out_nodata=-32768)
    assert_law_ran(est, law, SIZES[-1], K)
    np.testing.assert_array_equal(got, NR.narrow_values(want, np.int16, np.full(3, 100.0), np.zeros(3), -32768))
    assert (got[gone] == -32768).all() and (got[~gone] != -32768).all()
    np.testing.assert_array_equal(est.predict_chunks(iter(tiles)), want)  # (untyped: NaN stays NaN)


# ---- 4. refusals that remain -------------------------------------------------------------------------------------------------
def test_plain_callables_stay_refused(S):
    ref = S["ref"]
    tiles = S["tiles"]
    for kwargs, feed, msg in ((dict(nodata=NODATA), tiles, "nodata is not supported with callable weights"),
                              (dict(layout="bands"), as_bands(tiles), "layout='bands' is not supported with callable weights"),
                              (dict(out_dtype=np.int16, scale=100, out_nodata=-32768), tiles,
                               "typed outputs are not supported with callable weights"),
                              (dict(return_neighbors=True), tiles, "return_neighbors is not supported with callable weights")):
        with pytest.raises(NotImplementedError, match=msg):
            ref.predict_chunks(iter(feed), **kwargs)
    with pytest.raises(NotImplementedError, match="nodata is not supported with callable weights"):
        ref.engine_.predict(S["X"][:10], K, ref.weights, nodata=np.full(D, NODATA))
    with pytest.raises(ValueError, match="a stream predicts with"):
        ref.engine_.open_stream(K, weights=ref.weights)
    # ... and still answers tile by tile, on the host
    np.testing.assert_array_equal(ref.predict_chunks(iter(tiles)), S["pred"])
    assert_no_law(ref)


def test_the_call_must_name_the_handle_s_law(S):
    from sknnr_amd import _native

    est, law = S["est"], S["law"]
    X = S["X"][:20]
    est.predict(X)  # (the handle holds law 1 and its parameter)
    ix = est.engine_._index
    EXP = _native.WEIGHTS_EXPLICIT

    def refused(call, match):
        with pytest.raises(_native.HipBackendError, match=match) as err:
            call()
        assert err.value.code == _native.ERR_INVALID

    other = ix.make_opts(K, weight_mode=EXP, weight_law=_native.WEIGHT_LAWS["inverse_squared"])
    refused(lambda: ix.predict_host(X, other), "the handle holds the parameters of law 1")
    refused(lambda: ix.summarize_host(X, other, [0, 1, 5]), "the handle holds the parameters of law 1")
    refused(lambda: ix.predict_masked_host(X, other, np.full(D, NODATA)), "the handle holds the parameters of law 1")
    refused(lambda: ix.open_stream(other, want_dist=False, want_pred=True), "the handle holds the parameters of law 1")
    refused(lambda: ix.predict_host(X, ix.make_opts(K, weight_mode=EXP, weight_law=9)), "unknown weight law 9")
    # a law goes with the explicit base mode, and float32 weights do not exist for it
    for mode in (_native.WEIGHTS_UNIFORM, _native.WEIGHTS_DISTANCE, EXP | _native.WEIGHTS_F32_WEIGHTS):
        refused(lambda: ix.predict_host(X, ix.make_opts(K, weight_mode=mode, weight_law=law.code)), "a weight law takes weight mode")
    # without a law, explicit weights stay with the from-neighbours entry points, exactly as before
    refused(lambda: ix.predict_host(X, ix.make_opts(K, weight_mode=EXP)), "explicit weights go through sknnr_predict_from_neighbors")
    refused(lambda: ix.set_weight_law_params(law.code, 0.0, 0.0), "p0 must be finite and > 0")
    refused(lambda: ix.set_weight_law_params(7, 1.0, 0.0), "unknown weight law 7")
    # the parameters cannot change under an open stream (the same ones may be set again)
    stream = ix.open_stream(ix.make_opts(K, weight_mode=EXP, weight_law=law.code), want_dist=False, want_pred=True)
    try:
        ix.set_weight_law_params(law.code, *law.params)
        refused(lambda: ix.set_weight_law_params(law.code, 2.0, 0.0), "a query stream is open")
    finally:
        stream.close()
    # nothing above moved the handle's law: the estimator answers as before
    np.testing.assert_array_equal(est.predict(X), S["pred"][:20])
    assert_law_ran(est, law, 20, K)
