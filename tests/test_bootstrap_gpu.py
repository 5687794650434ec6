"""``bootstrap=`` end to end on the device: ``summarize`` against the numpy restatement (tests/_bootstrap.py) applied to
what ``kneighbors(X, n_neighbors=kw)`` returns, bit for bit; the streamed call against the one-shot call over tile cuts
{1, 63, 64, 65, rest}, with ``nodata``, ``layout="bands"`` and int16 + ``scale`` + ``out_nodata``; the replay of the
``(dist, idx)`` raster of ``kw`` columns a search stream stored against the search-side bootstrap, in float64 / int64, in
float32 / int32 storage and with dataframe ids (``bootstrap_neighbors_chunks``); an all-ones table; the tallies; the refusals the native layer makes; and that
calls without the keyword return what they returned before it existed.

Data: ``load_moscow_stjoes`` (165 rows, a transformed estimator) and a 300-row synthetic set with two co-located plots (exact
zero distances) under an int16 raster that repeats fitted rows exactly.

Without the feature every test here fails (``sknnr_amd`` has no ``Bootstrap``)."""

from __future__ import annotations

import numpy as np
import pytest

import _bootstrap as BS

pytestmark = pytest.mark.gpu

K, KW, B = 5, 20, 37
SIZES = (1, 63, 64, 65, 1807)
N = sum(SIZES)
NODATA = -32768
WEIGHTS = ("uniform", "distance", "law")
PLAN = [(1, "boot_se"), (0, "boot_mean"), "boot_count", (2, "boot_bias"), (1, "boot_mean"), (0, "boot_se")]


def cut(x, axis=0):
    edges = np.cumsum((0,) + SIZES)
    return [np.take(x, np.arange(a, b), axis=axis) for a, b in zip(edges[:-1], edges[1:])]


def reference_rows():
    rng = np.random.default_rng(31)
    X = rng.integers(100, 900, size=(300, 6)).astype(np.float64)
    X[10] = X[11]  # (two co-located plots: exact zero distances and ties)
    y = np.column_stack([X[:, 0] * 0.5 + X[:, 1], np.sqrt(X[:, 2]) * 10.0, (X[:, 3] - X[:, 4]) // 100])
    return X, y


def raster():
    rng = np.random.default_rng(32)
    X, _ = reference_rows()
    px = X[rng.integers(0, len(X), size=N)] + rng.integers(-40, 41, size=(N, 6))
    px[::9] += rng.integers(300, 3000, size=(len(px[::9]), 6))
    px[5::17] = X[rng.integers(0, len(X), size=len(px[5::17]))]
    px = px.astype(np.int16)
    px[3::13, 2] = NODATA
    return px


def weights_of(name):
    from sknnr_amd import weights as W

    return W.Triangular(1500.0) if name == "law" else name


def new_bootstrap(**kw):
    import sknnr_amd

    return sknnr_amd.Bootstrap(B, seed=11, n_candidates=KW, **kw)


def same(a, b):
    """Bit for bit, NaN payloads included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert a.tobytes() == b.tobytes()


@pytest.fixture(scope="module", params=WEIGHTS)
def setup(request):
    """An estimator per weight kind, the raster, its valid rows, what the calls without ``bootstrap=`` return before any
    bootstrap ran, and the search-side bootstrap of the whole raster in one tile.  Computed once, never changed."""
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    X, y = reference_rows()
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights_of(request.param)).fit(X, y)
    px = raster()
    valid = px[:, 2] != NODATA
    before = (est.summarize(px[valid].astype(np.float64)), est.predict_chunks(iter(cut(px)), nodata=NODATA),
              est.summarize(px[valid].astype(np.float64), outputs=[(0, "std"), (2, "max")]))
    bs = new_bootstrap()
    whole = est.predict_chunks([px], nodata=NODATA, outputs=PLAN, bootstrap=bs)
    whole.setflags(write=False)
    assert bs.pixels == valid.sum()
    return request.param, est, px, valid, y, before, whole


def test_summarize_equals_the_restatement(setup):
    name, est, px, valid, y, _, whole = setup
    Xv = px[valid].astype(np.float64)
    bs = new_bootstrap()
    got = est.summarize(Xv, outputs=PLAN, bootstrap=bs)
    dist, idx = est.kneighbors(Xv, n_neighbors=KW)
    want, tally = BS.bootstrap_of(y, dist, idx, bs.multiplicity, K, weights_of(name), PLAN)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.float64 and got.shape == (valid.sum(), len(PLAN))
    assert (bs.pixels, bs.replicates_used) == tuple(tally) and 0 < bs.share_short < 1
    np.testing.assert_array_equal(bs.multiplicity, BS.draw_table(B, 300, seed=11))
    same(got, whole[valid])  # (the streamed call's valid pixels)
    assert np.isnan(whole[~valid]).all()
    # the default: boot_se of every target
    default = est.summarize(Xv, bootstrap=new_bootstrap())
    np.testing.assert_array_equal(default, BS.bootstrap_of(y, dist, idx, bs.multiplicity, K, weights_of(name),
                                                           [(j, "boot_se") for j in range(3)])[0])
    same(default[:, [1, 0]], got[:, [0, 5]])
    # the fitted rows themselves, each left out of its own list
    bs0 = new_bootstrap()
    got0 = est.summarize(None, outputs=PLAN, bootstrap=bs0)
    d0, i0 = est.kneighbors(None, n_neighbors=KW)
    np.testing.assert_array_equal(got0, BS.bootstrap_of(y, d0, i0, bs0.multiplicity, K, weights_of(name), PLAN)[0])
    # CUDA tensors in, CUDA tensors out
    import torch

    on_device = est.summarize(torch.from_numpy(Xv).cuda(), outputs=PLAN, bootstrap=new_bootstrap())
    same(on_device.cpu().numpy(), got)


def test_tiles_equal_the_one_shot_call(setup):
    name, est, px, valid, y, _, whole = setup
    bs = new_bootstrap()
    got = est.predict_chunks(iter(cut(px)), nodata=NODATA, outputs=PLAN, bootstrap=bs)
    same(got, whole)
    assert bs.pixels == valid.sum()
    out = np.full((N + 3, len(PLAN)), 7.0)
    back = est.predict_chunks(iter(cut(px)), nodata=NODATA, outputs=PLAN, bootstrap=new_bootstrap(), out=out)
    same(back, whole)
    assert np.shares_memory(back, out) and (out[N:] == 7.0).all()
    # without a mask the masked rows are ordinary pixels (the nodata value is a number like any other)
    plain = est.predict_chunks(iter(cut(px)), outputs=PLAN, bootstrap=new_bootstrap())
    same(plain, est.summarize(px.astype(np.float64), outputs=PLAN, bootstrap=new_bootstrap()))
    same(plain[valid], whole[valid])


def test_tiles_as_bands(setup):
    name, est, px, valid, y, _, whole = setup
    bands = np.ascontiguousarray(px.T)
    got = est.predict_chunks(iter(cut(bands, 1)), nodata=NODATA, layout="bands", outputs=PLAN, bootstrap=new_bootstrap())
    same(got, whole.T)
    out = np.zeros((len(PLAN), N))
    est.predict_chunks(iter(cut(bands, 1)), nodata=NODATA, layout="bands", outputs=PLAN, bootstrap=new_bootstrap(), out=out)
    same(out, whole.T)


def test_tiles_typed(setup):
    name, est, px, valid, y, _, whole = setup
    kw = dict(nodata=NODATA, outputs=PLAN, out_dtype=np.int16, scale=10.0, offset=0.0, out_nodata=-9999)
    one = est.predict_chunks([px], bootstrap=new_bootstrap(), **kw)
    got = est.predict_chunks(iter(cut(px)), bootstrap=new_bootstrap(), **kw)
    same(got, one)
    want = np.where(np.isnan(whole), -9999, np.clip(np.rint(whole * 10.0 + 0.0), -32768, 32767)).astype(np.int16)
    np.testing.assert_array_equal(got, want)
    assert (got == -9999).any() and got.dtype == np.int16
    with pytest.raises(ValueError, match="out_nodata"):
        est.predict_chunks([px], outputs=PLAN, out_dtype=np.int16, bootstrap=new_bootstrap())


def pairs(dist, idx, axis=0):
    return list(zip(cut(dist, axis), cut(idx, axis)))


def test_replay_of_a_stored_raster(setup):
    name, est, px, valid, y, _, whole = setup
    dist, idx = est.kneighbors_chunks(iter(cut(px)), n_neighbors=KW, nodata=NODATA)
    assert dist.shape == (N, KW) and (idx[~valid] == -1).all()
    searches = est.engine_._index.stats()["queries"]
    bs = new_bootstrap()
    got = est.bootstrap_neighbors_chunks(iter(pairs(dist, idx)), outputs=PLAN, bootstrap=bs)
    same(got, whole)
    assert bs.pixels == valid.sum() and est.engine_._index.stats()["queries"] == searches
    same(est.bootstrap_neighbors(idx, dist, outputs=PLAN, bootstrap=new_bootstrap()), whole)
    same(est.bootstrap_neighbors_chunks(iter(pairs(np.ascontiguousarray(dist.T), np.ascontiguousarray(idx.T), 1)), layout="bands",
                                      outputs=PLAN, bootstrap=new_bootstrap()), whole.T)
    # the leading columns of a wider store: kw = 12 of the 20 stored
    b12 = new_bootstrap()
    got12 = est.bootstrap_neighbors_chunks(iter(pairs(dist, idx)), outputs=PLAN, bootstrap=b12, n_neighbors=12)
    v = np.flatnonzero(valid)
    want12, tally12 = BS.bootstrap_of(y, dist[v, :12], idx[v, :12], b12.multiplicity, K, weights_of(name), PLAN)
    np.testing.assert_array_equal(got12[v], want12)
    assert (b12.pixels, b12.replicates_used) == tuple(tally12) and b12.share_short > bs.share_short
    # narrow storage: int32 positions and float32 distances
    d32, i32 = est.kneighbors_chunks(iter(cut(px)), n_neighbors=KW, nodata=NODATA, index_dtype=np.int32, distance_dtype=np.float32)
    assert d32.dtype == np.float32 and i32.dtype == np.int32
    got32 = est.bootstrap_neighbors_chunks(iter(pairs(d32, i32)), outputs=PLAN, bootstrap=new_bootstrap())
    if name == "uniform":
        same(got32, whole)
        same(est.bootstrap_neighbors_chunks(iter(cut(i32)), outputs=PLAN, bootstrap=new_bootstrap()), whole)
    else:  # (the weights come from the float32 distances as widened: the restatement on those, bit for bit)
        want32, _ = BS.bootstrap_of(y, d32[v].astype(np.float64), i32[v].astype(np.int64), bs.multiplicity, K, weights_of(name), PLAN)
        np.testing.assert_array_equal(got32[v], want32)
        assert np.isnan(got32[~valid]).all()


def test_replay_with_dataframe_ids(setup):
    import pandas as pd

    import sknnr_amd

    name, est, px, valid, y, _, whole = setup
    X, _ = reference_rows()
    ids = np.random.default_rng(5).permutation(np.concatenate([np.arange(250) * 7 + 1000, -5 - 3 * np.arange(50)]))
    frame = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights_of(name)).fit(pd.DataFrame(X, index=ids), y)
    dist, stored = frame.kneighbors_chunks(iter(cut(px)), n_neighbors=KW, nodata=NODATA, return_dataframe_index=True)
    assert set(np.unique(stored[stored != -1])) <= set(ids)
    got = frame.bootstrap_neighbors_chunks(iter(pairs(dist, stored)), ids=True, outputs=PLAN, bootstrap=new_bootstrap())
    same(got, whole)
    bad = stored.copy()
    bad[7, 3] = 123456789
    bs = new_bootstrap()
    blanked = frame.bootstrap_neighbors_chunks(iter(pairs(dist, bad)), ids=True, unknown="nodata", outputs=PLAN, bootstrap=bs)
    assert np.isnan(blanked[7]).all() and bs.pixels == valid.sum() - 1
    same(np.delete(blanked, 7, axis=0), np.delete(whole, 7, axis=0))


def test_an_all_ones_table_is_the_point_prediction(setup):
    import sknnr_amd

    name, est, px, valid, y, _, _ = setup
    Xv = px[valid].astype(np.float64)
    bs = sknnr_amd.Bootstrap(multiplicity=np.ones((B, 300), dtype=np.uint8), n_candidates=KW)
    plan = [(j, s) for j in range(3) for s in ("boot_se", "boot_bias", "boot_mean")] + ["boot_count"]
    got = est.summarize(Xv, outputs=plan, bootstrap=bs)
    pred = est.predict(Xv)
    fine = ~np.isnan(pred[:, 0])  # (a compact law predicts NaN where all k neighbours lie beyond its bandwidth)
    assert fine.sum() > 100 and (name == "law") == (not fine.all())
    for j in range(3):
        np.testing.assert_array_equal(got[fine, 3 * j], 0.0)
        np.testing.assert_array_equal(got[fine, 3 * j + 1], 0.0)
        np.testing.assert_allclose(got[fine, 3 * j + 2], pred[fine, j], rtol=1e-12)  # (sequential against numpy's pairwise sums)
    np.testing.assert_array_equal(got[fine, 9], B)
    assert np.isnan(got[~fine, :9]).all() and (got[~fine, 9] == 0).all()
    assert bs.pixels == len(Xv) and bs.replicates_used == B * fine.sum()


def test_tallies_add_up_over_calls(setup):
    name, est, px, valid, y, _, _ = setup
    Xv = px[valid].astype(np.float64)
    a, b, both = new_bootstrap(), new_bootstrap(), new_bootstrap()
    est.summarize(Xv[:500], bootstrap=a)
    est.predict_chunks([Xv[500:900], Xv[900:]], bootstrap=b)
    est.summarize(Xv[:500], bootstrap=both)
    est.summarize(Xv[500:], bootstrap=both)
    assert a.pixels == 500 and b.pixels == len(Xv) - 500
    a += b
    assert (a.pixels, a.replicates_used) == (both.pixels, both.replicates_used) and a == both
    assert both.share_short == pytest.approx(1 - both.replicates_used / (both.pixels * B))


def test_calls_without_the_keyword_are_unchanged(setup):
    name, est, px, valid, y, before, _ = setup
    Xv = px[valid].astype(np.float64)
    same(est.summarize(Xv), before[0])
    same(est.summarize(Xv, bootstrap=None), before[0])
    same(est.predict_chunks(iter(cut(px)), nodata=NODATA, bootstrap=None), before[1])
    same(est.summarize(Xv, outputs=[(0, "std"), (2, "max")], bootstrap=None), before[2])
    dist, idx = est.kneighbors_chunks(iter(cut(px)), nodata=NODATA)
    same(est.predict_neighbors_chunks(iter(pairs(dist, idx))), before[1])


def test_refusals_on_a_fitted_estimator(setup):
    import sknnr_amd

    name, est, px, valid, y, _, _ = setup
    Xv = px[valid][:10].astype(np.float64)
    with pytest.raises(ValueError, match="bound to n = 299"):
        est.summarize(Xv, bootstrap=sknnr_amd.Bootstrap(multiplicity=np.ones((3, 299), dtype=int)))
    with pytest.raises(ValueError, match="n_neighbors = 5 exceeds n_candidates = 4"):
        est.summarize(Xv, bootstrap=sknnr_amd.Bootstrap(3, n_candidates=4))
    with pytest.raises(ValueError, match="need bootstrap="):
        est.predict_chunks([Xv], outputs=[(0, "boot_se")])
    with pytest.raises(ValueError, match="a zonal sum of pixel standard errors"):
        est.predict_chunks([Xv], zones=[np.zeros(10, dtype=int)], zonal=sknnr_amd.ZonalStats(2), out_dtype=np.int16,
                           out_nodata=-1, bootstrap=new_bootstrap())
    if name != "uniform":
        with pytest.raises(ValueError, match="need.* the stored distances"):
            est.bootstrap_neighbors(np.zeros((4, KW), dtype=np.int64), bootstrap=new_bootstrap())


def test_refusals_of_the_stream_entries(setup):
    from sknnr_amd import _native

    name, est, px, valid, y, _, _ = setup
    ix = est.engine_._index
    est.engine_.set_bootstrap(new_bootstrap()._bind(300))
    plan = BS.arrays([(0, "boot_se"), "boot_count"])
    opts = _native.Index.make_opts(KW)
    with ix.open_stream(opts, want_dist=False, want_pred=False) as s:
        with pytest.raises(_native.HipBackendError, match="opened without predictions"):
            s.set_bootstrap(K, plan)
    with ix.open_stream(opts, want_dist=True, want_pred=True) as s:
        for k in (0, KW + 1):
            with pytest.raises(_native.HipBackendError, match="1 <= k <= kw"):
                s.set_bootstrap(k, plan)
        with pytest.raises(_native.HipBackendError, match="column 3 outside"):
            s.set_bootstrap(K, BS.arrays([(3, "boot_se")]))
        with pytest.raises(_native.HipBackendError, match="unknown statistic 4"):
            s.set_bootstrap(K, (np.zeros(1, dtype=np.int32), np.full(1, 4, dtype=np.int32)))
        with pytest.raises(_native.HipBackendError, match="no bootstrap stage"):
            s.bootstrap()
        s.set_bootstrap(K, plan)
        assert s.pred_cols == 2
        with pytest.raises(_native.HipBackendError, match="it takes no per-target statistics"):
            s.set_statistics(np.zeros(3, dtype=np.int32))
        with pytest.raises(_native.HipBackendError, match="it takes no output plan"):
            s.set_plan((np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1)))
        with pytest.raises(_native.HipBackendError, match="it takes no usage tally"):
            s.set_tally()
        with pytest.raises(_native.HipBackendError, match="it takes no distance domain"):
            s.set_domain(np.arange(1.0, 9.0))
        with pytest.raises(_native.HipBackendError, match="it takes no zonal statistics"):
            s.set_zonal(4)
        _, _, pred = s.push(px[valid][:9].astype(np.float64), need_idx=False)
        assert pred.shape == (9, 2)
        np.testing.assert_array_equal(s.bootstrap()[0], 9)
        with pytest.raises(_native.HipBackendError, match="only before the first push"):
            s.set_bootstrap(K, plan)
    with ix.open_stream(opts, want_dist=True, want_pred=True) as s:
        s.set_output(pred_dtype=np.int16, scale=np.ones(3), offset=np.zeros(3), fill=-1)
        with pytest.raises(_native.HipBackendError, match="comes before sknnr_stream_set_output"):
            s.set_bootstrap(K, plan)
    for first in ("set_statistics", "set_plan", "set_tally", "set_domain", "set_zonal"):
        with ix.open_stream(opts, want_dist=True, want_pred=True) as s:
            args = dict(set_statistics=(np.ones(3, dtype=np.int32),), set_tally=(), set_domain=(np.arange(1.0, 9.0),), set_zonal=(4,),
                        set_plan=((np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1)),))[first]
            getattr(s, first)(*args)
            with pytest.raises(_native.HipBackendError, match="it takes no bootstrap"):
                s.set_bootstrap(K, plan)
    est.engine_.set_bootstrap(None)
    with ix.open_stream(opts, want_dist=False, want_pred=True) as s:
        with pytest.raises(_native.HipBackendError, match="no bootstrap table"):
            s.set_bootstrap(K, plan)


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_a_transformed_estimator_on_moscow(weights):
    import sknnr_amd
    from sknnr_amd.datasets import load_moscow_stjoes

    ds = load_moscow_stjoes()
    X, y = np.asarray(ds.data, dtype=np.float64), np.asarray(ds.target, dtype=np.float64)
    assert X.shape[0] == 165
    est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=K, weights=weights).fit(X[:132], y[:132])
    t = y.shape[1]
    plan = [(t - 1, "boot_se"), (0, "boot_se"), (0, "boot_mean"), "boot_count", (1, "boot_bias")]
    bs = sknnr_amd.Bootstrap(200, seed=4, groups=np.arange(132) // 4)
    got = est.summarize(X[132:], outputs=plan, bootstrap=bs)
    kw = bs.candidates(K, 132)
    assert kw == 28
    dist, idx = est.kneighbors(X[132:], n_neighbors=kw)
    want, tally = BS.bootstrap_of(y[:132], dist, idx, bs.multiplicity, K, weights, plan)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(bs.multiplicity, BS.draw_table(200, 132, seed=4, groups=np.arange(132) // 4))
    assert (bs.pixels, bs.replicates_used) == tuple(tally)
    tiles = est.predict_chunks([X[132:133], X[133:150], X[150:]], outputs=plan, bootstrap=sknnr_amd.Bootstrap(
        200, seed=4, groups=np.arange(132) // 4))
    same(tiles, got)
    stored = est.kneighbors_chunks([X[132:]], n_neighbors=kw)
    same(est.bootstrap_neighbors(stored[1], stored[0], outputs=plan, bootstrap=sknnr_amd.Bootstrap(
        200, seed=4, groups=np.arange(132) // 4)), got)
    own = est.summarize(None, outputs=plan, bootstrap=sknnr_amd.Bootstrap(multiplicity=bs.multiplicity, n_candidates=kw))
    d0, i0 = est.kneighbors(None, n_neighbors=kw)
    np.testing.assert_array_equal(own, BS.bootstrap_of(y[:132], d0, i0, bs.multiplicity, K, weights, plan)[0])
