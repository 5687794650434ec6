"""Neighbour usage at estimator level: ``usage=`` on ``kneighbors_chunks`` / ``predict_chunks`` and the one-shot
``neighbor_usage`` / ``independent_neighbor_usage``, on the Moscow fixture with ``n_neighbors = 5``.

Tiles are the 33 test rows repeated 100 times and jittered (3,300 pixels) in four pushes of 1, 1,500, 700 and 1,099.  The
expectation is always the numpy model (tests/_usage.py) applied to what ``kneighbors_chunks`` returns for the same tiles
WITHOUT ``usage``; everything a call with ``usage`` returns or writes must be bit-equal to the call without it.

Without the feature every test here fails: the keyword, the class and the methods do not exist.

Measured on an MI355X: the 7 cases take under a second together (0.45 s of it the RFNN fit).
"""

from __future__ import annotations

import numpy as np
import pytest

import _usage as U

pytestmark = pytest.mark.gpu

K = 5
SIZES = (1, 1_500, 700, 1_099)
NODATA = -32768
INT_COLS = slice(5, 20)  # Moscow columns whose rounded values fit int16 (the first two are UTM coordinates)


def cut(x):
    edges = np.cumsum((0,) + SIZES)
    assert edges[-1] == len(x)
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


def float_tiles(moscow):
    rng = np.random.default_rng(7)
    x = np.tile(moscow["X_test"], (100, 1))
    return cut(x * (1.0 + 0.01 * rng.standard_normal(x.shape)))


def int_tiles(moscow):
    """int16 tiles: some pixels hold nodata in one band, the 700-pixel tile in all of its pixels."""
    rng = np.random.default_rng(8)
    x = np.tile(np.rint(moscow["X_test"][:, INT_COLS]), (100, 1)) + rng.integers(-20, 21, size=(3_300, 15))
    tiles = cut(x.astype(np.int16))
    for t in tiles:
        rows = np.flatnonzero(rng.random(len(t)) < 0.2)
        t[rows, rng.integers(0, 15, size=rows.size)] = NODATA
    tiles[2][:, 3] = NODATA
    return tiles


def as_bands(tiles):
    return [np.ascontiguousarray(t.T) for t in tiles]


def expect(u, idx, dist, n_ref, times=1):
    """``u`` against the model on the neighbours a call without ``usage`` returned."""
    counts, mx, _ = U.tally(idx, dist, n_ref)
    assert u.shape == (n_ref, idx.shape[1])
    np.testing.assert_array_equal(u.counts, times * counts)
    np.testing.assert_array_equal(u.total, times * counts.sum(1))
    np.testing.assert_array_equal(u.max_distance, np.where(counts.sum(1) == 0, np.nan, mx))
    np.testing.assert_array_equal(u.unused, counts.sum(1) == 0)


@pytest.fixture(scope="module")
def raw(moscow):
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(moscow["X_train"], moscow["y_train"])
    tiles = float_tiles(moscow)
    dist, idx = est.kneighbors_chunks(iter(tiles))  # the reference of every row-layout test: computed once, never changed
    dist.setflags(write=False)
    idx.setflags(write=False)
    return est, tiles, dist, idx


def test_row_layout_float64(raw):
    import sknnr_amd

    est, tiles, dist, idx = raw
    n_ref = est.n_samples_fit_
    u = sknnr_amd.NeighborUsage()
    got_d, got_i = est.kneighbors_chunks(iter(tiles), usage=u)
    np.testing.assert_array_equal(got_i, idx)
    np.testing.assert_array_equal(got_d, dist)
    expect(u, idx, dist, n_ref)
    assert u.n_rows == sum(SIZES) and u.ids is None
    rec = est.engine_._index.debug_last_tally()
    assert rec["ran"] == 1 and rec["rows"] == sum(SIZES) and rec["k"] == K and rec["skipped"] == 0, rec
    assert rec["tallied"] == sum(SIZES) * K
    # predictions only: no neighbour leaves the device, the tally is the same
    want = est.predict_chunks(iter(tiles))
    p = sknnr_amd.NeighborUsage()
    np.testing.assert_array_equal(est.predict_chunks(iter(tiles), usage=p), want)
    assert p == u
    # ... and beside the neighbours
    q = sknnr_amd.NeighborUsage()
    pred, nd, ni = est.predict_chunks(iter(tiles), return_neighbors=True, usage=q)
    np.testing.assert_array_equal(pred, want)
    np.testing.assert_array_equal(ni, idx)
    np.testing.assert_array_equal(nd, dist)
    assert q == u


def test_two_calls_accumulate_and_another_k_is_refused(raw):
    import sknnr_amd

    est, tiles, dist, idx = raw
    u = sknnr_amd.NeighborUsage()
    est.kneighbors_chunks(iter(tiles[:2]), usage=u)
    est.predict_chunks(iter(tiles[2:]), usage=u)
    d1, i1 = est.kneighbors_chunks(iter(tiles[:2]))
    d2, i2 = est.kneighbors_chunks(iter(tiles[2:]))
    both_i, both_d = np.concatenate([i1, i2]), np.concatenate([d1, d2])
    expect(u, both_i, both_d, est.n_samples_fit_)
    est.kneighbors_chunks(iter(tiles[:2]), usage=u)
    est.kneighbors_chunks(iter(tiles[2:]), usage=u)
    expect(u, both_i, both_d, est.n_samples_fit_, times=2)
    before = u.counts.copy()
    with pytest.raises(ValueError, match=r"bound to \(n_ref, k\) = \(132, 5\)"):
        est.kneighbors_chunks(iter(tiles), n_neighbors=3, usage=u)
    np.testing.assert_array_equal(u.counts, before)
    other = sknnr_amd.NeighborUsage()
    est.kneighbors_chunks(iter(tiles[:1]), n_neighbors=3, usage=other)
    assert other.shape == (132, 3) and other.n_rows == 1
    empty = sknnr_amd.NeighborUsage()
    est.kneighbors_chunks(iter([]), usage=empty)  # nothing pushed: bound, all zero
    assert empty.shape == (132, 5) and empty.n_rows == 0 and empty.unused.all() and np.isnan(empty.max_distance).all()


def test_band_layout_masked_typed_plan_and_ids(moscow):
    """int16 band tiles with nodata, one tile fully masked; int16 predictions from an output plan; dataframe ids looked up
    on the device with fill_index = 0: none of it reaches the tally, which keys on row positions of valid pixels."""
    import pandas as pd
    import sknnr_amd

    x = np.rint(moscow["X_train"][:, INT_COLS])
    ids = np.arange(len(x), dtype=np.int64) * 3 + 1_000
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K).fit(pd.DataFrame(x, index=ids), moscow["y_train"][:, :3])
    tiles = int_tiles(moscow)
    feed = as_bands(tiles)
    valid = ~(np.concatenate(tiles) == NODATA).any(axis=1)
    assert 0 < valid.sum() < len(valid) and not valid[1_501:2_201].any()
    # the reference: row indices of the same tiles without usage (masked pixels: -1, which the model skips)
    ref_d, ref_i = est.kneighbors_chunks(iter(feed), layout="bands", nodata=NODATA)
    ref_d, ref_i = U.rows_form(ref_d, True), U.rows_form(ref_i, True)
    assert (ref_i[~valid] == -1).all() and (ref_i[valid] >= 0).all()
    plan = [(0, "mean"), (1, ("quantile", 0.9)), (2, "mode"), (0, "std")]
    kw = dict(layout="bands", nodata=NODATA, out_dtype=np.int16, scale=0.5, out_nodata=NODATA, outputs=plan)
    nb = dict(return_neighbors=True, return_dataframe_index=True, fill_index=0)

    base = est.predict_chunks(iter(feed), **kw, **nb)
    u = sknnr_amd.NeighborUsage()
    got = est.predict_chunks(iter(feed), **kw, **nb, usage=u)
    for a, b in zip(got, base):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
    assert got[0].dtype == np.int16 and (got[2][:, ~valid] == 0).all() and np.isin(got[2][:, valid], ids).all()
    expect(u, ref_i, ref_d, len(x))
    assert u.n_rows == valid.sum()
    np.testing.assert_array_equal(u.ids, ids)
    # predictions alone into a caller's raster
    out0 = np.zeros((len(plan), len(valid)), dtype=np.int16)
    out1 = np.zeros_like(out0)
    est.predict_chunks(iter(feed), out=out0, **kw)
    v = sknnr_amd.NeighborUsage()
    est.predict_chunks(iter(feed), out=out1, **kw, usage=v)
    np.testing.assert_array_equal(out1, out0)
    assert v == u
    # row indices with fill_index = 0: the expanded tile holds 0 for masked pixels, the tally must not see them
    w = sknnr_amd.NeighborUsage()
    d0, i0 = est.kneighbors_chunks(iter(feed), layout="bands", nodata=NODATA, fill_index=0, usage=w)
    assert (i0[:, ~valid] == 0).all()
    expect(w, ref_i, ref_d, len(x))
    # the row layout of the same pixels gives the same tally
    r = sknnr_amd.NeighborUsage()
    est.kneighbors_chunks(iter(tiles), nodata=NODATA, index_dtype=np.int32, distance_dtype=np.float32, usage=r)
    expect(r, ref_i, ref_d, len(x))


@pytest.mark.parametrize("kind", ["gnn", "rfnn"])
def test_transformed_estimators(moscow, kind):
    """The affine map (GNN) and the forest map (RFNN) on the device, through ``predict_chunks(usage=u)``."""
    import sknnr_amd

    X, y = moscow["X_train"], moscow["y_train"]
    if kind == "gnn":
        est = sknnr_amd.GNNRegressor(n_neighbors=K, weights="distance").fit(X, y)
    else:
        est = sknnr_amd.RFNNRegressor(n_neighbors=K, n_estimators=20, random_state=0).fit(X, y)
    assert est._map_on_device()
    tiles = float_tiles(moscow)
    dist, idx = est.kneighbors_chunks(iter(tiles))
    want = est.predict_chunks(iter(tiles))
    u = sknnr_amd.NeighborUsage()
    np.testing.assert_array_equal(est.predict_chunks(iter(tiles), usage=u), want)
    expect(u, idx, dist, len(X))
    assert u.n_rows == sum(SIZES)
    k3 = sknnr_amd.NeighborUsage()
    d3, i3 = est.kneighbors_chunks(iter(tiles), n_neighbors=3, usage=k3)
    expect(k3, i3, d3, len(X))
    # one-shot forms go through the same search as kneighbors
    Xq = moscow["X_test"]
    expect(est.neighbor_usage(Xq), *est.kneighbors(Xq)[::-1], len(X))
    expect(est.neighbor_usage(), *est.kneighbors()[::-1], len(X))
    groups = np.arange(len(X)) // 4
    expect(est.independent_neighbor_usage(groups), *est.independent_kneighbors(groups)[::-1], len(X))


def test_one_shot_forms(raw, moscow):
    est, _, _, _ = raw
    n_ref = est.n_samples_fit_
    Xq = moscow["X_test"]
    d, i = est.kneighbors(Xq)
    u = est.neighbor_usage(Xq)
    expect(u, i, d, n_ref)
    assert u.n_rows == len(Xq)
    d, i = est.kneighbors()
    u = est.neighbor_usage()
    expect(u, i, d, n_ref)
    assert u.n_rows == n_ref and u.counts.sum() == n_ref * K
    d, i = est.kneighbors(Xq, n_neighbors=2)
    expect(est.neighbor_usage(Xq, n_neighbors=2), i, d, n_ref)
    groups = np.arange(n_ref) % 11
    d, i = est.independent_kneighbors(groups)
    g = est.independent_neighbor_usage(groups)
    expect(g, i, d, n_ref)
    d, i = est.independent_kneighbors(groups, n_neighbors=3)
    expect(est.independent_neighbor_usage(groups, n_neighbors=3), i, d, n_ref)
    g += u  # two one-shot tallies of one shape merge
    assert g.n_rows == 2 * n_ref


def test_refusals_under_the_host_side_tie_policies(moscow):
    import sknnr_amd

    X, y = moscow["X_train"], moscow["y_train"]
    tiles = float_tiles(moscow)[:2]
    with sknnr_amd.hamming_tie_policy("numpy"):
        est = sknnr_amd.RFNNRegressor(n_neighbors=K, n_estimators=5, random_state=0).fit(X, y)
        for call in (est.kneighbors_chunks, est.predict_chunks):
            u = sknnr_amd.NeighborUsage()
            with pytest.raises(NotImplementedError, match=r"usage is not supported under hamming_tie_policy\('numpy'\)"):
                call(iter(tiles), usage=u)
            assert u.shape is None
    with sknnr_amd.tree_tie_policy("tree"):
        est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="kd_tree").fit(X, y)
        for call in (est.kneighbors_chunks, est.predict_chunks):
            with pytest.raises(NotImplementedError, match=r"usage is not supported under tree_tie_policy\('tree'\)"):
                call(iter(tiles), usage=sknnr_amd.NeighborUsage())
    callable_est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=lambda d: 1.0 / (1.0 + d)).fit(X, y)
    with pytest.raises(NotImplementedError, match="usage is not supported with callable weights"):
        callable_est.predict_chunks(iter(tiles), usage=sknnr_amd.NeighborUsage())
