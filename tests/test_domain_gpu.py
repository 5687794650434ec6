"""Distance domain at estimator level: ``distance_domain``, ``domain_scores`` and ``domain=`` / ``domain_out=`` /
``beyond=`` on ``kneighbors_chunks`` / ``predict_chunks``.

The raw estimator has 300 reference rows of 6 integer-valued features, 3 targets and ``n_neighbors = 5``; its raster is
2,000 int16 pixels -- most of them near the reference rows, some far outside their range, some holding nodata --
pushed as tiles of 700, 1 and 1,299 pixels.  ``GNNRegressor`` runs on the Moscow fixture and a small ``RFNNRegressor``
on the same synthetic rows.  The expectation is always the numpy model (tests/_domain.py) applied to the distances
``kneighbors_chunks`` returns for the same tiles WITHOUT ``domain``; everything a call with ``domain`` returns or writes
must be bit-equal to the call without it unless ``beyond="nodata"`` blanks it.

Without the feature every test here fails: the keywords, the class and the methods do not exist.

The last case has an estimator of its own: 64 reference rows, two tiles of 8 pixels, every side product in one call.

Measured on an MI355X: the 14 cases take 3.8 s, of which 3.1 s are the first fixture's device set-up; no case takes more than
0.05 s.
"""

from __future__ import annotations

import numpy as np
import pytest

import _domain as D

pytestmark = pytest.mark.gpu

K = 5
SIZES = (700, 1, 1_299)
N = sum(SIZES)
NODATA = -32768
N_ZONES = 7


def cut(x, sizes=SIZES, axis=0):
    edges = np.cumsum((0,) + tuple(sizes))
    assert edges[-1] == x.shape[axis]
    return [np.take(x, np.arange(a, b), axis=axis) for a, b in zip(edges[:-1], edges[1:])]


def reference_rows():
    rng = np.random.default_rng(21)
    X = rng.integers(100, 900, size=(300, 6)).astype(np.float64)
    X[10] = X[11]  # (two co-located plots: a zero in the table of a leave-one-out domain is legitimate)
    y = np.column_stack([X[:, 0] * 0.5 + X[:, 1], np.sqrt(X[:, 2]) * 10.0, X[:, 3] - X[:, 4]])
    return X, y


def raster():
    """(2000, 6) int16: reference rows jittered, every ninth pixel far outside, some reference rows themselves (distance
    0), every 13th pixel nodata in one band."""
    rng = np.random.default_rng(22)
    X, _ = reference_rows()
    px = X[rng.integers(0, len(X), size=N)] + rng.integers(-40, 41, size=(N, 6))
    px[::9] += rng.integers(300, 3000, size=(len(px[::9]), 6))
    px[5::17] = X[rng.integers(0, len(X), size=len(px[5::17]))]
    px = px.astype(np.int16)
    px[3::13, 2] = NODATA
    return px


def zone_codes():
    return ((np.arange(N) // 61) % N_ZONES).astype(np.int32)


def expect(domain, codes, dist, times=1):
    """``domain`` and the code plane against the model on the distances a call without ``domain`` returned."""
    if codes is not None:
        np.testing.assert_array_equal(codes, D.codes(dist, domain.table, domain.rank))
        np.testing.assert_array_equal(codes, domain.percent(dist[:, domain.rank - 1]))
    acc = D.acc(dist, domain.table, domain.rank, domain.threshold)
    np.testing.assert_array_equal(domain.hist, times * acc[:101])
    assert domain.n_pixels == times * acc[:101].sum()
    assert domain.n_beyond == times * acc[D.BEYOND] and domain.n_nodata == times * acc[D.NODATA]
    return acc


@pytest.fixture(scope="module")
def raw():
    import sknnr_amd
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    X, y = reference_rows()
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights="distance").fit(X, y)
    px = raster()
    # the reference of every test: computed once, without the lane, never changed
    dist, idx = est.kneighbors_chunks(iter(cut(px)), nodata=NODATA)
    pred = est.predict_chunks(iter(cut(px)), nodata=NODATA)
    for a in (dist, idx, pred):
        a.setflags(write=False)
    assert np.isnan(dist[:, 0]).sum() == len(px[3::13])
    return est, px, dist, idx, pred


def test_distance_domain_is_the_sorted_independent_distances(raw):
    import sknnr_amd

    est = raw[0]
    groups = np.arange(300) // 3
    for kw, rank in ((dict(), 1), (dict(groups=groups), 1), (dict(rank=3), 3),
                     (dict(buffer=(reference_rows()[0][:, :2], 60.0), rank=2), 2)):
        d = est.distance_domain(**kw)
        own = None if "buffer" in kw else np.arange(300)  # (self left out: every row a group of its own)
        want = est.independent_kneighbors(kw.get("groups", own), n_neighbors=rank, buffer=kw.get("buffer"))[0][:, rank - 1]
        assert isinstance(d, sknnr_amd.DistanceDomain) and d.rank == rank and d.threshold is None
        np.testing.assert_array_equal(d.table, np.sort(want))
        assert d.n_pixels == 0
    assert est.distance_domain().table[0] == 0.0  # (the co-located pair)
    table = est.distance_domain(groups).table
    for p in (0.05, 0.5, 0.013):
        d = est.distance_domain(groups, p=p)
        assert d.threshold == float(np.quantile(table, 1 - p))
        np.testing.assert_array_equal(d.table, table)
    assert est.distance_domain(threshold=12.5).threshold == 12.5
    with pytest.raises(ValueError, match="mutually exclusive"):
        est.distance_domain(p=0.1, threshold=1.0)


@pytest.mark.parametrize("rank", [1, K])
def test_codes_and_tallies_of_kneighbors_chunks(raw, rank):
    est, px, dist, idx, _ = raw
    d = est.distance_domain(rank=rank, p=0.05)
    plane = np.full(N, 77, dtype=np.uint8)
    got_d, got_i = est.kneighbors_chunks(iter(cut(px)), nodata=NODATA, domain=d, domain_out=plane)
    assert got_d.tobytes() == dist.tobytes() and got_i.tobytes() == idx.tobytes()
    acc = expect(d, plane, dist)
    # the raster was made to have all three kinds of pixel
    assert acc[D.NODATA] == len(px[3::13]) and (plane[3::13] == 255).all() and (plane != 255).sum() == d.n_pixels
    assert 0 < d.n_beyond < d.n_pixels and (plane == 100).sum() > 0 and (plane == 0).sum() > 0
    assert d.share_beyond == d.n_beyond / d.n_pixels
    rec = est.engine_._index.debug_last_domain()
    assert rec["ran"] == 1 and rec["pixels"] == N and rec["k"] == K and rec["rank"] == rank, rec
    assert rec["m"] == 300 and rec["nodata"] == acc[D.NODATA] and rec["blanked"] == 0, rec
    # without a plane the call tallies only, and a second call adds to the same object
    est.kneighbors_chunks(iter(cut(px)), nodata=NODATA, return_distance=False, domain=d)
    expect(d, None, dist, times=2)


def test_tile_cuts_do_not_change_a_byte(raw):
    est, px, dist, _, pred = raw
    planes, domains = [], []
    for sizes in ((N,), SIZES, (1, 1_998, 1)):
        d = est.distance_domain(p=0.1)
        plane = np.zeros(N, dtype=np.uint8)
        got = est.predict_chunks(iter(cut(px, sizes)), nodata=NODATA, domain=d, domain_out=plane)
        assert got.tobytes() == pred.tobytes()
        planes.append(plane)
        domains.append(d)
    assert planes[0].tobytes() == planes[1].tobytes() == planes[2].tobytes()
    assert domains[0] == domains[1] == domains[2]
    expect(domains[0], planes[0], dist)


def test_predictions_neighbours_and_ids_are_bit_identical(raw):
    est, px, dist, idx, pred = raw
    d = est.distance_domain(p=0.05)
    plane = np.zeros(N, dtype=np.uint8)
    p2, d2, i2 = est.predict_chunks(iter(cut(px)), nodata=NODATA, return_neighbors=True, domain=d, domain_out=plane)
    assert p2.tobytes() == pred.tobytes() and d2.tobytes() == dist.tobytes() and i2.tobytes() == idx.tobytes()
    expect(d, plane, dist)
    # typed neighbours: the codes are those of the float64 distances, not of the float32 ones that leave
    e = est.distance_domain(p=0.05)
    plane32 = np.zeros(N, dtype=np.uint8)
    base = est.kneighbors_chunks(iter(cut(px)), nodata=NODATA, index_dtype=np.int32, distance_dtype=np.float32)
    got = est.kneighbors_chunks(iter(cut(px)), nodata=NODATA, index_dtype=np.int32, distance_dtype=np.float32,
                                domain=e, domain_out=plane32)
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    assert plane32.tobytes() == plane.tobytes() and e == d


def test_dataframe_ids_leave_unchanged(moscow_frames):
    import sknnr_amd

    est = sknnr_amd.RawKNNRegressor(n_neighbors=K).fit(moscow_frames["X_train"], moscow_frames["y_train"])
    tiles = [moscow_frames["X_test"].iloc[:20], moscow_frames["X_test"].iloc[20:]]
    base_d, base_i = est.kneighbors_chunks(iter(tiles), return_dataframe_index=True)
    d = est.distance_domain()
    plane = np.zeros(33, dtype=np.uint8)
    got_d, got_i = est.kneighbors_chunks(iter(tiles), return_dataframe_index=True, domain=d, domain_out=plane)
    np.testing.assert_array_equal(got_i, base_i)
    np.testing.assert_array_equal(got_d, base_d)
    expect(d, plane, base_d)


def test_band_layout_with_windows(raw):
    est, px, dist, _, pred = raw
    windows = [np.ascontiguousarray(t.T) for t in cut(px)]
    windows[0] = windows[0].reshape(6, 28, 25)  # an (h, w) window of 700 pixels
    windows[2] = windows[2].reshape(6, 1, 1_299)
    d = est.distance_domain(rank=2, threshold=35.0)
    plane = np.zeros(N, dtype=np.uint8)
    out = np.zeros((3, N))
    got = est.predict_chunks(iter(windows), nodata=NODATA, layout="bands", out=out, domain=d, domain_out=plane)
    np.testing.assert_array_equal(got, pred.T)
    expect(d, plane, dist)


def test_beyond_nodata_blanks_floats_and_typed_outputs(raw):
    est, px, dist, idx, pred = raw
    d = est.distance_domain(p=0.05)
    far = D.beyond(dist, 1, d.threshold)
    assert 0 < far.sum() < N - len(px[3::13])
    plane = np.zeros(N, dtype=np.uint8)
    got, gd, gi = est.predict_chunks(iter(cut(px)), nodata=NODATA, return_neighbors=True, domain=d, domain_out=plane,
                                     beyond="nodata")
    np.testing.assert_array_equal(got, D.masked_predictions(pred, dist, 1, d.threshold))
    np.testing.assert_array_equal(np.isnan(got).all(1), far | np.isnan(dist[:, 0]))
    assert gd.tobytes() == dist.tobytes() and gi.tobytes() == idx.tobytes()  # (the neighbours are untouched)
    expect(d, plane, dist)
    assert est.engine_._index.debug_last_domain()["blanked"] == far.sum()
    # int16: out_nodata exactly on the beyond and the nodata rows, everything else as the call without the lane stores it
    kw = dict(nodata=NODATA, out_dtype=np.int16, scale=0.1, out_nodata=-9999)
    base = est.predict_chunks(iter(cut(px)), **kw)
    typed = est.predict_chunks(iter(cut(px)), domain=est.distance_domain(p=0.05), beyond="nodata", **kw)
    assert typed.dtype == np.int16
    np.testing.assert_array_equal(typed[far], np.full((far.sum(), 3), -9999))
    np.testing.assert_array_equal(typed[~far], base[~far])
    assert (base[far] != -9999).all()
    # the same call with beyond="keep" stores what the call without the lane stores
    kept = est.predict_chunks(iter(cut(px)), domain=est.distance_domain(p=0.05), **kw)
    assert kept.tobytes() == base.tobytes()
    # an output plan: every plane of a beyond pixel is blanked
    outputs = [(0, "mean"), (0, ("quantile", 0.9)), (2, "max"), (1, "nearest")]
    base = est.predict_chunks(iter(cut(px)), nodata=NODATA, outputs=outputs)
    planned = est.predict_chunks(iter(cut(px)), nodata=NODATA, outputs=outputs, domain=est.distance_domain(p=0.05),
                                 beyond="nodata")
    np.testing.assert_array_equal(planned, D.masked_predictions(base, dist, 1, d.threshold))


def test_beyond_nodata_with_zonal_and_usage(raw):
    import sknnr_amd

    est, px, dist, _, _ = raw
    zones = zone_codes()
    kw = dict(nodata=NODATA, out_dtype=np.int16, scale=0.1, out_nodata=-9999)
    z0, u0 = sknnr_amd.ZonalStats(N_ZONES), sknnr_amd.NeighborUsage()
    est.predict_chunks(iter(cut(px)), zones=iter(cut(zones)), zonal=z0, usage=u0, **kw)
    d = est.distance_domain(p=0.05)
    z1, u1 = sknnr_amd.ZonalStats(N_ZONES), sknnr_amd.NeighborUsage()
    plane = np.zeros(N, dtype=np.uint8)
    est.predict_chunks(iter(cut(px)), zones=iter(cut(zones)), zonal=z1, usage=u1, domain=d, domain_out=plane,
                       beyond="nodata", **kw)
    far = D.beyond(dist, 1, d.threshold)
    lost = np.bincount(zones[far], minlength=N_ZONES)
    assert lost.sum() == far.sum() and (lost > 0).any()
    np.testing.assert_array_equal(z1.count, z0.count - lost[:, None])
    assert u1 == u0  # (the usage tally is untouched)
    expect(d, plane, dist)
    # with beyond="keep" the zonal tables are those of the call without the lane
    z2 = sknnr_amd.ZonalStats(N_ZONES)
    est.predict_chunks(iter(cut(px)), zones=iter(cut(zones)), zonal=z2, domain=est.distance_domain(p=0.05), **kw)
    assert z2 == z0


def test_domain_scores_equals_the_streamed_plane(raw):
    est, px, dist, _, _ = raw
    valid = ~np.isnan(dist[:, 0])
    d = est.distance_domain(rank=2, p=0.1)
    plane = np.zeros(N, dtype=np.uint8)
    est.kneighbors_chunks(iter(cut(px)), nodata=NODATA, domain=d, domain_out=plane)
    one = est.distance_domain(rank=2, p=0.1)
    codes = est.domain_scores(one, px[valid].astype(np.float64))
    assert codes.dtype == np.uint8
    np.testing.assert_array_equal(codes, plane[valid])
    np.testing.assert_array_equal(one.hist, d.hist)
    assert one.n_beyond == d.n_beyond and one.n_nodata == 0
    # X=None: every fitted row among the others -- the table's own distances, so the codes are the ranks
    own = est.distance_domain()
    codes = est.domain_scores(own)
    np.testing.assert_array_equal(codes, own.percent(est.kneighbors()[0][:, 0]))
    assert own.n_pixels == 300 and codes.max() < 100


@pytest.mark.parametrize("kind", ["gnn", "rfnn"])
def test_transformed_estimators(moscow, kind):
    """The affine map (GNN, on Moscow) and the forest map (a small RFNN) on the device."""
    import sknnr_amd

    if kind == "gnn":
        X, y = moscow["X_train"], moscow["y_train"]
        est = sknnr_amd.GNNRegressor(n_neighbors=K, weights="distance").fit(X, y)
        rng = np.random.default_rng(7)
        px = np.tile(moscow["X_test"], (61, 1))[:N]
        px = px * (1.0 + 0.05 * rng.standard_normal(px.shape))
    else:
        X, y = reference_rows()
        est = sknnr_amd.RFNNRegressor(n_neighbors=K, n_estimators=10, random_state=0).fit(X, y)
        px = raster().astype(np.float64)
    assert est._map_on_device()
    dist, _ = est.kneighbors_chunks(iter(cut(px)))
    want = est.predict_chunks(iter(cut(px)))
    d = est.distance_domain(p=0.1)
    ref = est.regressor_.independent_kneighbors(np.arange(len(X)), n_neighbors=1)[0][:, 0]
    np.testing.assert_array_equal(d.table, np.sort(ref))
    assert d.threshold == float(np.quantile(d.table, 0.9))
    plane = np.zeros(N, dtype=np.uint8)
    got = est.predict_chunks(iter(cut(px)), domain=d, domain_out=plane)
    assert got.tobytes() == want.tobytes()
    expect(d, plane, dist)
    one = est.distance_domain(p=0.1)
    np.testing.assert_array_equal(est.domain_scores(one, px), plane)
    assert one == d
    blanked = est.predict_chunks(iter(cut(px)), domain=est.distance_domain(p=0.1), beyond="nodata")
    np.testing.assert_array_equal(blanked.reshape(N, -1), D.masked_predictions(want.reshape(N, -1), dist, 1, d.threshold))


def test_python_refusals(raw):
    import sknnr_amd

    est, px, _, _, _ = raw
    tiles = cut(px)
    d = est.distance_domain(p=0.05)
    plain = est.distance_domain()
    with pytest.raises(ValueError, match="rank=6 is above n_neighbors=5"):
        est.kneighbors_chunks(iter(tiles), domain=sknnr_amd.DistanceDomain(d.table, rank=6))
    with pytest.raises(ValueError, match="rank=3 is above n_neighbors=2"):
        est.kneighbors_chunks(iter(tiles), n_neighbors=2, domain=sknnr_amd.DistanceDomain(d.table, rank=3))
    with pytest.raises(ValueError, match="domain_out needs domain"):
        est.predict_chunks(iter(tiles), domain_out=np.zeros(N, dtype=np.uint8))
    for bad in (np.zeros(N, dtype=np.int8), np.zeros(2 * N, dtype=np.uint8)[::2], np.zeros((N, 1), dtype=np.uint8)):
        with pytest.raises(ValueError, match="domain_out must be"):
            est.predict_chunks(iter(tiles), domain=d, domain_out=bad)
    with pytest.raises(ValueError, match=f"domain_out holds {N - 1} pixels"):
        est.predict_chunks(iter(tiles), nodata=NODATA, domain=d, domain_out=np.zeros(N - 1, dtype=np.uint8))
    assert d.n_pixels == 0  # (a call that did not come through whole adds nothing)
    with pytest.raises(ValueError, match="needs a DistanceDomain with a threshold"):
        est.predict_chunks(iter(tiles), domain=plain, beyond="nodata")
    with pytest.raises(ValueError, match="out_nodata is required"):
        est.predict_chunks(iter(tiles), domain=d, beyond="nodata", out_dtype=np.int16)
    with pytest.raises(TypeError, match="DistanceDomain"):
        est.predict_chunks(iter(tiles), domain=d.table)
    X, y = reference_rows()
    called = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=lambda dd: 1.0 / (1.0 + dd)).fit(X, y)
    with pytest.raises(NotImplementedError, match="domain is not supported with callable weights"):
        called.predict_chunks(iter(tiles), domain=d)
    with sknnr_amd.tree_tie_policy("tree"):
        tree = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="kd_tree").fit(X, y)
        for call in (tree.kneighbors_chunks, tree.predict_chunks):
            with pytest.raises(NotImplementedError, match=r"domain is not supported under tree_tie_policy\('tree'\)"):
                call(iter(tiles), domain=d)
    with sknnr_amd.hamming_tie_policy("numpy"):
        ham = sknnr_amd.RFNNRegressor(n_neighbors=K, n_estimators=5, random_state=0).fit(X, y)
        for call in (ham.kneighbors_chunks, ham.predict_chunks):
            with pytest.raises(NotImplementedError, match=r"domain is not supported under hamming_tie_policy\('numpy'\)"):
                call(iter(tiles), domain=d)
    assert d.n_pixels == 0


def test_all_products_in_one_call_add_up_to_the_separate_calls_or_to_nothing():
    """usage, zonal and domain with ``domain_out`` in ONE ``predict_chunks`` call over two tiles of 8 pixels -- the smallest
    shape with two tiles and a partial last window: a ``domain_out`` one element short is refused at the second tile and
    leaves all three objects as they were; a whole call gives, byte for byte, what three calls with one keyword each
    give; and the replay of the stored neighbours does both just the same."""
    import copy

    import sknnr_amd

    rng = np.random.default_rng(5)
    X = rng.integers(0, 200, size=(64, 4)).astype(np.float64)
    y = np.column_stack([X[:, 0] + 0.25 * X[:, 1], X[:, 2] - X[:, 3]])
    est = sknnr_amd.RawKNNRegressor(n_neighbors=3).fit(X, y)
    px = rng.integers(0, 200, size=(16, 4)).astype(np.float64)
    zones = (np.arange(16) % 3).astype(np.int32)
    typed = dict(out_dtype=np.int16, scale=10.0)
    table = est.distance_domain().table

    def fresh():
        return sknnr_amd.NeighborUsage(), sknnr_amd.ZonalStats(3), sknnr_amd.DistanceDomain(table, threshold=table[40])

    # three separate calls, one keyword each: the expectation of every whole call below
    usage1, zonal1, domain1 = fresh()
    codes1 = np.full(16, 77, dtype=np.uint8)
    want = est.predict_chunks(iter(cut(px, (8, 8))), **typed)
    for one in (dict(usage=usage1), dict(zones=iter(cut(zones, (8, 8))), zonal=zonal1), dict(domain=domain1, domain_out=codes1)):
        assert est.predict_chunks(iter(cut(px, (8, 8))), **one, **typed).tobytes() == want.tobytes()
    assert want.dtype == np.int16 and usage1.n_rows == 16 and domain1.n_pixels == 16 and zonal1.n_planes == 2
    _, dist, idx = est.predict_chunks(iter(cut(px, (8, 8))), return_neighbors=True)

    def search(**kw):
        return est.predict_chunks(iter(cut(px, (8, 8))), **typed, **kw)

    def replay(**kw):
        return est.predict_neighbors_chunks(zip(cut(dist, (8, 8)), cut(idx, (8, 8))), **typed, **kw)

    for call in (search, replay):
        usage, zonal, domain = fresh()
        before = copy.deepcopy((usage, zonal, domain))
        with pytest.raises(ValueError, match="domain_out holds 15 pixels: the tiles hold at least 16"):
            call(usage=usage, zones=iter(cut(zones, (8, 8))), zonal=zonal, domain=domain,
                 domain_out=np.zeros(15, dtype=np.uint8))
        assert (usage, zonal, domain) == before
        assert usage.shape is None and zonal.n_planes is None and domain.n_pixels == 0
        codes = np.full(16, 77, dtype=np.uint8)
        got = call(usage=usage, zones=iter(cut(zones, (8, 8))), zonal=zonal, domain=domain, domain_out=codes)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        assert codes.tobytes() == codes1.tobytes()
        assert usage == usage1 and zonal == zonal1 and domain == domain1
        assert usage.counts.tobytes() == usage1.counts.tobytes() and zonal._acc.tobytes() == zonal1._acc.tobytes()
        assert domain.hist.tobytes() == domain1.hist.tobytes()
