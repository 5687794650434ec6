"""The side products of a streamed call (``sknnr_amd._products.StreamProducts``) without a device: a stub stream records
what the object hands to it -- the zone codes in lockstep with the tiles, the ``domain_out`` windows, the keywords of the
open call, the readers before ``close`` -- and the user's objects change only when a whole call is committed."""

from __future__ import annotations

import numpy as np
import pytest

import sknnr_amd
from sknnr_amd._products import _ZONES_LONG, _ZONES_SHORT, StreamProducts

N_REF, K, PLANES = 20, 3, 2
INT16 = dict(pred_dtype=np.dtype(np.int16), scale=None, offset=None, fill=None)
TABLE = np.arange(1.0, 11.0)
TALLY = (np.arange(N_REF * K, dtype=np.int64).reshape(N_REF, K), np.linspace(0.0, 2.0, N_REF))
ZONED = np.arange(3 * PLANES * 6, dtype=np.int64).reshape(3, PLANES, 6)
PLACED = np.arange(103, dtype=np.int64)
BOOTED = np.array([11, 40], dtype=np.int64)


def fitted(weights="uniform"):
    """A RawKNNRegressor in the state ``fit`` leaves it in, minus the device handle."""
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, weights=weights)
    rng = np.random.default_rng(0)
    est._fit_X, est._y = rng.standard_normal((N_REF, 6)), rng.standard_normal((N_REF, PLANES))
    est.n_features_in_, est.n_samples_fit_ = 6, N_REF
    est.effective_metric_, est.effective_metric_params_ = "euclidean", {}
    est._fit_method = "brute"
    est._affine = est._forest = est._ref_tree = est._engine = None
    return est


class StubStream:
    """Records every call; the readers answer fixed accumulators in the C ABI's form."""

    def __init__(self):
        self.calls = []

    def next_zones(self, codes):
        self.calls.append(("next_zones", codes))

    def next_domain_out(self, window):
        self.calls.append(("next_domain_out", window))

    def _read(name, value):
        def reader(self):
            self.calls.append((name,))
            return value
        return reader

    tally, zonal, domain, bootstrap = (_read("tally", TALLY), _read("zonal", (ZONED, None)), _read("domain", PLACED),
                                       _read("bootstrap", BOOTED))

    def close(self):
        self.calls.append(("close",))

    def names(self):
        return [c[0] for c in self.calls]


class StubEngine:
    def __init__(self):
        self.tables = []

    def set_bootstrap(self, table):
        self.tables.append(table)


def all_three(est, zones, domain_out=None):
    """usage + zonal + domain of one call, checked as ``predict_chunks`` checks them."""
    usage, zonal = sknnr_amd.NeighborUsage(), sknnr_amd.ZonalStats(3)
    domain = sknnr_amd.DistanceDomain(TABLE, threshold=4.0, rank=2)
    p = StreamProducts(usage=usage, zones=zones, zonal=zonal, domain=domain, domain_out=domain_out)
    p.check_usage(est, K)
    p.check_beyond()
    p.check_domain(est, K)
    p.check_zonal(est, PLANES, INT16)
    return p


def boot_products(est):
    boot = sknnr_amd.Bootstrap(n_replicates=4, seed=1, n_candidates=5)
    p = StreamProducts(bootstrap=boot)
    p.bootstrap_request(est, None, None)
    return p


def run(p, est, sizes, stream):
    """The feed of a streamed call over tiles of ``sizes`` pixels, then collect and close."""
    row = 0
    for n in sizes:
        p.next_tile()
        if n == 0:  # (an empty tile is skipped after its zone codes were taken)
            continue
        p.feed(stream, row, n)
        row += n
    p.end_of_tiles()
    try:
        p.collect(stream)
    finally:
        stream.close()
    return row


# ---- feed -----------------------------------------------------------------------------------------------------------------
def test_zone_entries_are_consumed_one_per_tile_empty_tiles_included():
    est, stream = fitted(), StubStream()
    entries = [np.full(3, 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.full((1, 5), 2, dtype=np.uint8)]
    p = all_three(est, entries)
    assert run(p, est, (3, 0, 5), stream) == 8
    fed = [c[1] for c in stream.calls if c[0] == "next_zones"]
    assert len(fed) == 2 and all(z.dtype == np.int32 and z.ndim == 1 for z in fed)  # (the empty tile's entry went unused)
    np.testing.assert_array_equal(fed[0], [1, 1, 1])
    np.testing.assert_array_equal(fed[1], [2] * 5)


def test_zones_short_and_long():
    est = fitted()
    with pytest.raises(ValueError) as err:
        run(all_three(est, [np.zeros(3, dtype=np.int32), np.zeros(0, dtype=np.int32)]), est, (3, 0, 5), StubStream())
    assert str(err.value) == _ZONES_SHORT
    stream = StubStream()
    with pytest.raises(ValueError) as err:
        run(all_three(est, [np.zeros(3, dtype=np.int32)] * 3), est, (3, 3), stream)
    assert str(err.value) == _ZONES_LONG
    assert "tally" not in stream.names()  # (refused after the last tile, before anything is read)


def test_domain_out_windows_and_the_short_plane():
    est, stream = fitted(), StubStream()
    codes = np.zeros(8, dtype=np.uint8)
    p = StreamProducts(domain=sknnr_amd.DistanceDomain(TABLE), domain_out=codes)
    p.check_domain(est, K)
    run(p, est, (3, 0, 5), stream)
    windows = [c[1] for c in stream.calls if c[0] == "next_domain_out"]
    assert [w.shape for w in windows] == [(3,), (5,)]
    for w, (a, b) in zip(windows, ((0, 3), (3, 8))):
        assert np.shares_memory(w, codes) and w.ctypes.data == codes[a:b].ctypes.data
    short, stream = np.zeros(7, dtype=np.uint8), StubStream()
    p = StreamProducts(domain=sknnr_amd.DistanceDomain(TABLE), domain_out=short)
    p.check_domain(est, K)
    with pytest.raises(ValueError, match="domain_out holds 7 pixels: the tiles hold at least 8"):
        run(p, est, (3, 0, 5), stream)
    assert stream.names() == ["next_domain_out"]  # (the first tile's window; refused at the third tile)


# ---- open -----------------------------------------------------------------------------------------------------------------
def test_open_keywords_of_each_product_alone_and_together():
    est, eng = fitted(), StubEngine()
    assert StreamProducts().open_keywords(eng, K) == {} and not StreamProducts()
    p = StreamProducts(usage=sknnr_amd.NeighborUsage())
    p.check_usage(est, K)
    assert p and p.open_keywords(eng, K) == dict(tally=True)

    p = StreamProducts(zones=[], zonal=sknnr_amd.ZonalStats(3, classes={1: 4}))
    p.check_zonal(est, PLANES, INT16)
    (name, (n_zones, n_classes)), = p.open_keywords(eng, K).items()
    assert name == "zonal" and n_zones == 3 and n_classes.dtype == np.int32
    np.testing.assert_array_equal(n_classes, [0, 4])
    p = StreamProducts(zones=[], zonal=sknnr_amd.ZonalStats(3))
    p.check_zonal(est, PLANES, INT16)
    assert p.open_keywords(eng, K) == dict(zonal=(3, None))

    for beyond, blank in (("keep", False), ("nodata", True)):
        domain = sknnr_amd.DistanceDomain(TABLE, threshold=4.0, rank=2)
        p = StreamProducts(domain=domain, beyond=beyond)
        assert p.check_beyond() is blank
        p.check_domain(est, K)
        kw = p.open_keywords(eng, K)
        assert set(kw) == {"domain"} and kw["domain"][0] is domain.table and kw["domain"][1:] == (2, 4.0, blank)

    p = all_three(est, [])
    kw = p.open_keywords(eng, K)
    assert list(kw) == ["tally", "zonal", "domain"] and kw["tally"] is True and kw["zonal"] == (3, None)
    assert kw["domain"][0] is p.domain.table and kw["domain"][1:] == (2, 4.0, False)
    assert eng.tables == []

    p = boot_products(est)
    kw = p.open_keywords(eng, K)
    kw_candidates, plan, table = p.request
    assert kw_candidates == 5 and set(kw) == {"bootstrap"} and kw["bootstrap"][0] == K and kw["bootstrap"][1] is plan
    assert len(eng.tables) == 1 and eng.tables[0] is table and table.shape == (4, N_REF)


# ---- collect and commit ---------------------------------------------------------------------------------------------------
def test_readers_run_once_each_and_before_close():
    est, stream = fitted(), StubStream()
    run(all_three(est, [np.zeros(4, dtype=np.int32)]), est, (4,), stream)
    assert stream.names() == ["next_zones", "tally", "zonal", "domain", "close"]
    stream = StubStream()
    run(boot_products(est), est, (4,), stream)
    assert stream.names() == ["bootstrap", "close"]


def test_nothing_is_added_unless_the_call_is_committed_and_commits_add_up():
    est = fitted()
    est.dataframe_index_in_ = np.arange(N_REF) + 100
    p, boot = all_three(est, [np.zeros(4, dtype=np.int32)]), boot_products(est)
    usage, zonal, domain, bootstrap = p.usage, p.zonal, p.domain, boot.bootstrap
    run(p, est, (4,), StubStream())
    run(boot, est, (4,), StubStream())
    # (a replay's unknown="raise" error is raised here, between collect and commit)
    assert usage.shape is None and zonal.n_planes is None and domain.n_pixels == 0
    assert (bootstrap.pixels, bootstrap.replicates_used) == (0, 0)
    p.commit(est, K)
    boot.commit(est, 5)
    assert usage.shape == (N_REF, K) and zonal.n_planes == PLANES
    np.testing.assert_array_equal(usage.counts, TALLY[0])
    np.testing.assert_array_equal(usage.ids, est.dataframe_index_in_)
    np.testing.assert_array_equal(zonal._acc[..., :4], ZONED[..., :4])
    assert domain.n_pixels == PLACED[:101].sum() and domain.n_beyond == 101
    assert (bootstrap.pixels, bootstrap.replicates_used) == (11, 40)
    # a second call on the same objects adds to them
    again = StreamProducts(usage=usage, zones=[np.zeros(4, dtype=np.int32)], zonal=zonal, domain=domain)
    again.check_usage(est, K)
    again.check_domain(est, K)
    again.check_zonal(est, PLANES, INT16)
    run(again, est, (4,), StubStream())
    again.commit(est, K)
    np.testing.assert_array_equal(usage.counts, 2 * TALLY[0])
    np.testing.assert_array_equal(zonal._acc[..., :4], 2 * ZONED[..., :4])
    assert domain.n_pixels == 2 * PLACED[:101].sum()
    more = StreamProducts(bootstrap=bootstrap)
    more.bootstrap_request(est, None, None)
    run(more, est, (4,), StubStream())
    more.commit(est, 5)
    assert (bootstrap.pixels, bootstrap.replicates_used) == (22, 80)


def test_a_call_without_a_pixel_binds_zonal_and_usage():
    est = fitted()
    p = all_three(est, [])
    p.end_of_tiles()
    p.commit(est, K)  # (no stream was opened: nothing was collected)
    assert p.usage.shape == (N_REF, K) and p.usage.counts.sum() == 0
    assert p.zonal.n_planes == PLANES and p.domain.n_pixels == 0


# ---- check: what can be checked now, and what needs k -----------------------------------------------------------------------
def test_checks_without_k_leave_the_rank_and_the_shape_to_settle():
    est = fitted()
    usage = sknnr_amd.NeighborUsage()
    usage._bind(N_REF, 2)
    p = StreamProducts(usage=usage, domain=sknnr_amd.DistanceDomain(TABLE, rank=3))
    p.check_usage(est)
    p.check_domain(est)
    with pytest.raises(ValueError, match="bound to"):
        p.settle(est, 3)
    with pytest.raises(ValueError, match="domain.rank=3 is above n_neighbors=2"):
        p.settle(est, 2)
    with pytest.raises(TypeError, match="usage must be a sknnr_amd.NeighborUsage"):
        StreamProducts(usage=object()).check_usage(est)
    with pytest.raises(ValueError, match="domain_out needs domain"):
        StreamProducts(domain_out=np.zeros(4, dtype=np.uint8)).check_domain(est)
    with pytest.raises(ValueError, match="zones and zonal come together"):
        StreamProducts(zonal=sknnr_amd.ZonalStats(3)).check_zonal(est, PLANES, INT16)
    with pytest.raises(NotImplementedError, match="zonal needs an integer out_dtype"):
        StreamProducts(zones=[], zonal=sknnr_amd.ZonalStats(3)).check_zonal(est, PLANES, None)
    with pytest.raises(ValueError, match="usage is not available with bootstrap="):
        StreamProducts(usage=usage, bootstrap=sknnr_amd.Bootstrap(n_replicates=2)).bootstrap_request(est, None, None)
