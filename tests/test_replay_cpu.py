"""Neighbour replay without a device: the numpy restatement (tests/_replay.py) against a plain Python loop on tiny inputs,
every refusal of ``predict_neighbors_chunks`` raised before the engine is touched, the new C entries declared in the
header, listed in ``_native.EXPORTED_SYMBOLS`` and refusing NULL handles, and a duplicate id table refused before the
handle is looked at.

Without the feature the estimator tests fail with ``AttributeError`` (no ``predict_neighbors_chunks``) and the symbol
tests on the missing names."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import _replay as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sknnr_index_create_targets", "sknnr_index_set_replay_ids", "sknnr_replay_begin", "sknnr_replay_push",
               "sknnr_replay_push_planes", "sknnr_replay_get_counts", "sknnr_debug_last_replay")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def tiny(idx_dtype, dist_dtype, ids, seed):
    rng = np.random.default_rng(seed)
    n_ref, n, ks = 9, 40, 4
    table = None
    idx = rng.integers(0, n_ref, size=(n, ks))
    if ids:
        table = rng.permutation(np.array([-7, -1, 0, 3, 4, 10, 2**31 + 5 if idx_dtype == np.int64 else 99, 12, 50]))
        idx = table[idx]
    idx = idx.astype(idx_dtype)
    fill = -1 if not ids else -5
    idx[::8, 0] = fill                      # masked: the first column decides ...
    idx[::8, 1:] = 10**6                    # ... whatever the others hold
    idx[3, 0] = 10**5                       # unknown in column 0
    idx[5, 2] = -3 if not ids else 7        # unknown in the last used column (k = 3)
    idx[6, 3] = 10**5                       # an unused column: must not count
    idx[7, 1] = fill                        # the fill value in another column is an ordinary (here unknown) value
    dist = None if dist_dtype is None else rng.uniform(0.0, 4.0, size=(n, ks)).astype(dist_dtype)
    return idx, dist, n_ref, fill, table


@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("dist_dtype", [None, np.float32, np.float64])
@pytest.mark.parametrize("ids", [False, True])
def test_restatement_equals_the_loop(idx_dtype, dist_dtype, ids):
    idx, dist, n_ref, fill, table = tiny(idx_dtype, dist_dtype, ids, 3)
    for k in (3, 1, 4):
        got = RP.decode(idx, dist, k, n_ref, fill, table)
        want = RP.decode_loop(idx, dist, k, n_ref, fill, table)
        for g, w in zip(got, want):
            if w is None:
                assert g is None
            else:
                np.testing.assert_array_equal(g, w)
        assert got[0].dtype == np.int64 and (got[1] is None or got[1].dtype == np.float64)
    i3, d3, masked, unknown = RP.decode(idx, dist, 3, n_ref, fill, table)
    assert masked.sum() == 5 and list(np.flatnonzero(unknown)) == [3, 5, 7] and not unknown[6]
    assert (i3[masked | unknown] == -1).all() and (d3 is None or np.isnan(d3[masked | unknown]).all())
    if d3 is not None:  # widening is exact
        np.testing.assert_array_equal(d3[~(masked | unknown)], dist[~(masked | unknown), :3].astype(np.float64))
    # band-first planes decode to the same tile
    planes = (np.ascontiguousarray(idx.T).reshape(4, 5, 8), None if dist is None else np.ascontiguousarray(dist.T).reshape(4, 5, 8))
    for g, w in zip(RP.decode(planes[0], planes[1], 3, n_ref, fill, table, bands=True), (i3, d3, masked, unknown)):
        if w is not None:
            np.testing.assert_array_equal(g, w)


def test_restatement_reduces_the_good_pixels_only():
    idx, dist, n_ref, fill, _ = tiny(np.int64, np.float64, False, 4)
    y = np.random.default_rng(0).standard_normal((n_ref, 2))
    i3, d3, masked, unknown = RP.decode(idx, dist, 3, n_ref, fill)
    pred = RP.reduce(y, i3, d3, "uniform")
    assert np.isnan(pred[masked | unknown]).all() and not np.isnan(pred[~(masked | unknown)]).any()
    np.testing.assert_array_equal(pred[~(masked | unknown)], y[i3[~(masked | unknown)]].mean(axis=1))
    assert RP.reduce(y, i3, d3, "distance", outputs=[(1, ("quantile", 0.5)), (0, "max"), (1, "mean")]).shape == (len(idx), 3)


# ---- Python-level refusals, raised without a device -------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device engine was touched ({name}) before the arguments were refused")


def fitted(weights="uniform", ids=None, y_cols=3, k=3):
    """A RawKNNRegressor in the state ``fit`` leaves it in, minus the device handle."""
    import sknnr_amd

    est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights)
    rng = np.random.default_rng(0)
    est._fit_X = rng.standard_normal((20, 6))
    est._y = rng.standard_normal((20, y_cols)) if y_cols else rng.standard_normal(20)
    est.n_features_in_, est.n_samples_fit_ = 6, 20
    est.effective_metric_, est.effective_metric_params_ = "euclidean", {}
    est._fit_method = "brute"
    est._affine = est._forest = est._ref_tree = None
    est._device = 0
    est._engine = _NoDevice()
    if ids is not None:
        est.dataframe_index_in_ = np.asarray(ids)
    return est


IDX = np.zeros((4, 5), dtype=np.int32)
DIST = np.zeros((4, 5), dtype=np.float32)


@pytest.mark.parametrize("tiles, kwargs, match", [
    ([IDX], dict(unknown="skip"), "unknown must be 'raise' or 'nodata'"),
    ([IDX], dict(layout="columns"), "layout must be"),
    ([IDX], dict(beyond="drop"), "beyond must be"),
    ([IDX], dict(fill_index=1.5), "fill_index must be an integer"),
    ([IDX], dict(n_neighbors=0), "n_neighbors must be a positive integer"),
    ([IDX], dict(n_neighbors=6), "n_neighbors=6 is above the 5 stored neighbour columns"),
    ([IDX], dict(y=np.zeros((19, 2))), "y has 19 rows"),
    ([IDX], dict(y=np.array([["a"] * 2] * 20)), "y must be a numeric"),
    ([IDX], dict(statistic=["mean", "mean"]), "one name per target"),
    ([IDX], dict(y=np.zeros((20, 4)), statistic=["mean"] * 3), r"one name per target \(4\)"),
    ([IDX], dict(outputs=[(3, "mean")]), r"target 3 is outside \[0, 3\)"),
    ([IDX], dict(scale=2.0), "scale needs out_dtype"),
    ([IDX], dict(out_dtype=np.int16, unknown="nodata"), "out_nodata is required"),
    ([IDX], dict(out_dtype=np.uint8, out_nodata=300), "not representable"),
    ([IDX], dict(zones=[np.zeros(4, dtype=np.int32)]), "zones and zonal come together"),
    ([IDX], dict(domain_out=np.zeros(4, dtype=np.uint8)), "domain_out needs domain"),
    ([IDX], dict(beyond="nodata"), "needs domain"),
    ([IDX.astype(np.float32)], {}, "tile 0: stored neighbours are int32 or int64"),
    ([IDX.astype(np.uint64)], {}, "tile 0: stored neighbours are int32 or int64"),
    ([(DIST.astype(np.float16), IDX)], {}, "tile 0: stored distances are float32 or float64"),
    ([(DIST[:3], IDX)], {}, "tile 0: the distances have shape"),
    ([IDX[0]], {}, "tile 0: a tile of stored neighbours is"),
    ([IDX[:0], IDX[:0].astype(np.int64)], {}, "tile 1: the tiles of one call share one ks and one dtype pair"),
    ([IDX[:0], IDX[:0, :4]], {}, "tile 1: the tiles of one call share"),
    ([(DIST[:0], IDX[:0]), IDX[:0]], {}, "tile 1: the tiles of one call share"),
])
def test_refusals_need_no_device(tiles, kwargs, match):
    with pytest.raises(ValueError, match=match):
        fitted().predict_neighbors_chunks(tiles, **kwargs)


def test_distances_missing_is_refused_before_any_device_work():
    import sknnr_amd
    from sknnr_amd import weights as W

    with pytest.raises(ValueError, match="weights='distance' needs the stored distances"):
        fitted("distance").predict_neighbors_chunks([IDX])
    with pytest.raises(ValueError, match="a weight law needs the stored distances"):
        fitted(W.InverseDistance()).predict_neighbors_chunks([IDX])
    with pytest.raises(ValueError, match="usage needs the stored distances"):
        fitted().predict_neighbors_chunks([IDX], usage=sknnr_amd.NeighborUsage())
    with pytest.raises(TypeError, match="usage must be a sknnr_amd.NeighborUsage"):
        fitted().predict_neighbors_chunks([IDX], usage=object())
    with pytest.raises(TypeError, match="domain must be a sknnr_amd.DistanceDomain"):
        fitted().predict_neighbors_chunks([IDX], domain=object())
    with pytest.raises(TypeError, match="zonal must be a sknnr_amd.ZonalStats"):
        fitted().predict_neighbors_chunks([IDX], zones=[np.zeros(4)], zonal=object(), out_dtype=np.int16)


def test_callable_weights_and_host_tie_policies_are_refused():
    with pytest.raises(NotImplementedError, match="predict_neighbors_chunks is not supported with callable weights"):
        fitted(lambda d: 1.0 / (1.0 + d)).predict_neighbors_chunks([(DIST, IDX)])


def test_ids_refusals():
    from sklearn.exceptions import NotFittedError

    with pytest.raises(NotFittedError, match="ids=True needs an estimator fitted with a dataframe"):
        fitted().predict_neighbors_chunks([IDX], ids=True)
    with pytest.raises(NotImplementedError, match="ids=True needs integer dataframe ids"):
        fitted(ids=[f"p{i}" for i in range(20)]).predict_neighbors_chunks([IDX], ids=True)
    with pytest.raises(ValueError, match="fit int64"):
        fitted(ids=np.arange(20, dtype=np.uint64)).predict_neighbors_chunks([IDX], ids=True)
    with pytest.raises(ValueError, match="unique dataframe ids"):
        fitted(ids=np.arange(20) // 2).predict_neighbors_chunks([IDX], ids=True)


def test_one_tile_entry_and_wrappers_exist():
    import inspect

    import sknnr_amd

    for cls in (sknnr_amd.RawKNNRegressor, sknnr_amd.GNNRegressor, sknnr_amd.RFNNRegressor):
        assert callable(getattr(cls, "predict_neighbors_chunks")) and callable(getattr(cls, "predict_neighbors"))
    sig = inspect.signature(sknnr_amd.RawKNNRegressor.predict_neighbors_chunks)
    assert list(sig.parameters)[1:] == ["neighbor_tiles", "y", "n_neighbors", "ids", "fill_index", "unknown", "out", "layout",
                                        "out_dtype", "scale", "offset", "out_nodata", "statistic", "outputs", "usage", "zones",
                                        "zonal", "domain", "domain_out", "beyond"]
    with pytest.raises(ValueError, match="tile 0: a tile of stored neighbours is"):
        fitted().predict_neighbors(IDX[0])


# ---- the C surface -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entries():
    from sknnr_amd import _native

    with open(os.path.join(ROOT, "include", "sknnr_hip.h")) as f:
        header = f.read()
    assert "Neighbour replay.  THE CONTRACT" in header
    for name in NEW_SYMBOLS:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _native.EXPORTED_SYMBOLS, name
    assert re.search(r"#define SKNNR_ABI_VERSION 5\b", header)


@pytest.fixture(scope="module")
def native():
    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_new_entries_refuse_null_handles(native):
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.sknnr_abi_version() == 5
    out8 = (ctypes.c_int64 * 8)()
    h = ctypes.c_void_p()
    idx = (ctypes.c_int64 * 5)()
    ids = (ctypes.c_int64 * 3)(4, 5, 6)

    def refused(rc, what):
        assert rc == native.ERR_INVALID and what in lib.sknnr_last_error(), lib.sknnr_last_error()

    refused(lib.sknnr_index_create_targets(None, 3, 1, 0, ctypes.byref(h)), b"sknnr_index_create_targets")
    refused(lib.sknnr_index_create_targets(None, 3, 1, 0, None), b"out is NULL")
    refused(lib.sknnr_index_set_replay_ids(None, ids, 3), b"index is NULL")
    refused(lib.sknnr_replay_begin(None, 1, 1, 0, 0, 0, native.REPLAY_NO_DIST, -1, 0, 0, 1, ctypes.byref(h)), b"index is NULL")
    refused(lib.sknnr_replay_begin(None, 1, 1, 0, 0, 0, native.REPLAY_NO_DIST, -1, 0, 0, 1, None), b"out is NULL")
    refused(lib.sknnr_replay_push(None, idx, None, 1, None, None, None), b"stream is NULL")
    refused(lib.sknnr_replay_push_planes(None, idx, None, 1, 1, None, None, None, 1), b"stream is NULL")
    refused(lib.sknnr_replay_get_counts(None, out8), b"stream is NULL")
    refused(lib.sknnr_debug_last_replay(None, out8), b"NULL argument")


def test_a_duplicate_id_table_is_refused_before_the_handle_is_looked_at(native):
    lib = native.load()
    dup = (ctypes.c_int64 * 4)(7, -2, 9, -2)
    assert lib.sknnr_index_set_replay_ids(None, dup, 4) == native.ERR_INVALID
    msg = lib.sknnr_last_error()
    assert b"id -2 names rows 1 and 3" in msg and b"unique" in msg, msg
    ok = (ctypes.c_int64 * 4)(7, -2, 9, 2**40)
    assert lib.sknnr_index_set_replay_ids(None, ok, 4) == native.ERR_INVALID
    assert b"index is NULL" in lib.sknnr_last_error()


def test_instance_codes_match_the_header():
    from sknnr_amd import _native

    assert _native.replay_instance(np.int32, None, False) == 0
    assert _native.replay_instance(np.int32, np.float32, True) == 3
    assert _native.replay_instance(np.int64, np.float64, False) == 10
    assert _native.replay_instance(np.int64, np.float64, True) == 11
