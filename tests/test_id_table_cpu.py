"""Dataframe ids on the device and neighbours beside predictions, the part that needs no device: the numpy restatement
of the lookup (tests/_id_table.py) on hand cases, every refusal ``predict_chunks`` promises to make before any device
work for its neighbour keywords, what the estimators hand to the stream with and without ``return_neighbors``, and the
argument errors of ``sknnr_narrow_ids`` / ``sknnr_stream_set_id_table`` that return before any device call."""

from __future__ import annotations

import ctypes
import types

import numpy as np
import pytest

import _id_table as IT


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_restatement_hand_cases():
    table = np.array([70, -5, 2**40, 0], dtype=np.int64)
    got = IT.lookup([[0, 1], [2, 3], [-1, 0]], table, fill=-9)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, [[70, -5], [2**40, 0], [-9, 70]])
    # the sign is tested on the index, not on the id: a negative id is an id
    np.testing.assert_array_equal(IT.lookup([1, -1], table, fill=0), [-5, 0])
    # a negative index never reaches the table -- numpy would wrap -1 to the last entry
    np.testing.assert_array_equal(IT.lookup([-1, -7], np.array([11, 22]), fill=5), [5, 5])
    # index 0 is an index
    np.testing.assert_array_equal(IT.lookup([0], np.array([33]), fill=5), [33])


def test_restatement_narrows_after_the_lookup():
    table = np.array([2**31 - 1, -2**31, 12], dtype=np.int64)
    got = IT.lookup([2, 0, -1, 1], table, fill=-1, dtype=np.int32)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, np.array([12, 2**31 - 1, -1, -2**31], dtype=np.int32))
    assert IT.lookup(np.empty((0, 3), dtype=np.int64), table).shape == (0, 3)


# ---- Python argument errors, on a fitted estimator, with no device ----------------------------------------------------
class _NoDevice:
    """Stands where the device engine would: any use beyond the target count is a failure of the test."""

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        raise AssertionError(f"the device engine was touched ({name}) before the arguments were refused")


def fitted(cls=None, y_cols=3, metric="euclidean", algorithm="brute", weights="uniform", ids=None, engine=None):
    """A RawKNNRegressor in the state ``fit`` leaves it in, minus the device handle."""
    import sknnr_amd

    est = (cls or sknnr_amd.RawKNNRegressor)(n_neighbors=3, weights=weights, algorithm=algorithm)
    rng = np.random.default_rng(0)
    est._fit_X = rng.standard_normal((20, 6))
    est._y = rng.standard_normal((20, y_cols)) if y_cols else rng.standard_normal(20)
    est.n_features_in_ = 6
    est.n_samples_fit_ = 20
    est.effective_metric_ = metric
    est.effective_metric_params_ = {}
    est._fit_method = algorithm
    est._affine = est._forest = est._ref_tree = None
    est._engine = engine if engine is not None else _NoDevice(max(y_cols, 1))
    if ids is not None:
        est.dataframe_index_in_ = np.asarray(ids)
    return est


TILES = [np.zeros((4, 6))]


@pytest.mark.parametrize("kwargs, match", [
    (dict(neighbors_out=(None, np.zeros((4, 3), dtype=np.int64))), "neighbors_out needs return_neighbors=True"),
    (dict(return_distance=False), "return_distance needs return_neighbors=True"),
    (dict(return_dataframe_index=True), "return_dataframe_index needs return_neighbors=True"),
    (dict(fill_index=0), "fill_index needs return_neighbors=True"),
    (dict(index_dtype=np.int32), "index_dtype needs return_neighbors=True"),
    (dict(distance_dtype=np.float32), "distance_dtype needs return_neighbors=True"),
])
def test_neighbor_keywords_need_return_neighbors(kwargs, match):
    with pytest.raises(ValueError, match=match):
        fitted().predict_chunks(TILES, **kwargs)


@pytest.mark.parametrize("kwargs, ids, match", [
    (dict(index_dtype=np.int16), None, "index_dtype=int16 is not supported"),
    (dict(distance_dtype=np.float16), None, "distance_dtype=float16 is not supported"),
    (dict(index_dtype=np.int32, nodata=0.0, fill_index=2**31), None, "fill_index=2147483648 is not representable"),
    (dict(index_dtype=np.int32, return_dataframe_index=True), np.arange(20) + 2**31, "needs integer dataframe ids"),
    (dict(index_dtype=np.int32, return_dataframe_index=True), np.array([f"p{i}" for i in range(20)]),
     "needs integer dataframe ids"),
    (dict(neighbors_out=(None,)), None, "neighbors_out must be"),
    (dict(out_dtype=np.int16, nodata=0.0), None, "out_nodata is required"),
])
def test_return_neighbors_refuses_before_any_device_work(kwargs, ids, match):
    with pytest.raises(ValueError, match=match):
        fitted(ids=ids).predict_chunks(TILES, return_neighbors=True, **kwargs)


def test_return_dataframe_index_needs_a_dataframe():
    from sklearn.exceptions import NotFittedError

    with pytest.raises(NotFittedError, match="fitted with a dataframe"):
        fitted().predict_chunks(TILES, return_neighbors=True, return_dataframe_index=True)


def test_host_side_paths_refuse_return_neighbors():
    import sknnr_amd

    with sknnr_amd.tree_tie_policy("tree"):
        with pytest.raises(NotImplementedError, match="return_neighbors is not supported under tree_tie_policy"):
            fitted(algorithm="kd_tree").predict_chunks(TILES, return_neighbors=True)
    with sknnr_amd.hamming_tie_policy("numpy"):
        with pytest.raises(NotImplementedError, match="return_neighbors is not supported under hamming_tie_policy"):
            fitted(metric="hamming").predict_chunks(TILES, return_neighbors=True)
    est = fitted(weights=lambda d: 1.0 / (1.0 + d))
    with pytest.raises(NotImplementedError, match="return_neighbors is not supported with callable weights"):
        est.predict_chunks(TILES, return_neighbors=True)
    with pytest.raises(ValueError, match="index_dtype needs return_neighbors=True"):  # (refused whatever the weights)
        est.predict_chunks(TILES, index_dtype=np.int32)


def transformed(reg):
    import sknnr_amd
    from sknnr_amd._base import TransformedKNeighborsRegressor

    est = sknnr_amd.EuclideanKNNRegressor(n_neighbors=3)
    assert isinstance(est, TransformedKNeighborsRegressor)
    est.regressor_ = reg
    est.transformer_ = types.SimpleNamespace()
    est._map_on_device = lambda: True
    return est


def test_transformed_estimators_pass_the_arguments_through():
    est = transformed(fitted())
    with pytest.raises(ValueError, match="fill_index needs return_neighbors=True"):
        est.predict_chunks(TILES, fill_index=0)
    with pytest.raises(ValueError, match="index_dtype=int16 is not supported"):
        est.predict_chunks(TILES, return_neighbors=True, index_dtype=np.int16)
    with pytest.raises(NotImplementedError, match="return_neighbors is not supported with callable weights"):
        transformed(fitted(weights=lambda d: d)).predict_chunks(TILES, return_neighbors=True)


# ---- what reaches the stream ---------------------------------------------------------------------------------------------
BEFORE = {"apply_affine", "weights", "return_distance", "use_deterministic_ordering", "out", "owner", "nodata", "bands",
          "output", "statistic"}  # the keywords predict_chunks handed to _stream_tiles before return_neighbors existed
BEFORE |= {"products"}  # (the call's side products as one object: empty in these calls)


def recording(est, k=3, t=3):
    """Replace the estimator's stream by a recorder that answers (dist, idx, pred) of the right shapes."""
    calls = []

    def stream_tiles(tiles, validate, k_, **kw):
        calls.append((k_, kw))
        n = sum(len(x) for x in tiles)
        nb = kw.get("neighbors", False)
        dist = np.zeros((n, k_)) if kw["return_distance"] else None
        idx = np.zeros((n, k_), dtype=(kw.get("output") or {}).get("index_dtype") or np.int64) if nb or kw["weights"] is None else None
        return dist, idx, (np.zeros((n, t)) if kw["weights"] is not None else None)

    est._stream_tiles = stream_tiles
    return calls


def engine_stub(t=3):
    return types.SimpleNamespace(t=t, d_in=6, pred_dtype=lambda weights: np.float64)


@pytest.mark.parametrize("wrap", [False, True])
def test_without_return_neighbors_nothing_new_reaches_the_stream(wrap):
    reg = fitted(engine=engine_stub(), ids=np.arange(20, dtype=np.int64) * 7)
    calls = recording(reg)
    est = transformed(reg) if wrap else reg
    pred = est.predict_chunks(TILES)
    assert pred.shape == (4, 3)
    (k, kw), = calls
    assert k == 3 and set(kw) == BEFORE and kw["return_distance"] is False and kw["output"] is None
    assert not kw["products"] and kw["products"].open_keywords(None, k) == {}
    pred = est.predict_chunks(TILES, return_neighbors=False, return_distance=True, return_dataframe_index=False,
                              neighbors_out=None, fill_index=-1, index_dtype=None, distance_dtype=None)
    assert set(calls[1][1]) == BEFORE and not calls[1][1]["products"] and not isinstance(pred, tuple)


@pytest.mark.parametrize("wrap", [False, True])
def test_return_neighbors_hands_the_table_and_the_types_to_one_stream(wrap):
    ids = np.arange(20, dtype=np.int32)[::-1] * 3
    reg = fitted(engine=engine_stub(), ids=ids)
    calls = recording(reg)
    est = transformed(reg) if wrap else reg
    o_idx = np.zeros((4, 3), dtype=np.int32)
    res = est.predict_chunks(TILES, nodata=-1.0, out_dtype=np.int16, out_nodata=-32768, return_neighbors=True,
                             return_dataframe_index=True, fill_index=0, index_dtype=np.int32,
                             distance_dtype=np.float32, neighbors_out=(None, o_idx))
    assert len(res) == 3 and len(calls) == 1
    k, kw = calls[0]
    assert k == 3 and kw["neighbors"] is True and kw["return_distance"] is True and kw["use_deterministic_ordering"] is True
    assert kw["id_table"].dtype == np.int64 and kw["id_table"].flags.c_contiguous
    np.testing.assert_array_equal(kw["id_table"], ids)
    assert kw["fill_index"] == -1 and kw["fill_id"] == 0  # (the expansion writes -1; the lookup turns it into the caller's fill)
    assert kw["output"] == dict(pred_dtype=np.dtype(np.int16), scale=None, offset=None, fill=-32768.0,
                                index_dtype=np.dtype(np.int32), distance_dtype=np.dtype(np.float32))
    assert kw["out"][0] is None and kw["out"][1] is o_idx and kw["out"][2] is None
    # without distances: (pred, idx), and row indices keep the caller's fill_index on the stream itself
    res = est.predict_chunks(TILES, nodata=-1.0, return_neighbors=True, return_distance=False, fill_index=7)
    assert len(res) == 2 and res[1].dtype == np.int64
    kw = calls[1][1]
    assert kw["id_table"] is None and kw["fill_index"] == 7 and kw["return_distance"] is False and kw["out"] is None


def test_kneighbors_chunks_hands_integer_tables_to_the_stream_and_keeps_labels_on_the_host():
    for ids, on_device in ((np.arange(20, dtype=np.int64) + 5, True), (np.arange(20, dtype=np.int16), True),
                           (np.arange(20, dtype=np.uint32), True), (np.arange(20, dtype=np.uint64), False),
                           (np.array([f"p{i}" for i in range(20)]), False), (np.arange(20) * 0.5, False)):
        reg = fitted(engine=engine_stub(), ids=ids)
        calls = recording(reg)
        dist, idx = reg.kneighbors_chunks(TILES, return_dataframe_index=True, nodata=-1.0, fill_index=0)
        kw = calls[0][1]
        assert kw["fill_index"] == -1 and kw["fill_id"] == 0
        if on_device:
            assert kw["id_table"].dtype == np.int64
            np.testing.assert_array_equal(kw["id_table"], ids)
            assert idx.dtype == ids.dtype  # (the one astype of a table that is not int64, as kneighbors does)
        else:
            assert kw["id_table"] is None
            assert idx.dtype == ids.dtype and idx[0, 0] == ids[0]  # the host looked index 0 up
    import sknnr_amd

    with sknnr_amd.tree_tie_policy("tree"):  # the host answers tile by tile: no table for a stream that is never opened
        assert fitted(algorithm="kd_tree", ids=np.arange(20))._device_id_table(True) is None
    assert fitted(ids=np.arange(20))._device_id_table(False) is None


# ---- C argument errors, without a device ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    import os

    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_narrow_ids_argument_errors_without_touching_a_device(native):
    lib = native.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    wide = ctypes.c_int32(7)

    def call(src=p, n=4, c=2, table=p, n_table=8, has_fill=1, fill_id=-1, dst=p, dtype=0, stride=0):
        return lib.sknnr_narrow_ids(src, n, c, table, n_table, has_fill, fill_id, dst, dtype, stride, 0, None,
                                    ctypes.byref(wide))

    inv = native.ERR_INVALID
    assert call(table=None) == inv and b"table is NULL" in lib.sknnr_last_error()
    assert call(n_table=0) == inv and call(n_table=-3) == inv and b"n_table" in lib.sknnr_last_error()
    for dtype in (1, 2, 3, 4, 6, -1, 99):  # ids leave as int64 or int32
        assert call(dtype=dtype) == inv
    assert b"int64 (0) or int32" in lib.sknnr_last_error()
    assert call(n=-1) == inv and b"n must be" in lib.sknnr_last_error()
    assert call(c=0) == inv and call(c=65537) == inv and b"outside [1, 65536]" in lib.sknnr_last_error()
    assert call(stride=3) == inv and b"below n" in lib.sknnr_last_error()
    assert call(src=None) == inv and call(dst=None) == inv and b"NULL" in lib.sknnr_last_error()
    assert call(n=0, table=None) == inv and call(n=0, n_table=0) == inv  # the table is looked at before n == 0
    assert wide.value == 0
    assert call(n=0, src=None, dst=None) == 0 and call(n=0, dtype=5) == 0
    assert lib.sknnr_stream_set_id_table(None, p, 8, -1) == inv and b"stream is NULL" in lib.sknnr_last_error()
    # plain sknnr_narrow still has no int64 -> int64 pair: without a table there is nothing to do
    assert lib.sknnr_narrow(p, 1, 4, 2, p, 0, 0, None, None, 0, 0.0, 0, None, ctypes.byref(wide)) == inv
