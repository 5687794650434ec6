"""Distance domain without a GPU: ``DistanceDomain`` (validation, ``percent`` against the contract's formula and its
properties, value semantics, pickle), the refusals of ``domain=`` / ``domain_out=`` / ``beyond=`` that come before any
device work, the new C symbols, and the one-shot entry's own refusals, which need no handle.

Without the feature every test here fails: the class, the keywords and the symbols do not exist."""

from __future__ import annotations

import ctypes
import pickle

import numpy as np
import pytest

import _domain as D


def test_table_is_validated_sorted_and_read_only():
    import sknnr_amd

    raw = np.array([3.0, 0.5, -0.0, 2.0, 0.5])
    d = sknnr_amd.DistanceDomain(raw)
    np.testing.assert_array_equal(d.table, [0.0, 0.5, 0.5, 2.0, 3.0])
    assert not np.signbit(d.table[0]) and d.table.dtype == np.float64 and not d.table.flags.writeable
    np.testing.assert_array_equal(raw, [3.0, 0.5, -0.0, 2.0, 0.5])  # (the caller's array is not sorted in place)
    assert d.rank == 1 and d.threshold is None
    assert sknnr_amd.DistanceDomain([1, 2, 3], threshold=2, rank=3).threshold == 2.0
    for bad in ([1.0, np.nan], [1.0, -1e-300], [np.inf, 1.0], [], np.empty((0, 3))):
        with pytest.raises(ValueError, match="table"):
            sknnr_amd.DistanceDomain(bad)
    for rank in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="rank"):
            sknnr_amd.DistanceDomain([1.0], rank=rank)
    for thr in (np.nan, -0.5, np.inf):
        with pytest.raises(ValueError, match="threshold"):
            sknnr_amd.DistanceDomain([1.0], threshold=thr)


def test_percent_is_the_contract_formula():
    import sknnr_amd

    rng = np.random.default_rng(3)
    table = np.sort(np.round(rng.gamma(2.0, 1.5, size=997), 1))  # (one decimal: many duplicates)
    d = sknnr_amd.DistanceDomain(rng.permutation(table))
    s = np.concatenate([table, np.nextafter(table, np.inf), np.nextafter(table, -np.inf), (table[1:] + table[:-1]) / 2,
                        [0.0, -0.0, -1.0, np.inf, np.nan, table[-1] * 2]])
    got = d.percent(s)
    assert got.dtype == np.uint8 and got.shape == s.shape
    # the formula, entry by entry, in Python integers
    for v, g in zip(s, got):
        want = 255 if np.isnan(v) else (100 * int(np.sum(table < v))) // table.size
        assert g == want, (v, g, want)
    np.testing.assert_array_equal(got, D.codes(s[:, None], table, 1))
    np.testing.assert_array_equal(d.percent(s[:3992].reshape(2, 4, -1)), got[:3992].reshape(2, 4, -1))  # (any shape)
    # monotone in s
    order = np.argsort(s[~np.isnan(s)], kind="stable")
    assert np.all(np.diff(got[~np.isnan(s)][order].astype(int)) >= 0)
    # 100 iff above the maximum; a tie is not above
    finite = ~np.isnan(s)
    np.testing.assert_array_equal(got[finite] == 100, s[finite] > table[-1])
    assert d.percent(table[-1]) < 100 and d.percent(np.nextafter(table[-1], np.inf)) == 100
    lo = sknnr_amd.DistanceDomain([2.0, 2.0, 2.0, 2.0])
    np.testing.assert_array_equal(lo.percent([1.9, 2.0, np.nextafter(2.0, 3.0), 0.0, -0.0]), [0, 0, 100, 0, 0])
    assert d.percent(np.nan) == 255 and d.percent(np.inf) == 100 and d.percent(-0.0) == 0
    # a single entry: everything is 0 or 100
    one = sknnr_amd.DistanceDomain([1.5])
    np.testing.assert_array_equal(one.percent([0.0, 1.5, 1.6]), [0, 0, 100])


def test_model_on_a_hand_written_case():
    table = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 4.0, 4.0])  # m = 8
    dist = np.array([[9.0, 0.0], [9.0, 1.0], [9.0, 1.5], [9.0, 4.0], [9.0, 4.5], [9.0, np.nan], [9.0, -0.0], [9.0, np.inf]])
    np.testing.assert_array_equal(D.codes(dist, table, 2), [0, 25, 62, 75, 100, 255, 0, 100])
    a = D.acc(dist, table, 2, threshold=1.0)
    assert a[0] == 2 and a[25] == 1 and a[62] == 1 and a[75] == 1 and a[100] == 2
    assert a[:101].sum() == 7 and a[D.BEYOND] == 4 and a[D.NODATA] == 1
    assert D.acc(dist, table, 2)[D.BEYOND] == 0
    np.testing.assert_array_equal(D.codes(dist, table, 1), np.full(8, 100))
    pred = np.arange(16.0).reshape(8, 2)
    out = D.masked_predictions(pred, dist, 2, 1.0)
    np.testing.assert_array_equal(np.isnan(out).all(1), [False, False, True, True, True, False, False, True])
    np.testing.assert_array_equal(out[:2], pred[:2])


def test_value_semantics_and_pickle():
    import sknnr_amd

    table = [0.5, 1.0, 2.0]
    a = sknnr_amd.DistanceDomain(table, threshold=1.0)
    assert a.n_pixels == 0 and a.n_beyond == 0 and a.n_nodata == 0 and np.isnan(a.share_beyond)
    assert a.hist.shape == (101,) and a.hist.dtype == np.int64
    acc = np.zeros(103, dtype=np.int64)
    acc[[0, 33, 100, 101, 102]] = [4, 3, 2, 5, 7]
    a._add(acc)
    assert (a.n_pixels, a.n_beyond, a.n_nodata) == (9, 5, 7) and a.share_beyond == 5 / 9
    assert a.hist[33] == 3
    b = pickle.loads(pickle.dumps(a))
    assert b == a and not b.table.flags.writeable and b.threshold == 1.0 and b.rank == 1
    b += a
    assert b != a and b.n_pixels == 18 and b.n_nodata == 14
    assert a == sknnr_amd.DistanceDomain([2.0, 0.5, 1.0], threshold=1.0)._add(acc)
    assert a != sknnr_amd.DistanceDomain(table, threshold=1.0)          # other tallies
    assert sknnr_amd.DistanceDomain(table) != sknnr_amd.DistanceDomain(table, threshold=1.0)
    assert (a == 3) is False
    for other in (sknnr_amd.DistanceDomain(table), sknnr_amd.DistanceDomain(table, threshold=1.0, rank=2),
                  sknnr_amd.DistanceDomain([0.5, 1.0, 2.5], threshold=1.0)):
        with pytest.raises(ValueError, match="equal table, threshold and rank"):
            a += other
    with pytest.raises(TypeError):
        a += 1
    with pytest.raises(TypeError):
        hash(a)
    assert "m=3" in repr(a) and "n_beyond=5" in repr(a)


class _Fitted:
    """An estimator that looks fitted but has no engine: a refusal that comes before any device work never needs one."""

    def __new__(cls, k=5, weights="uniform"):
        import sknnr_amd

        est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights)
        est._fit_X = np.zeros((12, 3))
        est._y = np.zeros((12, 2))
        est.n_samples_fit_, est.n_features_in_ = 12, 3
        est._fit_method = "brute"
        return est


def test_refusals_need_no_device():
    import inspect

    import sknnr_amd

    tiles = [np.zeros((4, 3))]
    est = _Fitted()
    plain = sknnr_amd.DistanceDomain([1.0, 2.0])
    thr = sknnr_amd.DistanceDomain([1.0, 2.0], threshold=1.5)
    plane = np.zeros(4, dtype=np.uint8)
    for call in (est.kneighbors_chunks, est.predict_chunks):
        with pytest.raises(TypeError, match="DistanceDomain"):
            call(iter(tiles), domain=object())
        with pytest.raises(ValueError, match="domain_out needs domain"):
            call(iter(tiles), domain_out=plane)
        with pytest.raises(ValueError, match="rank=6 is above n_neighbors=5"):
            call(iter(tiles), domain=sknnr_amd.DistanceDomain([1.0], rank=6))
        for bad in (np.zeros(4, dtype=np.int8), np.zeros(8, dtype=np.uint8)[::2], np.zeros((4, 1), dtype=np.uint8),
                    [0, 0, 0, 0]):
            with pytest.raises(ValueError, match="domain_out must be"):
                call(iter(tiles), domain=plain, domain_out=bad)
    with pytest.raises(ValueError, match="rank=3 is above n_neighbors=2"):
        est.kneighbors_chunks(iter(tiles), n_neighbors=2, domain=sknnr_amd.DistanceDomain([1.0], rank=3))
    # the mask
    with pytest.raises(ValueError, match="beyond must be"):
        est.predict_chunks(iter(tiles), domain=thr, beyond="drop")
    with pytest.raises(ValueError, match="needs a DistanceDomain with a threshold"):
        est.predict_chunks(iter(tiles), domain=plain, beyond="nodata")
    with pytest.raises(ValueError, match="beyond='nodata' needs domain"):
        est.predict_chunks(iter(tiles), beyond="nodata")
    with pytest.raises(ValueError, match="out_nodata is required"):
        est.predict_chunks(iter(tiles), domain=thr, beyond="nodata", out_dtype=np.int16)
    # a callable runs on the host between the search and the reduction
    with pytest.raises(NotImplementedError, match="domain is not supported with callable weights"):
        _Fitted(weights=lambda d: 1.0 / (1.0 + d)).predict_chunks(iter(tiles), domain=plain)
    # the host-side tie policies answer tile by tile on the host
    with sknnr_amd.tree_tie_policy("tree"):
        tree = _Fitted()
        tree._fit_method = "kd_tree"
        for call in (tree.kneighbors_chunks, tree.predict_chunks):
            with pytest.raises(NotImplementedError, match=r"domain is not supported under tree_tie_policy\('tree'\)"):
                call(iter(tiles), domain=plain)
    with sknnr_amd.hamming_tie_policy("numpy"):
        ham = _Fitted()
        ham.effective_metric_ = "hamming"
        for call in (ham.kneighbors_chunks, ham.predict_chunks):
            with pytest.raises(NotImplementedError, match=r"domain is not supported under hamming_tie_policy\('numpy'\)"):
                call(iter(tiles), domain=plain)
    # the one-shot entries
    with pytest.raises(TypeError, match="DistanceDomain"):
        est.domain_scores(object())
    with pytest.raises(ValueError, match="rank=6 is above n_neighbors=5"):
        est.domain_scores(sknnr_amd.DistanceDomain([1.0], rank=6))
    for bad in (dict(p=0.1, threshold=1.0), dict(p=0.0), dict(p=1.0), dict(rank=0)):
        with pytest.raises(ValueError, match="mutually exclusive|inside \\(0, 1\\)|rank must be"):
            est.distance_domain(**bad)
    # the transformed family takes the keywords too
    for cls in (sknnr_amd.RawKNNRegressor, sknnr_amd.GNNRegressor, sknnr_amd.RFNNRegressor):
        for name in ("domain", "domain_out", "beyond"):
            assert name in inspect.signature(cls.predict_chunks).parameters
        for name in ("domain", "domain_out"):
            assert name in inspect.signature(cls.kneighbors_chunks).parameters
        assert callable(cls.distance_domain) and callable(cls.domain_scores)


@pytest.fixture(scope="module")
def native():
    import os

    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


NEW_SYMBOLS = ("sknnr_domain_from_neighbors", "sknnr_stream_set_domain", "sknnr_stream_next_domain_out",
               "sknnr_stream_get_domain", "sknnr_debug_last_domain", "sknnr_debug_domain_geometry")


def test_new_symbols_are_exported_and_the_abi_stays_5(native):
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert lib.sknnr_abi_version() == 5
    acc = (ctypes.c_int64 * 103)()
    out = (ctypes.c_int64 * 8)()
    table = (ctypes.c_double * 1)(1.0)
    plane = (ctypes.c_uint8 * 1)()
    assert lib.sknnr_stream_set_domain(None, table, 1, 1, 0, 0.0, 0) == native.ERR_INVALID
    assert b"stream is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_stream_next_domain_out(None, plane, 1) == native.ERR_INVALID
    assert lib.sknnr_stream_get_domain(None, acc) == native.ERR_INVALID
    assert lib.sknnr_debug_last_domain(None, out) == native.ERR_INVALID
    assert lib.sknnr_debug_domain_geometry(0, out) == native.ERR_INVALID
    assert lib.sknnr_debug_domain_geometry(2**31, out) == native.ERR_INVALID
    geo = native.domain_geometry(1)  # (no device work)
    assert geo["pixels_per_workgroup"] >= 1 and geo["skeleton"] >= 1 and geo["stride"] == 1 and geo["skeleton_used"] == 1
    s = geo["skeleton"]
    for m in (s - 1, s, s + 1, 2 * s + 1, 40_000, 2**31 - 1):
        g = native.domain_geometry(m)
        # the skeleton spans the table: entries j * stride below m, at most `skeleton` of them, none wasted
        assert 1 <= g["skeleton_used"] <= s and (g["skeleton_used"] - 1) * g["stride"] < m <= g["skeleton_used"] * g["stride"], g
        assert g["stride"] == -(-m // s), g


def test_one_shot_entry_refuses_on_the_host(native):
    """The table, the rank and the threshold are checked before the handle is looked at: with a NULL handle a good
    call says so, and a bad one names its own fault."""
    lib = native.load()
    acc = (ctypes.c_int64 * 103)()
    dist = (ctypes.c_double * 3)(1.0, 2.0, 3.0)

    def call(table, k=3, rank=1, has_thr=0, thr=0.0, m=None):
        arr = None if table is None else (ctypes.c_double * max(len(table), 1))(*table)
        rc = lib.sknnr_domain_from_neighbors(None, dist, 1, k, rank, arr, len(table or ()) if m is None else m, has_thr, thr,
                                             None, acc, 0, native.MEM_HOST, None)
        return rc, lib.sknnr_last_error()

    rc, msg = call([0.0, 1.0, 1.0, 2.5])
    assert rc == native.ERR_INVALID and b"index is NULL" in msg
    for table, what in (([1.0, 0.5], b"not sorted"), ([1.0, float("nan")], b"finite"), ([-1.0, 1.0], b"finite"),
                        ([0.0, float("inf")], b"finite"), ([], b"m = 0"), (None, b"table is NULL")):
        rc, msg = call(table)
        assert rc == native.ERR_INVALID and what in msg, (table, msg)
    rc, msg = call([-0.0, 0.0, 1.0])  # (-0.0 is 0: accepted)
    assert b"index is NULL" in msg
    for rank in (0, 4, -1):
        rc, msg = call([1.0], rank=rank)
        assert rc == native.ERR_INVALID and b"rank" in msg, msg
    rc, msg = call([1.0], k=0)
    assert rc == native.ERR_INVALID and b"k must be" in msg
    rc, msg = call([1.0], m=2**31)
    assert rc == native.ERR_INVALID and b"outside [1, 2^31 - 1]" in msg
    for thr in (float("nan"), -1.0, float("inf")):
        rc, msg = call([1.0], has_thr=1, thr=thr)
        assert rc == native.ERR_INVALID and b"threshold" in msg
    rc, msg = call([1.0], has_thr=0, thr=float("nan"))  # (no threshold: the value is not read)
    assert b"index is NULL" in msg
