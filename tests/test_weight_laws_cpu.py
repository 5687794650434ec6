"""Distance-weight laws (sknnr_amd/weights.py), the part that needs no device: each law against its defining expression
written out here, what scikit-learn makes of a law, value semantics (pickle, clone, ==, repr), constructor refusals, the
header's enum against the binding, the pinned ABI facts the feature must not move, the refusals ``predict_chunks`` makes
before any device work, and the recorded values the stand-alone host check (scripts/weight_law_check.cpp) reads."""

from __future__ import annotations

import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from sknnr_amd import weights as W

TINY = np.nextafter(0.0, 1.0)  # the smallest subnormal


def expression(law, d):
    """The table of the module's docstring, written out: numpy float64, operation by operation."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(over="ignore"):
        if isinstance(law, W.InverseDistance):
            return 1.0 / (law.offset + d)
        if isinstance(law, W.InverseSquaredDistance):
            return 1.0 / (law.offset + d * d)
        if isinstance(law, W.Triangular):
            return np.maximum(0.0, 1.0 - d / law.bandwidth)
        u = d / law.bandwidth
        return np.maximum(0.0, 1.0 - u * u)


LAWS = [W.InverseDistance(), W.InverseDistance(0.25), W.InverseDistance(3.7), W.InverseSquaredDistance(),
        W.InverseSquaredDistance(0.5), W.InverseSquaredDistance(1e-3), W.Triangular(1.0), W.Triangular(2.5),
        W.Triangular(0.3), W.Epanechnikov(1.0), W.Epanechnikov(2.5), W.Epanechnikov(0.3)]


def crafted_distances(law):
    """0, subnormals, 1e-300, 1e308 (d * d overflows: the weight is 0), and the law's parameter with its two float64
    neighbours (the edge of a compact law's support)."""
    p = law.params[0]
    return np.array([0.0, TINY, 7 * TINY, 2.0**-1030, 1e-300, 1e308, p, np.nextafter(p, np.inf), np.nextafter(p, -np.inf),
                     0.1, 1.0 / 3.0, 1.0, 2.0, 1e155, 1.5e154])


@pytest.mark.parametrize("law", LAWS, ids=repr)
def test_call_is_the_table_expression(law):
    d = crafted_distances(law)
    got = law(d)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == d.shape
    np.testing.assert_array_equal(got, expression(law, d))
    assert np.isfinite(got).all() and (got >= 0).all()
    # d * d overflows at 1e308: the inverse-squared weight is exactly 0, the compact laws are 0 beyond the bandwidth
    if isinstance(law, W.InverseSquaredDistance):
        assert got[5] == 0.0
    if law.can_vanish:
        assert got[5] == 0.0 and got[6] == 0.0 and got[7] == 0.0 and got[8] > 0.0 and got[0] == 1.0
    rng = np.random.default_rng(3)
    for shape in ((0, 5), (7, 1), (3, 192)):
        d = rng.random(shape) * 4.0
        got = law(d)
        assert got.dtype == np.float64 and got.shape == shape
        np.testing.assert_array_equal(got, expression(law, d))
    # float32 distances are widened first; lists are taken as arrays
    d32 = (rng.random((4, 3)) * 2).astype(np.float32)
    np.testing.assert_array_equal(law(d32), expression(law, d32.astype(np.float64)))
    np.testing.assert_array_equal(law([0.0, 0.5]), expression(law, [0.0, 0.5]))


@pytest.mark.parametrize("law", LAWS[::3], ids=repr)
def test_torch_in_torch_out(law):
    import torch

    d = crafted_distances(law)
    got = law(torch.as_tensor(d))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == d.shape
    np.testing.assert_array_equal(got.numpy(), expression(law, d))
    got = law(torch.as_tensor(d[:5].astype(np.float32)).reshape(5, 1))
    assert got.dtype == torch.float64 and tuple(got.shape) == (5, 1)


@pytest.mark.parametrize("law", [W.InverseDistance(1.0), W.InverseSquaredDistance(0.5), W.Triangular(1.2), W.Epanechnikov(1.2)],
                         ids=repr)
def test_scikit_learn_takes_a_law_as_any_callable(law):
    from sklearn.neighbors import KNeighborsRegressor

    rng = np.random.default_rng(0)
    x, y = rng.random((200, 3)), rng.standard_normal((200, 2))
    q = rng.random((50, 3))
    reg = KNeighborsRegressor(n_neighbors=5, algorithm="brute", weights=law).fit(x, y)
    dist, idx = reg.kneighbors(q)
    w = expression(law, dist)
    with np.errstate(invalid="ignore"):
        want = np.stack([np.sum(y[idx, j] * w, axis=1) / np.sum(w, axis=1) for j in range(2)], axis=1)
        got = reg.predict(q)
    np.testing.assert_array_equal(got, want)
    same = KNeighborsRegressor(n_neighbors=5, algorithm="brute", weights=lambda d: expression(law, d)).fit(x, y)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got, same.predict(q))


def test_value_semantics():
    from sklearn.base import clone
    from sklearn.neighbors import KNeighborsRegressor

    import sknnr_amd

    for law in LAWS:
        for other in (pickle.loads(pickle.dumps(law)), clone(law), eval(repr(law), vars(W)),
                      clone(KNeighborsRegressor(weights=law)).weights,
                      clone(sknnr_amd.RawKNNRegressor(weights=law)).weights):
            assert other == law and type(other) is type(law) and hash(other) == hash(law)
            assert other.params == law.params and other.can_vanish == law.can_vanish
        assert law != "distance" and law is not None and callable(law) and isinstance(law, W.DistanceWeights)
    assert W.InverseDistance(1.0) != W.InverseDistance(2.0)
    assert W.InverseDistance(1.0) != W.InverseSquaredDistance(1.0)
    assert W.Triangular(1.0) != W.Epanechnikov(1.0)
    assert W.InverseDistance() == W.InverseDistance(1) == W.InverseDistance(offset=1.0)
    assert repr(W.Triangular(2)) == "Triangular(bandwidth=2.0)"
    assert W.InverseDistance(0.5).offset == 0.5 and W.Epanechnikov(3).bandwidth == 3.0
    assert sknnr_amd.weights is W and "weights" not in sknnr_amd.__all__


def test_can_vanish_is_read_only():
    assert not W.InverseDistance().can_vanish and not W.InverseSquaredDistance().can_vanish
    assert W.Triangular(1.0).can_vanish and W.Epanechnikov(1.0).can_vanish
    for law in (W.InverseDistance(), W.Triangular(1.0)):
        with pytest.raises(AttributeError):
            law.can_vanish = not law.can_vanish
        with pytest.raises(AttributeError):
            law.params = (2.0, 0.0)


@pytest.mark.parametrize("cls", [W.InverseDistance, W.InverseSquaredDistance, W.Triangular, W.Epanechnikov])
@pytest.mark.parametrize("bad", [0, 0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf"), "wide", None])
def test_constructors_refuse_bad_parameters(cls, bad):
    with pytest.raises(ValueError, match="must be"):
        cls(bad)


def test_bandwidth_is_required():
    with pytest.raises(TypeError):
        W.Triangular()
    with pytest.raises(TypeError):
        W.Epanechnikov()


# ---- the header, the binding and the pinned ABI facts -------------------------------------------------------------------
def test_law_codes_match_the_header():
    from sknnr_amd import _native

    header = open(os.path.join(ROOT, "include", "sknnr_hip.h")).read()
    body = re.search(r"enum sknnr_weight_law \{(.*?)\}", header, re.S).group(1)
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"SKNNR_LAW_(\w+) = (\d+)", body)}
    assert codes.pop("none") == 0 == _native.WEIGHT_LAW_NONE
    assert codes == _native.WEIGHT_LAWS == {"inverse": 1, "inverse_squared": 2, "triangular": 3, "epanechnikov": 4}
    for cls in (W.InverseDistance, W.InverseSquaredDistance, W.Triangular, W.Epanechnikov):
        assert _native.WEIGHT_LAWS[cls.name] == cls.code
    # the kernel header's constants are the same numbers
    khead = open(os.path.join(ROOT, "sknnr_amd", "csrc", "weights.hip.h")).read()
    line = re.search(r"constexpr int kLawNone = (\d+), kLawInverse = (\d+), kLawInverseSquared = (\d+), "
                     r"kLawTriangular = (\d+), kLawEpanechnikov = (\d+);", khead)
    assert [int(g) for g in line.groups()] == [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def native():
    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_abi_facts_stay(native):
    lib = native.load()
    assert lib.sknnr_abi_version() == native.ABI_VERSION == 5
    assert ctypes.sizeof(native.QueryOpts) == 48
    assert native.QueryOpts.weight_law.offset == 36 and native.QueryOpts.row_offset.offset == 40
    opts = native.Index.make_opts(5)
    assert opts.weight_law == 0, "no law unless asked for: the field is what reserved_ was"
    assert native.Index.make_opts(5, weight_mode=native.WEIGHTS_EXPLICIT, weight_law=3).weight_law == 3
    assert (native.WEIGHTS_UNIFORM, native.WEIGHTS_DISTANCE, native.WEIGHTS_EXPLICIT) == (0, 1, 2)
    assert native.STATISTICS == {"mean": 0, "mode": 1, "min": 2, "max": 3, "nearest": 4, "std": 5}


def test_argument_errors_without_touching_a_device(native):
    lib = native.load()
    INV = native.ERR_INVALID
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sknnr_index_set_weight_law_params(None, 1, 1.0, 0.0) == INV and b"index is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_debug_last_weight_law(None, (ctypes.c_int64 * 8)()) == INV
    for law in (0, 5, -1):
        assert lib.sknnr_debug_weight_law(law, 1.0, 0.0, p, 8, p, 0, 0) == INV
        assert b"unknown weight law" in lib.sknnr_last_error()
    assert lib.sknnr_debug_weight_law(1, 1.0, 0.0, p, -1, p, 0, 0) == INV
    assert lib.sknnr_debug_weight_law(1, 1.0, 0.0, p, 8, p, 7, 0) == INV and b"memspace" in lib.sknnr_last_error()
    assert lib.sknnr_debug_weight_law(1, 1.0, 0.0, None, 0, None, 0, 0) == 0, "n == 0 is SKNNR_OK"


# ---- predict_chunks: refusals before any device work ----------------------------------------------------------------------
class _NoDevice:
    """Stands where the device engine would: any use beyond the target count is a failure of the test."""

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        raise AssertionError(f"the device engine was touched ({name}) before the arguments were refused")


def fitted(weights):
    """A RawKNNRegressor in the state ``fit`` leaves it in, minus the device handle."""
    import sknnr_amd

    est = sknnr_amd.RawKNNRegressor(n_neighbors=3, weights=weights)
    rng = np.random.default_rng(0)
    est._fit_X = rng.standard_normal((20, 6))
    est._y = rng.standard_normal((20, 3))
    est.n_features_in_ = 6
    est.n_samples_fit_ = 20
    est.effective_metric_ = "euclidean"
    est.effective_metric_params_ = {}
    est._fit_method = "brute"
    est._affine = est._forest = est._ref_tree = None
    est._engine = _NoDevice(3)
    return est


TILES = [np.zeros((4, 6))]


@pytest.mark.parametrize("law", [W.Triangular(1.0), W.Epanechnikov(2.0)], ids=repr)
@pytest.mark.parametrize("dtype", [np.int16, np.uint16, np.uint8, np.int32])
def test_compact_law_needs_out_nodata_for_integer_outputs(law, dtype):
    with pytest.raises(ValueError, match="out_nodata is required"):
        fitted(law).predict_chunks(TILES, out_dtype=dtype)
    with pytest.raises(ValueError, match="out_nodata is required"):
        fitted(law).predict_chunks(TILES, out_dtype=dtype, return_neighbors=True)


def test_other_laws_and_float32_do_not_need_out_nodata():
    """The refusal is for a law that can vanish and an integer type only: these calls pass the argument checks and reach
    the engine (which the stand-in reports)."""
    for weights, dtype in ((W.InverseDistance(), np.int16), (W.InverseSquaredDistance(2.0), np.uint8),
                           (W.Triangular(1.0), np.float32), ("distance", np.int16)):
        with pytest.raises(AssertionError, match="the device engine was touched"):
            fitted(weights).predict_chunks(TILES, out_dtype=dtype)


def test_a_plain_callable_keeps_every_refusal():
    est = fitted(lambda d: 1.0 / (1.0 + d))
    bands = [np.zeros((6, 4))]
    for kwargs, tiles, msg in ((dict(nodata=-1.0), TILES, "nodata is not supported with callable weights"),
                               (dict(layout="bands"), bands, "layout='bands' is not supported with callable weights"),
                               (dict(out_dtype=np.int16, scale=100.0, out_nodata=-32768), TILES,
                                "typed outputs are not supported with callable weights"),
                               (dict(out_dtype=np.float32), TILES, "typed outputs are not supported with callable weights"),
                               (dict(return_neighbors=True), TILES, "return_neighbors is not supported with callable weights"),
                               (dict(return_neighbors=True, return_dataframe_index=True, index_dtype=np.int32), TILES,
                                "return_neighbors is not supported with callable weights")):
        with pytest.raises(NotImplementedError, match=msg):
            est.predict_chunks(tiles, **kwargs)
    # a callable that wraps a law is a plain callable
    law = W.InverseDistance()
    with pytest.raises(NotImplementedError, match="nodata is not supported with callable weights"):
        fitted(lambda d: law(d)).predict_chunks(TILES, nodata=-1.0)


def test_engine_keeps_its_refusals_for_plain_callables():
    from sknnr_amd._engine import KNNEngine

    eng = KNNEngine.__new__(KNNEngine)  # (no handle: both refusals come before the engine looks at it)
    eng.t = 3
    eng._law_key = None
    with pytest.raises(NotImplementedError, match="nodata is not supported with callable weights"):
        eng.predict(np.zeros((2, 6)), 3, lambda d: d, nodata=np.zeros(6))
    with pytest.raises(ValueError, match="a stream predicts with"):
        eng.open_stream(3, weights=lambda d: d)
    assert eng.weight_law("distance") == 0 and eng.weight_law(lambda d: d) == 0 and eng.weight_law(None) == 0


# ---- the recorded values of the stand-alone host check ---------------------------------------------------------------------
def read_fixture():
    rows = []
    for line in open(os.path.join(GOLDEN, "weight_laws.txt")):
        if line.startswith("#") or not line.strip():
            continue
        law, p0, d, w = line.split()
        rows.append((int(law), *(np.array([int(v, 16)], dtype=np.uint64).view(np.float64)[0] for v in (p0, d, w))))
    return rows


def test_recorded_values_are_numpy_s():
    """tests/golden/weight_laws.txt (law code, then p0, d and w as float64 bit patterns) holds what the laws give here: the
    stand-alone C++ program compares the kernel header's host-callable law with these, under the sanitizers."""
    by_code = {cls.code: cls for cls in (W.InverseDistance, W.InverseSquaredDistance, W.Triangular, W.Epanechnikov)}
    rows = read_fixture()
    assert len(rows) >= 4 * 3 * 15 and {r[0] for r in rows} == set(by_code)
    for code, p0, d, w in rows:
        got = by_code[code](p0)(np.array([d]))[0]
        assert got.tobytes() == np.float64(w).tobytes(), (code, p0, d, w, got)
