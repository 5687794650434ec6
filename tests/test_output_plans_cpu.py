"""Output plans without a device: the numpy restatement of the weighted quantile (tests/_output_plans.py) against numpy's
own ``np.quantile(..., method="inverted_cdf", weights=)``, ``normalize_outputs`` / ``resolve_statistic`` with every refusal,
the refusals of the four new C entries that come before any device work, and the exports.

Without the feature these tests fail with ``ImportError`` (no ``normalize_outputs``) or ``AttributeError`` (no
``sknnr_summarize_plan`` in the library); the restatement-vs-numpy test alone touches nothing the feature adds."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import _output_plans as OP

ROOT = os.path.join(os.path.dirname(__file__), "..")
KS = (1, 2, 5, 8, 9, 17, 40, 192)
QS = (0.0, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0)
ROWS = 400  # per (k, kind, q): 8 * 4 * 8 * 400 = 102,400 rows


def grid_inputs(k, kind, rng):
    """Values and weights of one kind: uniform weights, continuous inverse weights, 0 / 1 masks whose zeros lead in sorted
    order, lattice values with many equal ones."""
    v = rng.standard_normal((ROWS, k))
    if kind == "uniform":
        w = np.ones((ROWS, k))
    elif kind == "inverse":
        w = 1.0 / rng.uniform(0.1, 7.0, size=(ROWS, k))
    elif kind == "mask":
        w = (rng.integers(0, 3, size=(ROWS, k)) == 0).astype(np.float64)
        low = np.argsort(v, axis=1)[:, : max(1, k // 3)]
        np.put_along_axis(w, low, 0.0, axis=1)  # leading zeros in sorted order
    else:
        v = rng.integers(-2, 3, size=(ROWS, k)).astype(np.float64)
        v[v == 0.0] = np.where(rng.integers(0, 2, size=int((v == 0.0).sum())) == 0, 0.0, -0.0)
        w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 1 / 3, 0.1]), size=(ROWS, k))
    return v, w


@pytest.mark.parametrize("kind", ["uniform", "inverse", "mask", "lattice"])
@pytest.mark.parametrize("k", KS)
def test_the_restatement_is_numpy_s_inverted_cdf(k, kind):
    if int(np.__version__.split(".")[0]) < 2:
        pytest.skip("np.quantile takes weights from numpy 2.0 on")
    rng = np.random.default_rng(100 * k + len(kind))
    v, w = grid_inputs(k, kind, rng)
    live = w.sum(axis=1) > 0  # (numpy returns garbage, not NaN, where the weights sum to 0)
    for q in QS:
        got = OP.weighted_quantile(v, w, q)
        want = np.array([np.quantile(v[r], q, method="inverted_cdf", weights=w[r]) for r in np.flatnonzero(live)])
        np.testing.assert_array_equal(got[live], want, err_msg=f"k={k} {kind} q={q}")
        assert np.isnan(got[~live]).all()


def test_the_restatement_gives_nan_without_weight_and_keeps_neighbour_order():
    v = np.array([[3.0, 1.0, 2.0], [0.0, -0.0, 0.0]])
    assert np.isnan(OP.weighted_quantile(v, np.zeros((2, 3)), 0.5)).all()
    # -0.0 == 0.0: the stable order is the neighbour order, so q = 0 gives the first neighbour's +0.0 and the leading
    # zero weight skips to the second one's -0.0
    got = OP.weighted_quantile(v[1:], np.ones((1, 3)), 0.0)
    assert got[0] == 0.0 and not np.signbit(got[0])
    got = OP.weighted_quantile(v[1:], np.array([[0.0, 1.0, 1.0]]), 0.0)
    assert got[0] == 0.0 and np.signbit(got[0])
    # no cdf reaches q (cannot happen for q <= 1 with a positive total, but the rule is k - 1): q above 1
    assert OP.weighted_quantile(v[:1], np.ones((1, 3)), 1.5)[0] == 3.0


# ---- normalize_outputs / resolve_statistic ---------------------------------------------------------------------------------
def test_normalize_outputs_accepts():
    from sknnr_amd._base import normalize_outputs

    cols, codes, params = normalize_outputs([(2, "mean"), (0, "std"), (2, ("quantile", 0.1)), (2, "median"), (1, "mode"),
                                             (0, ["quantile", 1]), (0, "nearest"), (1, "min"), (1, "max")], 3)
    assert cols.dtype == np.int32 and codes.dtype == np.int32 and params.dtype == np.float64
    assert cols.tolist() == [2, 0, 2, 2, 1, 0, 0, 1, 1]
    assert codes.tolist() == [0, 5, 6, 6, 1, 6, 4, 2, 3]
    assert params.tolist() == [0, 0, 0.1, 0.5, 0, 1.0, 0, 0, 0]
    cols, codes, params = normalize_outputs(((np.int64(0), "mean"),) * 1024, 1)
    assert cols.size == 1024
    want = OP.arrays([(2, "mean"), (0, ("quantile", 0.25)), (1, "median")])
    got = normalize_outputs([(2, "mean"), (0, ("quantile", 0.25)), (1, "median")], 3)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("outputs, msg", [
    ([(3, "mean")], r"outputs\[0\]: target 3 is outside \[0, 3\)"),
    ([(0, "mean"), (-1, "std")], r"outputs\[1\]: target -1 is outside"),
    ([(0.0, "mean")], "must be an integer column position"),
    ([(True, "mean")], "must be an integer column position"),
    ([("a", "mean")], "must be an integer column position"),
    ([(0, "average")], r"outputs\[0\]: unknown statistic 'average'"),
    ([(0, "quantile")], "unknown statistic 'quantile'"),
    ([(0, ("quantile",))], "unknown statistic"),
    ([(0, ("quantile", "0.5"))], "unknown statistic"),
    ([(0, ("quantile", 1.5))], r"q must lie in \[0, 1\]"),
    ([(0, ("quantile", -0.1))], r"q must lie in \[0, 1\]"),
    ([(0, ("quantile", float("nan")))], r"q must lie in \[0, 1\]"),
    ([(0, ("quantile", float("inf")))], r"q must lie in \[0, 1\]"),
    ([], "at least one"),
    ([(0, "mean")] * 1025, "at most 1024"),
    ("mean", "sequence of"),
    (5, "sequence of"),
    ([0, "mean"], r"outputs\[0\] must be a \(target, statistic\) pair"),
    ([(0, "mean", 1)], "must be a"),
])
def test_normalize_outputs_refuses(outputs, msg):
    from sknnr_amd._base import normalize_outputs

    with pytest.raises(ValueError, match=msg):
        normalize_outputs(outputs, 3)


def test_resolve_statistic():
    from sknnr_amd._base import OutputPlan, normalize_statistic, resolve_statistic

    assert resolve_statistic(None, None, 3) is None
    # the six old names: the per-target codes, exactly normalize_statistic's
    for s in ("std", ["mean", "mode", "max"]):
        got = resolve_statistic(s, None, 3)
        assert not isinstance(got, OutputPlan)
        np.testing.assert_array_equal(got, normalize_statistic(s, 3))
    got = resolve_statistic(["mean", ("quantile", 0.9), "mode"], None, 3)
    assert isinstance(got, OutputPlan) and got.per_target and got.n_out == 3
    assert got.cols.tolist() == [0, 1, 2] and got.codes.tolist() == [0, 6, 1] and got.params.tolist() == [0, 0.9, 0]
    got = resolve_statistic(("quantile", 0.5), None, 2)
    assert got.per_target and got.codes.tolist() == [6, 6] and got.params.tolist() == [0.5, 0.5]
    # in ``statistic`` the median is spelled ("quantile", 0.5): the bare name stays the unknown statistic it was
    for s in ("median", ["mean", "median"], [("quantile", 0.5), "median"]):
        with pytest.raises(ValueError, match="unknown statistic 'median'"):
            resolve_statistic(s, None, 2)
    got = resolve_statistic(None, [(1, "median")], 2)
    assert isinstance(got, OutputPlan) and not got.per_target and got.cols.tolist() == [1]
    with pytest.raises(ValueError, match="outputs and statistic cannot be given together"):
        resolve_statistic("mean", [(0, "mean")], 2)
    with pytest.raises(ValueError, match="one name per target"):
        resolve_statistic([("quantile", 0.5)], None, 2)
    with pytest.raises(ValueError, match=r"statistic\[1\]: a quantile's q must lie"):
        resolve_statistic(["mean", ("quantile", 2)], None, 2)
    with pytest.raises(ValueError, match=r"statistic\[0\]: unknown statistic"):
        resolve_statistic(["avg", ("quantile", 0.5)], None, 2)
    # the old refusals keep their words
    with pytest.raises(ValueError, match="must be strings"):
        resolve_statistic(["mean", 1], None, 2)
    with pytest.raises(ValueError, match="unknown statistic 'avg'"):
        resolve_statistic("avg", None, 2)


class _NoDevice:
    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        raise AssertionError(f"the device engine was touched ({name}) before the arguments were refused")


def test_estimators_refuse_before_any_device_work():
    import sknnr_amd

    est = sknnr_amd.RawKNNRegressor(n_neighbors=3)
    rng = np.random.default_rng(0)
    est._fit_X = rng.standard_normal((20, 6))
    est._y = rng.standard_normal((20, 3))
    est.n_features_in_ = 6
    est.n_samples_fit_ = 20
    est._engine = _NoDevice(3)
    X = np.zeros((4, 6))
    for call in (lambda **kw: est.summarize(X, **kw), lambda **kw: est.predict_chunks([X], **kw)):
        with pytest.raises(ValueError, match="cannot be given together"):
            call(outputs=[(0, "mean")], statistic="mean")
        with pytest.raises(ValueError, match="outside"):
            call(outputs=[(3, "mean")])
        with pytest.raises(ValueError, match="q must lie"):
            call(outputs=[(0, ("quantile", 1.01))])
        with pytest.raises(ValueError, match="q must lie"):
            call(statistic=["mean", "mean", ("quantile", -1)])
    # scale / offset: scalars or one per OUTPUT PLANE
    with pytest.raises(ValueError, match=r"one value per target \(4\), got 3"):
        est.predict_chunks([X], outputs=[(0, "mean")] * 4, out_dtype=np.int16, scale=[1.0, 2.0, 3.0], out_nodata=-1)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("sknnr_summarize_plan_from_neighbors", "sknnr_summarize_plan", "sknnr_stream_set_plan", "sknnr_debug_last_plan")


@pytest.fixture(scope="module")
def native():
    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_exports_and_header(native):
    lib = native.load()
    header = open(os.path.join(ROOT, "include", "sknnr_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert lib.sknnr_abi_version() == native.ABI_VERSION == 5
    assert re.search(r"SKNNR_STAT_QUANTILE = (\d+)", header).group(1) == "6"
    assert native.PLAN_STATISTICS == {**native.STATISTICS, "quantile": 6} == OP.CODES
    assert native.PLAN_MAX_OUT == 1024
    khead = open(os.path.join(ROOT, "sknnr_amd", "csrc", "plan.hip.h")).read()
    assert re.search(r"constexpr int kStatQuantile = 6;", khead) and re.search(r"constexpr int kPlanMaxOut = 1024;", khead)


def test_argument_errors_without_touching_a_device(native):
    lib = native.load()
    INV = native.ERR_INVALID
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cols, stat, param = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 2)(0, 6), (ctypes.c_double * 2)(0.0, 0.5)
    assert lib.sknnr_summarize_plan_from_neighbors(None, p, p, None, 4, 3, 0, cols, stat, param, 2, p, 0, None) == INV
    assert b"index is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_summarize_plan(None, p, 4, None, cols, stat, param, 2, p, None, None, 0, None) == INV
    assert b"index is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_stream_set_plan(None, cols, stat, param, 2) == INV and b"stream is NULL" in lib.sknnr_last_error()
    assert lib.sknnr_debug_last_plan(None, (ctypes.c_int64 * 8)()) == INV
