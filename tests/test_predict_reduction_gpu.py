"""predict_kernel bit for bit against scikit-learn's own predict on the same neighbours (tests/_predict_ref.py).

Shapes where a reduction goes wrong: one target (numpy's pairwise mean) against several (the k slices in order), both
sides of k = 8 (the kernel's register branch) and of k = 128 (numpy's split), float32 targets and float32 weights (the
binary32 reductions), rows with zero distances.  Every assertion is exact and checks the dtype."""

from __future__ import annotations

import numpy as np
import pytest

from _predict_ref import crafted_neighbours, sklearn_predict, targets, weights_f32
from conftest import yaimpute_weights

pytestmark = pytest.mark.gpu

KS = [1, 7, 8, 9, 16, 17, 128, 129, 191]
WEIGHTS = ["uniform", "distance", yaimpute_weights, weights_f32]


@pytest.fixture(scope="module")
def N():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return _native


def assert_same(got, want, msg=""):
    """Exact equality, same dtype; ``got`` may be a torch tensor or carry a unit column where ``want`` is 1-D."""
    if hasattr(got, "cpu"):
        got = got.cpu().numpy()
    got = np.asarray(got)
    assert got.dtype == want.dtype, f"{msg}: dtype {got.dtype}, scikit-learn {want.dtype}"
    np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=msg)


def _problem(n_ref=2000, nq=1000, d=8):
    from sknnr_amd import synth

    x_ref, y, x_q = synth.make_problem(n_ref, nq, d, t=3)
    return x_ref, y[:, 0].copy(), x_q


# ---------------------------------------------------------------------------------------------
# the reduction alone (sknnr_predict_from_neighbors) on crafted neighbours
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int64])
@pytest.mark.parametrize("t", [None, 2, 9])
def test_reduction_alone_equals_scikit_learn(N, t, dtype):
    import torch

    from sknnr_amd._engine import KNNEngine

    rng = np.random.default_rng(5 + (t or 1) * 7 + np.dtype(dtype).itemsize)
    n_ref = 400
    y = targets(n_ref, t, dtype, rng)
    eng = KNNEngine(np.zeros((n_ref, 2)), y)
    try:
        for k in KS:
            dist, idx = crafted_neighbours(n_ref, 40, k, rng)
            for weights in WEIGHTS:
                want = sklearn_predict(y, dist, idx, weights)
                name = getattr(weights, "__name__", weights)
                assert_same(eng.predict_from_neighbors(dist, idx, weights), want, f"host k={k} {name}")
                if weights in ("uniform", "distance"):  # the callables here read numpy arrays
                    dd = torch.as_tensor(dist, device="cuda")
                    di = torch.as_tensor(idx, device="cuda")
                    got = eng.predict_from_neighbors(dd, di, weights)
                    assert got.is_cuda
                    assert_same(got, want, f"device k={k} {name}")
            # float32 weights straight from a torch callable on the device
            w_t = lambda d: (1.0 / (1.0 + d)).to(torch.float32)  # noqa: E731
            want = sklearn_predict(y, dist, idx, weights_f32)
            got = eng.predict_from_neighbors(torch.as_tensor(dist, device="cuda"), torch.as_tensor(idx, device="cuda"),
                                             w_t)
            assert_same(got, want, f"device k={k} float32 torch callable")
    finally:
        eng.close()


def test_reduction_rejects_k_above_the_search_limit(N):
    from sknnr_amd._engine import KNNEngine

    eng = KNNEngine(np.zeros((300, 2)), np.arange(300.0))
    try:
        dist, idx = crafted_neighbours(300, 4, 192, np.random.default_rng(0))
        assert eng.predict_from_neighbors(dist, idx, "distance").shape == (4, 1)
        dist, idx = crafted_neighbours(300, 4, 193, np.random.default_rng(0))
        with pytest.raises(N.HipBackendError, match="limit of 192"):
            eng.predict_from_neighbors(dist, idx, "distance")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# end to end: one target, k up to the cap
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    return _problem()


@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("cls_name", ["RawKNNRegressor", "EuclideanKNNRegressor"])
@pytest.mark.parametrize("k", [8, 9, 16, 64, 129, 191])
def test_one_target_end_to_end(N, problem, cls_name, k, weights):
    import torch
    from sklearn.metrics import r2_score

    import sknnr_amd

    x_ref, y, x_q = problem
    est = getattr(sknnr_amd, cls_name)(n_neighbors=k, weights=weights).fit(x_ref, y)

    dist, idx = est.kneighbors(x_q)
    want = sklearn_predict(y, dist, idx, weights)
    assert_same(est.predict(x_q), want, "predict(X)")
    got = est.predict(torch.as_tensor(x_q, device="cuda"))
    assert got.is_cuda
    assert_same(got, want, "predict(cuda X)")
    assert_same(est.predict_chunks([x_q[:300], x_q[300:650], x_q[650:]]), want, "predict_chunks")
    assert est.score(x_q, y[: len(x_q)]) == float(r2_score(y[: len(x_q)], want))

    sd, si = est.kneighbors()  # X=None: k + 1 searched, the row itself dropped (k = 191: the cap)
    want_self = sklearn_predict(y, sd, si, weights)
    assert_same(est.independent_prediction_, want_self, "independent_prediction_")
    assert_same(est.predict(None), want_self, "predict(None)")
    assert est.independent_score_ == float(r2_score(y, want_self))


@pytest.mark.parametrize("k", [64, 129, 191])
def test_many_neighbours_search_equals_the_oracle(N, problem, k):
    """Continuous, tie-free data: indices and distances at large k, with X and with X=None."""
    from oracle import oracle as O

    import sknnr_amd

    x_ref, y, x_q = problem
    est = sknnr_amd.RawKNNRegressor(n_neighbors=k).fit(x_ref, y)
    dist, idx = est.kneighbors(x_q)
    od, oi = O.kneighbors(x_ref, x_q, k, est._formula())
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(dist, od)
    dist, idx = est.kneighbors()
    od, oi = O.kneighbors(x_ref, None, k, est._formula())
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(dist, od)


# ---------------------------------------------------------------------------------------------
# float32 targets and float32 weights
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["uniform", "distance", weights_f32], ids=["uniform", "distance", "f32_callable"])
@pytest.mark.parametrize("t", [None, 3])
@pytest.mark.parametrize("k", [5, 9, 129])
def test_float32_targets(N, problem, weights, t, k):
    import torch

    import sknnr_amd

    x_ref, _, x_q = problem
    rng = np.random.default_rng(k * 10 + (t or 1))
    y = targets(len(x_ref), t, np.float32, rng)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights).fit(x_ref, y)
    dist, idx = est.kneighbors(x_q)
    want = sklearn_predict(y, dist, idx, weights)
    assert want.dtype == (np.float32 if weights == "uniform" else np.float64)
    assert_same(est.predict(x_q), want, "predict(X)")
    tiles = [x_q[:250], x_q[250:700], x_q[700:]]
    assert_same(est.predict_chunks(tiles), want, "predict_chunks")
    out = np.full((len(x_q),) + y.shape[1:], np.nan)
    est.predict_chunks(tiles, out=out)
    np.testing.assert_array_equal(out, want.astype(np.float64))  # the float32 values held exactly
    if not callable(weights):
        got = est.predict(torch.as_tensor(x_q, device="cuda"))
        assert got.is_cuda
        assert_same(got, want, "predict(cuda X)")
    sd, si = est.kneighbors()
    assert_same(est.independent_prediction_, sklearn_predict(y, sd, si, weights), "independent_prediction_")


def test_float32_weights_with_float64_targets(N, problem):
    import sknnr_amd

    x_ref, y, x_q = problem
    for k in (7, 9, 191):
        est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights_f32).fit(x_ref, y)
        dist, idx = est.kneighbors(x_q)
        assert_same(est.predict(x_q), sklearn_predict(y, dist, idx, weights_f32), f"k={k}")


# ---------------------------------------------------------------------------------------------
# a forest estimator
# ---------------------------------------------------------------------------------------------
def test_forest_estimator_one_target(N):
    import sknnr_amd

    rng = np.random.default_rng(21)
    X = rng.normal(size=(3000, 5))
    y = X @ np.array([1.0, -2.0, 0.5, 0.0, 3.0]) + rng.normal(size=len(X))
    Xq = rng.normal(size=(800, 5))
    est = sknnr_amd.RFNNRegressor(n_neighbors=9, n_estimators=20, random_state=0).fit(X, y)
    dist, idx = est.kneighbors(Xq)
    assert_same(est.predict(Xq), sklearn_predict(y, dist, idx, "uniform"), "RFNN predict(X)")
    sd, si = est.kneighbors()
    assert_same(est.independent_prediction_, sklearn_predict(y, sd, si, "uniform"), "RFNN independent_prediction_")


# ---------------------------------------------------------------------------------------------
# the k cap: the message names the limit the check applies
# ---------------------------------------------------------------------------------------------
def test_k_cap(N, problem):
    import sknnr_amd
    from sknnr_amd._engine import KNNEngine

    x_ref, y, x_q = problem
    eng = KNNEngine(x_ref, y)
    try:
        assert eng.kneighbors(x_q[:50], 192)[1].shape == (50, 192)
        with pytest.raises(N.HipBackendError, match=r"n_neighbors = 193 exceeds the HIP backend's limit of 192\b"):
            eng.kneighbors(x_q[:50], 193)
        assert eng.kneighbors(None, 191, exclude_self=True)[1].shape == (len(x_ref), 191)
        with pytest.raises(N.HipBackendError, match=r"n_neighbors = 192 exceeds the HIP backend's limit of 191\b"):
            eng.kneighbors(None, 192, exclude_self=True)
    finally:
        eng.close()

    est = sknnr_amd.RawKNNRegressor(n_neighbors=191).fit(x_ref, y)  # fit searches k + 1 for X=None
    assert est.kneighbors(x_q[:50], n_neighbors=192)[1].shape == (50, 192)
    with pytest.raises(Exception, match=r"limit of 192\b"):
        est.kneighbors(x_q[:50], n_neighbors=193)
    with pytest.raises(Exception, match=r"limit of 191\b"):
        sknnr_amd.RawKNNRegressor(n_neighbors=192).fit(x_ref, y)


def test_weight_mode_flags_are_validated(N):
    from sknnr_amd._engine import KNNEngine

    eng = KNNEngine(np.zeros((50, 2)), np.arange(50.0))
    try:
        dist, idx = crafted_neighbours(50, 6, 5, np.random.default_rng(1))
        w = 1.0 / (1.0 + dist)
        for bad in (3, N.WEIGHTS_UNIFORM | N.WEIGHTS_F32_WEIGHTS, N.WEIGHTS_DISTANCE | N.WEIGHTS_F32_WEIGHTS,
                    N.WEIGHTS_EXPLICIT | 0x400):
            with pytest.raises(N.HipBackendError, match="unknown weight mode"):
                eng._index.predict_from_neighbors_host(dist, idx, w, bad)
        opts = eng._index.make_opts(5, weight_mode=N.WEIGHTS_UNIFORM | N.WEIGHTS_F32_WEIGHTS)
        with pytest.raises(N.HipBackendError, match="unknown weight mode"):
            eng._index.predict_host(np.zeros((3, 2)), opts)
    finally:
        eng.close()
