"""The expected value of every predict-reduction test: scikit-learn's own ``KNeighborsRegressor.predict`` run on
neighbours chosen elsewhere (by the GPU, or crafted by the test).  Its real ``_get_weights``, ``np.mean``, ``np.sum``
and dtype rules decide the answer.  Shared by test_predict_reduction_cpu.py and test_predict_reduction_gpu.py."""

from __future__ import annotations

import numpy as np


def sklearn_predict(y, dist, idx, weights="uniform"):
    """``KNeighborsRegressor(n_neighbors=k, algorithm="brute", weights=weights).fit(dummy, y).predict`` with its
    ``kneighbors`` answering ``(dist, idx)`` (numpy arrays, ``(nq, k)``)."""
    from sklearn.neighbors import KNeighborsRegressor

    dist = np.asarray(dist, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    y = np.asarray(y)
    reg = KNeighborsRegressor(n_neighbors=idx.shape[1], algorithm="brute", weights=weights)
    reg.fit(np.zeros((y.shape[0], 1)), y)

    def kneighbors(X=None, n_neighbors=None, return_distance=True):
        return (dist.copy(), idx.copy()) if return_distance else idx.copy()

    reg.kneighbors = kneighbors
    return KNeighborsRegressor.predict(reg, np.zeros((idx.shape[0], 1)))


def weights_f32(d):
    """A weights callable that returns float32: scikit-learn then sums the denominator in binary32."""
    return (1.0 / (1.0 + np.asarray(d))).astype(np.float32)


def targets(n, t, dtype, rng):
    """Targets of ``n`` rows: 1-D for ``t`` None, else ``(n, t)``; spread over several binades so that the order of
    the additions shows in the last bits (integers stay small: every sum of them is exact)."""
    shape = (n,) if t is None else (n, t)
    if np.dtype(dtype).kind == "i":
        return rng.integers(-1000, 1000, size=shape).astype(dtype)
    v = rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, size=shape))
    return v.astype(dtype)


def crafted_neighbours(n_ref, nq, k, rng):
    """``(dist, idx)`` ``(nq, k)``: ascending positive distances over several binades, repeated rows allowed, and rows
    with one exact zero (at the first, a middle and the last slot), several zeros, and only zeros."""
    idx = rng.integers(0, n_ref, size=(nq, k)).astype(np.int64)
    dist = np.sort(rng.uniform(0.05, 1.0, size=(nq, k)) * np.exp2(rng.integers(-4, 5, size=(nq, 1))), axis=1)
    if nq >= 6:
        dist[0, 0] = 0.0
        dist[1, k // 2] = 0.0
        dist[2, k - 1] = 0.0
        dist[3, : max(1, k // 3)] = 0.0
        dist[4, :] = 0.0
        dist[5, ::2] = 0.0
    return dist, idx
