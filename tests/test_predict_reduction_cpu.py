"""The summation order predict_kernel reproduces, pinned on numpy itself, and the oracle's predict pinned on
scikit-learn's (no GPU).

``predict_kernel`` (sknnr_amd/csrc/exact.hip.h) promises sums bit-identical to numpy's: its pairwise sum over k for
``np.sum(..., axis=1)`` of ``(nq, k)`` and for ``np.mean`` of ``(nq, k, 1)``, the k slices in order for ``np.mean`` of
``(nq, k, t >= 2)``, in binary32 for float32 operands.  If numpy ever changes its reduction order, the model below
stops matching here before any GPU test fails."""

from __future__ import annotations

import zlib

import numpy as np
import pytest

from _predict_ref import crafted_neighbours, sklearn_predict, targets, weights_f32
from conftest import yaimpute_weights


def pairwise_sum(v):
    """numpy's pairwise sum of the 1-D array ``v``, in ``v``'s dtype (numpy scalars round like its loops)."""
    n = len(v)
    if n < 8:
        r = v[0]
        for i in range(1, n):
            r = r + v[i]
        return r
    if n <= 128:
        r = list(v[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + v[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(i, n):
            res = res + v[i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(v[:n2]) + pairwise_sum(v[n2:])


def sequential_sum(rows):
    """The k slices of ``rows`` (k, t) added one after another."""
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = acc + r
    return acc


def model_mean(s, k, dtype):
    """``sum / k`` rounded once to ``dtype`` (binary32: the float32 quotient, as numpy divides float32 by k)."""
    return (s / dtype(k)).astype(dtype) if isinstance(s, np.ndarray) else dtype(s / dtype(k))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_numpy_sum_and_mean_follow_the_kernels_model(dtype):
    rng = np.random.default_rng(11)
    for k in range(1, 201):
        v = targets(24 * k, None, dtype, rng).reshape(24, k)
        want_sum = np.array([pairwise_sum(r) for r in v], dtype=dtype)
        want_mean = np.array([model_mean(s, k, dtype) for s in want_sum], dtype=dtype)
        np.testing.assert_array_equal(np.sum(v, axis=1), want_sum, err_msg=f"np.sum (nq, k) k={k}")
        np.testing.assert_array_equal(np.mean(v, axis=1), want_mean, err_msg=f"np.mean (nq, k) k={k}")
        m3 = np.mean(v[:, :, None], axis=1)
        assert m3.dtype == dtype
        np.testing.assert_array_equal(m3[:, 0], want_mean, err_msg=f"np.mean (nq, k, 1) k={k}")
        for t in (2, 3, 9):
            y3 = targets(6 * k * t, None, dtype, rng).reshape(6, k, t)
            want = np.stack([model_mean(sequential_sum(r), k, dtype) for r in y3])
            got = np.mean(y3, axis=1)
            assert got.dtype == dtype
            np.testing.assert_array_equal(got, want, err_msg=f"np.mean (nq, k, {t}) k={k}")


def test_the_two_orders_really_differ():
    """The pairwise and the sequential order differ at k >= 8 (1-D uniform), and the single split differs from one
    8-accumulator run above k = 128: the model's distinctions are visible in the last bits."""
    rng = np.random.default_rng(3)
    for k in (8, 16, 129, 191):
        v = targets(200 * k, None, np.float64, rng).reshape(200, k)
        seq = np.array([sequential_sum(r[:, None])[0] for r in v])
        assert np.any(np.sum(v, axis=1) != seq), k
    v = targets(200 * 191, None, np.float64, rng).reshape(200, 191)
    one_run = []
    for r in v:
        acc = list(r[:8])
        for i in range(8, 184, 8):
            for j in range(8):
                acc[j] = acc[j] + r[i + j]
        res = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
        for i in range(184, 191):
            res = res + r[i]
        one_run.append(res)
    assert np.any(np.sum(v, axis=1) != np.array(one_run))


KS = [1, 7, 8, 9, 16, 17, 128, 129, 191]
WEIGHTS = ["uniform", "distance", yaimpute_weights, weights_f32]


@pytest.mark.parametrize("weights", WEIGHTS, ids=["uniform", "distance", "yaimpute", "f32_callable"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int64])
@pytest.mark.parametrize("t", [None, 1, 3, 40])
def test_oracle_predict_equals_scikit_learn(weights, dtype, t):
    from oracle import oracle as O

    rng = np.random.default_rng(zlib.crc32(f"{np.dtype(dtype).name}/{t}".encode()))
    n_ref = 300
    y = targets(n_ref, t, dtype, rng)
    for k in KS:
        dist, idx = crafted_neighbours(n_ref, 12, k, rng)
        want = sklearn_predict(y, dist, idx, weights)
        got = O.predict(y, dist, idx, weights)
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, want.dtype)
        np.testing.assert_array_equal(got, want, err_msg=f"k={k}")


def test_reference_dtypes():
    """The dtype rules the device path follows: float32 targets keep float32 under uniform weights only."""
    rng = np.random.default_rng(0)
    dist, idx = crafted_neighbours(50, 8, 9, rng)
    for dtype, weights, want in [(np.float32, "uniform", np.float32), (np.float32, "distance", np.float64),
                                 (np.float32, weights_f32, np.float64), (np.float32, yaimpute_weights, np.float64),
                                 (np.int64, "uniform", np.float64), (np.float64, weights_f32, np.float64)]:
        assert sklearn_predict(targets(50, None, dtype, rng), dist, idx, weights).dtype == want, (dtype, weights)
