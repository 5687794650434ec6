"""The bootstrap without a device: the numpy restatement (tests/_bootstrap.py) against scikit-learn fitted on the actually
resampled rows, the host logic of ``sknnr_amd.Bootstrap``, and every estimator-level refusal that needs no device.

The oracle: for every replicate ``b`` a ``KNeighborsRegressor(algorithm="brute")`` fitted on ``np.repeat`` of the rows by
``M[b]`` -- what "bootstrap the plots, refit, predict" means -- on continuous random data without ties.  Bounds: a valid
``p_b`` within rtol 1e-12 (the forward bound of a <= 192-term float64 weighted mean is about 2e-14: a 50x margin); the mean
and the standard error over replicates against ``np.mean`` / ``np.std(ddof=1)`` within rtol 1e-10, for inputs whose
``se / |mean| >= 1e-3`` (asserted: the cancellation in ``S2 - S1 * S1 / m`` loses about ``(mean / se)^2`` of 1e-16).

Without the feature this file fails on the missing class ``sknnr_amd.Bootstrap``."""

from __future__ import annotations

import pickle

import numpy as np
import pytest

import _bootstrap as BS

N, D, NQ, B, K = 60, 4, 65, 37, 5


def problem():
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((N, D))
    y = rng.uniform(1.0, 10.0, size=(N, 2))
    Xq = rng.standard_normal((NQ, D))
    M = BS.draw_table(B, N, seed=5)
    return X, y, Xq, M


def neighbour_lists(X, Xq, kw):
    from sklearn.neighbors import NearestNeighbors

    return NearestNeighbors(n_neighbors=kw, algorithm="brute").fit(X).kneighbors(Xq)


_ORACLE = {}


def oracle(weights):
    """``(B, NQ, 2)``: scikit-learn fitted on the resampled rows, one replicate after the other; computed once."""
    if weights not in _ORACLE:
        from sklearn.neighbors import KNeighborsRegressor

        X, y, Xq, M = problem()
        out = np.empty((B, NQ, 2))
        for b in range(B):
            rows = np.repeat(np.arange(N), M[b])
            out[b] = KNeighborsRegressor(n_neighbors=K, weights=weights, algorithm="brute").fit(X[rows], y[rows]).predict(Xq)
        _ORACLE[weights] = out
    return _ORACLE[weights]


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_restatement_against_scikit_learn_on_the_resampled_rows(weights):
    X, y, Xq, M = problem()
    dist, idx = neighbour_lists(X, Xq, N)
    r = BS.replicates(y, dist, idx, M, K, weights, [0, 1])
    assert not r["short"].any() and r["valid"].all()  # (kw = n: every replicate finds its k copies)
    want = oracle(weights).transpose(1, 0, 2)
    rel = np.abs(r["p"] - want) / np.abs(want)
    print(f"{weights}: replicate values, max relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-12
    plan = [(0, "boot_mean"), (0, "boot_se"), (1, "boot_mean"), (1, "boot_se"), "boot_count"]
    out, tally = BS.bootstrap_of(y, dist, idx, M, K, weights, plan)
    mean, se = want.mean(axis=1), want.std(axis=1, ddof=1)
    assert (se / np.abs(mean)).min() >= 1e-3
    for j in range(2):
        print(f"{weights}: target {j} mean {np.abs(out[:, 2 * j] / mean[:, j] - 1).max():.3g} "
              f"se {np.abs(out[:, 2 * j + 1] / se[:, j] - 1).max():.3g}")
        np.testing.assert_allclose(out[:, 2 * j], mean[:, j], rtol=1e-10)
        np.testing.assert_allclose(out[:, 2 * j + 1], se[:, j], rtol=1e-10)
    np.testing.assert_array_equal(out[:, 4], B)
    np.testing.assert_array_equal(tally, [NQ, NQ * B])


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_short_pairs_are_those_with_fewer_than_k_copies_in_the_list(weights):
    X, y, Xq, M = problem()
    kw = 8
    dist, idx = neighbour_lists(X, Xq, kw)
    r = BS.replicates(y, dist, idx, M, K, weights, [0, 1])
    in_list = M[:, idx].sum(axis=2).T  # (NQ, B) copies inside the list
    np.testing.assert_array_equal(r["short"], in_list < K)
    assert r["short"].any() and ((r["c"] > 0) & (r["c"] < r["mult"])).any()
    # the pairs that are not short agree with the oracle: the k nearest copies all lie inside the list
    want = oracle(weights).transpose(1, 0, 2)
    ok = ~r["short"]
    np.testing.assert_allclose(r["p"][ok], want[ok], rtol=1e-12)
    out, tally = BS.bootstrap_of(y, dist, idx, M, K, weights, ["boot_count", (1, "boot_se")])
    np.testing.assert_array_equal(out[:, 0], ok.sum(axis=1))
    np.testing.assert_array_equal(tally, [NQ, ok.sum()])


def test_the_fold_is_the_wave_order():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((3, 200, 2))
    P = [[sum(a[q, l::64, c].tolist(), 0.0) for l in range(64)] for q in range(3) for c in range(2)]  # noqa: E741
    want = []
    for p in P:
        p = list(p)
        s = 32
        while s:
            p = [p[l] + p[l + s] for l in range(s)]  # noqa: E741
            s //= 2
        want.append(p[0])
    np.testing.assert_array_equal(BS.fold64(a).reshape(-1), want)
    # a segment of 32 or 16 lanes gives the same bits when B fits in it
    small = rng.standard_normal((5, 16, 1))
    p16 = small[:, :, 0].copy()
    s = 8
    while s:
        p16 = p16[:, :s] + p16[:, s:2 * s]
        s //= 2
    np.testing.assert_array_equal(BS.fold64(small)[:, 0], p16[:, 0])


# ---- the class ------------------------------------------------------------------------------------------------------------------
def test_the_table_is_drawn_on_binding_and_by_seed():
    import sknnr_amd

    bs = sknnr_amd.Bootstrap(7, seed=3)
    with pytest.raises(ValueError, match="not been used yet"):
        bs.multiplicity
    assert bs.n is None
    table = bs._bind(50)
    assert table.dtype == np.uint8 and table.shape == (7, 50) and bs.n == 50
    np.testing.assert_array_equal(table, BS.draw_table(7, 50, seed=3))
    rng = np.random.default_rng(3)
    np.testing.assert_array_equal(table[0], np.bincount(rng.integers(0, 50, size=50), minlength=50))
    np.testing.assert_array_equal(table.sum(axis=1), 50)
    assert bs._bind(50) is table
    np.testing.assert_array_equal(sknnr_amd.Bootstrap(7, seed=3)._bind(50), table)
    assert not np.array_equal(sknnr_amd.Bootstrap(7, seed=4)._bind(50), table)
    with pytest.raises(ValueError, match="bound to n = 50"):
        bs._bind(51)


def test_groups_share_counts():
    import sknnr_amd

    groups = np.array(["c", "a", "b", "a", "c", "c", "b", "d"])
    bs = sknnr_amd.Bootstrap(9, seed=1, groups=groups)
    table = bs._bind(8)
    np.testing.assert_array_equal(table, BS.draw_table(9, 8, seed=1, groups=groups))
    for g in "abcd":
        cols = table[:, groups == g]
        assert (cols == cols[:, :1]).all()
    first = np.array([np.flatnonzero(groups == g)[0] for g in "abcd"])
    np.testing.assert_array_equal(table[:, first].sum(axis=1), 4)  # (each replicate draws G groups)
    with pytest.raises(ValueError, match="one label per fitted row"):
        sknnr_amd.Bootstrap(2, groups=groups)._bind(9)
    with pytest.raises(ValueError, match="at least two groups"):
        sknnr_amd.Bootstrap(2, groups=np.zeros(8))._bind(8)


def test_a_given_table_is_taken_as_it_is_and_clamped():
    import sknnr_amd

    jack = 1 - np.eye(6, dtype=np.int64)  # a delete-one jackknife
    bs = sknnr_amd.Bootstrap(multiplicity=jack)
    assert bs.n_replicates == 6 and bs.n == 6
    np.testing.assert_array_equal(bs.multiplicity, jack)
    np.testing.assert_array_equal(bs._bind(6), jack)
    big = sknnr_amd.Bootstrap(multiplicity=np.array([[0, 255, 256, 100000]]))
    np.testing.assert_array_equal(big.multiplicity, [[0, 255, 255, 255]])
    with pytest.raises(ValueError, match="bound to n = 6"):
        bs._bind(7)
    # the table is read-only, drawn or given: the device reduces from a copy of it
    for table in (bs.multiplicity, sknnr_amd.Bootstrap(3)._bind(5)):
        with pytest.raises(ValueError, match="read-only"):
            table[0, 0] = 9
    jack[0, 0] = 7  # (the caller's own array stays the caller's)
    assert bs.multiplicity[0, 0] == 0


def test_constructor_refusals():
    import sknnr_amd

    B_ = sknnr_amd.Bootstrap
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="n_replicates must lie in"):
            B_(bad)
    for bad in (2.5, True, "3"):
        with pytest.raises((TypeError, ValueError)):
            B_(bad)
    with pytest.raises(TypeError, match="needs n_replicates"):
        B_()
    for bad in (0, 193):
        with pytest.raises(ValueError, match="n_candidates must lie in"):
            B_(5, n_candidates=bad)
    with pytest.raises(TypeError, match="n_candidates must be an integer"):
        B_(5, n_candidates=8.0)
    with pytest.raises(ValueError, match="must be a .B, n. table"):
        B_(multiplicity=np.ones(4, dtype=int))
    with pytest.raises(TypeError, match="must hold integers"):
        B_(multiplicity=np.ones((2, 4)))
    with pytest.raises(ValueError, match="must not be negative"):
        B_(multiplicity=np.array([[1, -1]]))
    with pytest.raises(ValueError, match="n_replicates = 3, but multiplicity has 2 rows"):
        B_(3, multiplicity=np.ones((2, 4), dtype=int))
    with pytest.raises(ValueError, match="a ready multiplicity takes none"):
        B_(multiplicity=np.ones((2, 4), dtype=int), groups=np.arange(4))
    with pytest.raises(ValueError, match="n_replicates must lie in"):
        B_(multiplicity=np.ones((4097, 2), dtype=np.uint8))


def test_candidates():
    import sknnr_amd

    bs = sknnr_amd.Bootstrap(5)
    assert bs.candidates(5, 1000) == 28 and bs.candidates(5, 20) == 20 and bs.candidates(60, 1000) == 192
    with pytest.raises(ValueError, match="exceeds n_candidates = 4"):
        sknnr_amd.Bootstrap(5, n_candidates=4).candidates(5, 100)
    with pytest.raises(ValueError, match="exceeds the 19 rows"):
        sknnr_amd.Bootstrap(5, n_candidates=20).candidates(5, 19)
    assert sknnr_amd.Bootstrap(5, n_candidates=20).candidates(5, 20) == 20


def test_value_semantics():
    import sknnr_amd

    a, b = sknnr_amd.Bootstrap(5, seed=2, n_candidates=12), sknnr_amd.Bootstrap(5, seed=2, n_candidates=12)
    assert a == b and a != sknnr_amd.Bootstrap(5, seed=3, n_candidates=12) and a != sknnr_amd.Bootstrap(6, seed=2, n_candidates=12)
    assert (a == 3) is False
    with pytest.raises(TypeError):
        hash(a)
    a._bind(30)
    assert a != b  # (one has its table, the other not yet)
    b._bind(30)
    assert a == b
    a._add((10, 45))
    assert a != b and a.pixels == 10 and a.replicates_used == 45 and a.share_short == pytest.approx(1 - 45 / 50)
    assert np.isnan(b.share_short)
    c = pickle.loads(pickle.dumps(a))
    assert c == a and c.pixels == 10 and c.n == 30 and not c.multiplicity.flags.writeable
    b._add((4, 20))
    b += a
    assert b.pixels == 14 and b.replicates_used == 65
    with pytest.raises(ValueError, match="only the tallies of the same bootstrap"):
        b += sknnr_amd.Bootstrap(5, seed=9, n_candidates=12)
    with pytest.raises(TypeError):
        b += 3
    g = sknnr_amd.Bootstrap(multiplicity=np.ones((2, 3), dtype=int))
    assert g == pickle.loads(pickle.dumps(g)) and g != sknnr_amd.Bootstrap(multiplicity=np.zeros((2, 3), dtype=int))
    assert "Bootstrap(" in repr(g)


def test_outputs_of_a_bootstrap_call():
    from sknnr_amd._bootstrap import normalize_boot_outputs

    cols, codes = normalize_boot_outputs(None, 3)
    np.testing.assert_array_equal(cols, [0, 1, 2])
    np.testing.assert_array_equal(codes, [0, 0, 0])
    cols, codes = normalize_boot_outputs([(2, "boot_mean"), "boot_count", (0, "boot_bias"), (2, "boot_se")], 3)
    np.testing.assert_array_equal(cols, [2, 0, 0, 2])
    np.testing.assert_array_equal(codes, [1, 3, 2, 0])
    np.testing.assert_array_equal(normalize_boot_outputs("boot_count", 1)[1], [3])
    for name in ("mean", "mode", "min", "max", "nearest", "std"):
        with pytest.raises(ValueError, match="not available with bootstrap="):
            normalize_boot_outputs([(0, name)], 3)
    with pytest.raises(ValueError, match="not available with bootstrap="):
        normalize_boot_outputs([(0, ("quantile", 0.5))], 3)
    with pytest.raises(ValueError, match=r"target 3 outside \[0, 3\)"):
        normalize_boot_outputs([(3, "boot_se")], 3)
    with pytest.raises(TypeError, match="integer column position"):
        normalize_boot_outputs([(1.0, "boot_se")], 3)
    with pytest.raises(ValueError, match="an entry is"):
        normalize_boot_outputs(["boot_se"], 3)
    with pytest.raises(ValueError, match="1 to 1024"):
        normalize_boot_outputs([], 3)


# ---- estimator-level refusals, raised without a device --------------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device engine was touched ({name}) before the arguments were refused")


def fitted(weights="uniform", k=3, n=20):
    """A RawKNNRegressor in the state ``fit`` leaves it in, minus the device handle."""
    import sknnr_amd

    est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights=weights)
    rng = np.random.default_rng(0)
    est._fit_X = rng.standard_normal((n, 6))
    est._y = rng.standard_normal((n, 3))
    est.n_features_in_, est.n_samples_fit_ = 6, n
    est.effective_metric_, est.effective_metric_params_ = "euclidean", {}
    est._fit_method = "brute"
    est._affine = est._forest = est._ref_tree = None
    est._device = 0
    est._engine = _NoDevice()
    return est


X4 = np.zeros((4, 6))
IDX = np.zeros((4, 12), dtype=np.int32)
DIST = np.zeros((4, 12), dtype=np.float32)


def every_call(est, bs, **kw):
    """The four public calls with the bootstrap ``bs`` and the same extra keywords (the two that reduce stored neighbours
    take ``outputs`` but have no ``statistic``)."""
    stored = {key: v for key, v in kw.items() if key != "statistic"}
    calls = [lambda: est.summarize(X4, bootstrap=bs, **kw), lambda: est.predict_chunks([X4], bootstrap=bs, **kw)]
    if stored == kw:
        calls += [lambda: est.bootstrap_neighbors_chunks([(DIST, IDX)], bs, **kw),
                  lambda: est.bootstrap_neighbors(IDX, DIST, bootstrap=bs, **kw)]
    return calls


def test_refusals_of_every_call():
    import sknnr_amd

    bs = sknnr_amd.Bootstrap(4, n_candidates=12)
    for call in every_call(fitted(), object()):
        with pytest.raises(TypeError, match="bootstrap must be a sknnr_amd.Bootstrap"):
            call()
    for call in every_call(fitted(weights=lambda d: 1.0 / (1.0 + d)), bs):
        with pytest.raises(NotImplementedError, match="is not supported with callable weights"):
            call()
    for call in every_call(fitted(), bs, statistic="mean"):
        with pytest.raises(ValueError, match="statistic is not available with bootstrap="):
            call()
    for name in ("mean", "mode", "min", "max", "nearest", "std"):
        for call in every_call(fitted(), bs, outputs=[(0, name)]):
            with pytest.raises(ValueError, match="not available with bootstrap="):
                call()
    for call in every_call(fitted(), sknnr_amd.Bootstrap(multiplicity=np.ones((4, 21), dtype=int), n_candidates=12)):
        with pytest.raises(ValueError, match="bound to n = 21"):
            call()
    assert bs.pixels == 0 and bs.replicates_used == 0


def test_refusals_of_the_candidates():
    import sknnr_amd

    est = fitted(k=5)
    for call in every_call(est, sknnr_amd.Bootstrap(4, n_candidates=4))[:2]:
        with pytest.raises(ValueError, match="n_neighbors = 5 exceeds n_candidates = 4"):
            call()
    for call in every_call(est, sknnr_amd.Bootstrap(4, n_candidates=21))[:2]:
        with pytest.raises(ValueError, match="n_candidates = 21 exceeds the 20 rows"):
            call()
    with pytest.raises(ValueError, match="n_candidates = 20 exceeds the 19 rows"):  # (X=None: a row is no neighbour of itself)
        est.summarize(None, bootstrap=sknnr_amd.Bootstrap(4, n_candidates=20))
    # stored neighbours: the candidates are the stored columns in use
    with pytest.raises(ValueError, match="n_neighbors = 5 exceeds the 4 candidates in use"):
        est.bootstrap_neighbors(IDX, DIST, bootstrap=sknnr_amd.Bootstrap(4), n_neighbors=4)
    with pytest.raises(ValueError, match="is above the 12 stored neighbour columns"):
        est.bootstrap_neighbors(IDX, DIST, bootstrap=sknnr_amd.Bootstrap(4, n_candidates=13))
    # every stored column is a candidate by default: more than 192 of them, or more than there are fitted rows, are refused
    # here, not by the device entry
    wide = fitted(k=5, n=300)
    with pytest.raises(ValueError, match="200 candidates in use exceed the limit of 192"):
        wide.bootstrap_neighbors(np.zeros((4, 200), dtype=np.int32), bootstrap=sknnr_amd.Bootstrap(4))
    with pytest.raises(ValueError, match="25 candidates in use exceed the 20 rows"):
        est.bootstrap_neighbors(np.zeros((4, 25), dtype=np.int32), bootstrap=sknnr_amd.Bootstrap(4))


def test_refusals_of_the_streamed_keywords():
    import sknnr_amd

    bs = sknnr_amd.Bootstrap(4, n_candidates=12)
    est = fitted()
    zonal = sknnr_amd.ZonalStats(3)
    streamed = lambda **kw: [lambda: est.predict_chunks([X4], bootstrap=bs, **kw)]  # noqa: E731
    for call in streamed(zones=[np.zeros(4, dtype=int)], zonal=zonal):
        with pytest.raises(ValueError, match="a zonal sum of pixel standard errors is not the standard error of the zonal mean"):
            call()
    for call in streamed(usage=sknnr_amd.NeighborUsage()):
        with pytest.raises(ValueError, match="usage is not available with bootstrap="):
            call()
    for call in streamed(domain=object()):
        with pytest.raises(ValueError, match="domain is not available with bootstrap="):
            call()
    with pytest.raises(ValueError, match="return_neighbors is not available with bootstrap="):
        est.predict_chunks([X4], bootstrap=bs, return_neighbors=True)
    for call in streamed(out_dtype=np.int16) + [lambda: est.bootstrap_neighbors_chunks([(DIST, IDX)], bs, out_dtype=np.int16)]:
        with pytest.raises(ValueError, match="out_nodata"):  # (the planes can be NaN: an integer type needs its nodata value)
            call()
    # the replay of stored neighbours keeps its parameter list; the bootstrap planes have an entry of their own, which has
    # none of the keywords a bootstrap refuses
    import inspect

    assert "bootstrap" not in inspect.signature(type(est).predict_neighbors_chunks).parameters
    assert list(inspect.signature(type(est).bootstrap_neighbors_chunks).parameters)[1:] == [
        "neighbor_tiles", "bootstrap", "y", "n_neighbors", "ids", "fill_index", "unknown", "out", "layout", "out_dtype", "scale",
        "offset", "out_nodata", "outputs"]
    with pytest.raises(TypeError, match="bootstrap must be a sknnr_amd.Bootstrap"):
        est.bootstrap_neighbors_chunks([(DIST, IDX)], None)


def test_boot_names_need_a_bootstrap():
    est = fitted()
    for call in (lambda: est.summarize(X4, outputs=[(0, "boot_se")]), lambda: est.summarize(X4, statistic="boot_mean"),
                 lambda: est.predict_chunks([X4], outputs=["boot_count"]),
                 lambda: est.predict_neighbors(IDX, DIST, outputs=[(1, "boot_bias")])):
        with pytest.raises(ValueError, match="need bootstrap="):
            call()


def test_host_side_tie_policies_refuse():
    import sknnr_amd

    est = fitted()
    est._fit_method = "kd_tree"
    with sknnr_amd.tree_tie_policy("tree"):
        for call in every_call(est, sknnr_amd.Bootstrap(4, n_candidates=12)):
            with pytest.raises(NotImplementedError, match=r"not supported under tree_tie_policy\('tree'\)"):
                call()
