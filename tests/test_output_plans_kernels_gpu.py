"""The plan kernels (sknnr_amd/csrc/plan.hip.h) run alone through ``sknnr_summarize_plan_from_neighbors`` on synthetic
``(dist, idx)`` -- no search runs here, so the wide path costs none -- and compared with the numpy restatement
(tests/_output_plans.py) by ``assert_array_equal`` over the WHOLE output buffer: every value (NaN positions equal) and the 64
guard bytes in front of and behind it, which must keep their pattern.  The scheme is that of
test_neighbor_stats_kernels_gpu.py; every device buffer carries 257 rows of slack.

Shapes: nq of {1, 255, 256, 257, 1000} x k of {1, 2, 5, 8} (the register path with its padded slots) and {9, 17, 129, 192}
(the wide path, on both sides of numpy's 128-term split) x the three weight modes; every case runs four plans over a 300-row
``y`` with t = 3: one entry; 7 entries with repeated and unordered targets; all six old statistics of one target plus three
quantiles; and ``(j, "mean")`` for every j in order.  The q rotate over {0, 0.1, 0.5, 0.9, 1}.

Data: column 0 holds labels of 5 levels (inexact values in several binades), column 1 continuous values, column 2 five
levels among them -0.0 and 0.0 (equal values that keep neighbour order).  Distances are multiples of 0.5, sorted, one row in
eight starting with exact zeros; explicit weights come from {0, 0.5, 1, 2, 1/3, 0.1} with some rows all zero (NaN) and, in
one row of four, weight 0 on the smallest value (a leading zero in sorted order: the ``cdf != 0`` rule).

Every case checks, per plan: the values against the restatement; per entry with one of the six old statistics, the plane
against column j of the existing ``summarize_from_neighbors`` with that statistic; ``sknnr_debug_last_plan`` (the path, and
that the predict kernels ran exactly when the plan holds a mean); and that the host-memory call gives the same bits as the
device-memory one.

One more test runs reductions of every kind one after another on one handle (searches on a small handle of its own): each
gives the bits it gives alone on a fresh handle, so a handle carries nothing from one call's reduction into the next.

Without the feature every test here fails with ``AttributeError`` (``Index`` has no ``summarize_plan_from_neighbors_device``)."""

from __future__ import annotations

import numpy as np
import pytest

import _neighbor_stats as NS
import _output_plans as OP

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
SLACK_ROWS = 257
NQS = (1, 255, 256, 257, 1000)
KS = (1, 2, 5, 8, 9, 17, 129, 192)
WEIGHTS = ("uniform", "distance", "explicit")
QS = (0.0, 0.1, 0.5, 0.9, 1.0)
N_REF = 300
T = 3


def targets():
    rng = np.random.default_rng(77)
    levels = 3.0 * np.arange(5) - 2.0 + rng.uniform(0.05, 0.45, size=5) * np.exp2(rng.integers(-6, 2, size=5))
    zeros = np.array([-1.5, -0.0, 0.0, 2.25, 7.1])
    return np.ascontiguousarray(np.stack([levels[rng.integers(0, 5, size=N_REF)], rng.standard_normal(N_REF) * 10.0,
                                          zeros[rng.integers(0, 5, size=N_REF)]], axis=1))


Y = targets()


def neighbours(nq, k, weights, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N_REF, size=(nq, k)).astype(np.int64)
    dist = np.sort(rng.integers(1, 13, size=(nq, k)) * 0.5, axis=1)
    for r in np.flatnonzero(rng.integers(0, 8, size=nq) == 0):
        dist[r, : min(k, 1 + r % 3)] = 0.0
    w = None
    if weights == "explicit":
        w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 1 / 3, 0.1]), size=(nq, k))
        rows = np.flatnonzero(rng.integers(0, 4, size=nq) == 0)
        w[rows, np.argmin(Y[idx[rows], 1], axis=1)] = 0.0  # a leading zero in column 1's sorted order
        w[rng.integers(0, 16, size=nq) == 0] = 0.0
    return dist, idx, w


def plans(n):
    """The four plans of case number ``n``; the q rotate with it."""
    q = lambda i: ("quantile", QS[(n + i) % 5])  # noqa: E731
    j = (n // 3) % 3
    return [
        [(j, q(0))],
        [(2, q(1)), (0, "mode"), (2, "mean"), (1, q(2)), (0, q(3)), (2, "std"), (1, "median")],
        [(j, s) for s in NS.STATISTICS] + [(j, q(4)), (j, q(5)), (j, q(6))],
        [(c, "mean") for c in range(T)],
    ]


def cases():
    return [(nq, k, WEIGHTS[c], a * len(KS) * 3 + b * 3 + c)
            for a, nq in enumerate(NQS) for b, k in enumerate(KS) for c in range(3)]


def test_the_rotation_covers():
    """On the case list alone: every q and every target meet both paths under every weight mode."""
    for weights in WEIGHTS:
        for small in (True, False):
            mine = [plans(n) for nq, k, w, n in cases() if w == weights and (k <= 8) == small]
            for p in range(3):
                got = {(j, OP.split(s)[1]) for pl in mine for j, s in pl[p] if OP.split(s)[0] == "quantile"}
                assert {q for _, q in got} == set(QS) and {j for j, _ in got} == {0, 1, 2}, (weights, small, p)


@pytest.fixture(scope="module")
def index():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    ix = _native.Index(np.random.default_rng(5).standard_normal((N_REF, 2)), Y)
    yield ix
    ix.close()


def guarded(nbytes, slack):
    import torch

    host = np.full(GUARD + nbytes + GUARD + slack, PATTERN, dtype=np.uint8)
    return host, torch.from_numpy(host.copy()).cuda()


def padded(a, fill):
    import torch

    return torch.from_numpy(np.concatenate([a, np.full((SLACK_ROWS, a.shape[1]), fill, dtype=a.dtype)])).cuda()


@pytest.mark.parametrize("nq, k, weights, n", cases())
def test_plan_kernels(index, nq, k, weights, n):
    import torch

    from sknnr_amd import _native

    ix = index
    dist, idx, w = neighbours(nq, k, weights, seed=nq * 1000 + k * 7)
    d_dist, d_idx = padded(dist, 1.0), padded(idx, 0)
    d_w = padded(w, 1.0) if w is not None else None
    ptrs = (d_dist.data_ptr(), d_idx.data_ptr(), 0 if d_w is None else d_w.data_ptr(), nq, k)
    mode = {"uniform": _native.WEIGHTS_UNIFORM, "distance": _native.WEIGHTS_DISTANCE, "explicit": _native.WEIGHTS_EXPLICIT}[weights]
    stream = torch.cuda.current_stream().cuda_stream
    old = {}  # the existing entry's (nq, t) result per statistic name

    def old_column(name, j):
        if name not in old:
            out = torch.empty((nq, T), dtype=torch.float64, device="cuda")
            ix.summarize_from_neighbors_device(*ptrs, mode, np.full(T, NS.CODES[name], dtype=np.int32), out.data_ptr(), stream)
            torch.cuda.synchronize()
            old[name] = out.cpu().numpy()
        return old[name][:, j]

    for plan in plans(n):
        n_out = len(plan)
        arrays = OP.arrays(plan)
        want = OP.plan_of(Y, dist, idx, w, weights, plan)
        host, d_out = guarded(nq * n_out * 8, SLACK_ROWS * n_out * 8)
        ix.summarize_plan_from_neighbors_device(*ptrs, mode, arrays, d_out.data_ptr() + GUARD, stream)
        rec = ix.debug_last_plan()
        srec = ix.debug_last_summary()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        msg = f"nq={nq} k={k} {weights} {plan}"
        end = GUARD + nq * n_out * 8
        values = got[GUARD:end].view(np.float64).reshape(nq, n_out)
        np.testing.assert_array_equal(values, want, err_msg=msg)
        np.testing.assert_array_equal(got[:GUARD], host[:GUARD], err_msg="front guard: " + msg)
        np.testing.assert_array_equal(got[end:], host[end:], err_msg="back guard: " + msg)
        n_mean = sum(s == "mean" for _, s in plan)
        assert rec == dict(ran=1, path=1 if k <= 8 else 2, rows=nq, n_out=n_out, k=k, n_mean=n_mean,
                           predict_ran=int(n_mean > 0), reserved=0), msg
        assert srec["path"] == 0 and srec["cols"] == 0 and srec["predict_ran"] == int(n_mean > 0), msg
        for e, (j, s) in enumerate(plan):
            if isinstance(s, str) and s in NS.CODES:
                np.testing.assert_array_equal(values[:, e], old_column(s, j), err_msg=f"entry {e} vs summarize: " + msg)
        # host memory in and out: the same bits
        on_host = ix.summarize_plan_from_neighbors_host(None if weights == "uniform" else dist, idx, w, mode, arrays)
        np.testing.assert_array_equal(on_host.view(np.uint64), np.ascontiguousarray(values).view(np.uint64), err_msg="host: " + msg)
    # a reduction without a plan clears the plan record
    out = torch.empty((nq, T), dtype=torch.float64, device="cuda")
    ix.summarize_from_neighbors_device(*ptrs, mode, np.full(T, NS.CODES["max"], dtype=np.int32), out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert ix.debug_last_plan()["ran"] == 0 and ix.debug_last_summary()["path"] == (1 if k <= 8 else 2)


def test_a_handle_carries_no_reduction_into_the_next_call():
    """Seven calls of different reductions on ONE handle -- a plan, a mean, a statistics table, three masked means (no row,
    a third of the rows, every row holding nodata), a stream with an all-mean table, a bootstrap stream, a mean again --
    give, call by call, the bits of the same call on a fresh handle; the two plain means are equal and leave no plan record."""
    from sknnr_amd import _native

    n_ref, d, t, k, nq, B, kw = 300, 8, 3, 5, 257, 8, 8
    rng = np.random.default_rng(2024)
    ref, y, q = rng.standard_normal((n_ref, d)), rng.standard_normal((n_ref, t)), rng.standard_normal((nq, d))
    table = np.stack([np.bincount(rng.integers(0, n_ref, n_ref), minlength=n_ref) for _ in range(B)]).astype(np.uint8)
    nodata = np.full(d, -9999.0)
    third, every = q.copy(), q.copy()
    third[rng.permutation(nq)[: nq // 3], rng.integers(0, d, nq // 3)] = -9999.0
    every[np.arange(nq), rng.integers(0, d, nq)] = -9999.0
    plan = OP.arrays([(1, ("quantile", 0.25)), (0, "max"), (1, "mean"), (1, "median")])
    mixed = np.array([NS.CODES["max"], NS.CODES["mean"], NS.CODES["std"]], dtype=np.int32)
    boot = (np.array([0, 2, 0], dtype=np.int32),
            np.array([_native.BOOT_STATISTICS[s] for s in ("boot_se", "boot_mean", "boot_count")], dtype=np.int32))
    opts, opts_kw = _native.Index.make_opts(k), _native.Index.make_opts(kw)

    def plain(ix):
        out = ix.predict_host(q, opts)
        assert ix.debug_last_plan()["ran"] == 0
        return [out]

    def masked(ix):
        outs = [ix.predict_masked_host(x, opts, nodata) for x in (q, third, every)]
        assert [nv for _, nv in outs] == [nq, nq - nq // 3, 0]  # (mask_finish: in place, packed and expanded, the fill alone)
        return [pred for pred, _ in outs]

    def stream(ix):
        with ix.open_stream(opts, want_dist=False, want_pred=True) as s:
            s.set_statistics(np.zeros(t, dtype=np.int32))
            outs = [s.push(x, need_idx=False)[2] for x in (q[:130], q[130:])]
        return outs

    def boot_stream(ix):
        with ix.open_stream(opts_kw, want_dist=False, want_pred=True) as s:
            s.set_bootstrap(k, boot)
            outs = [s.push(q, need_idx=False)[2]]
        return outs

    steps = [lambda ix: [ix.summarize_plan_host(q, opts, plan)], plain, lambda ix: [ix.summarize_host(q, opts, mixed)],
             masked, stream, boot_stream, plain]

    def fresh():
        ix = _native.Index(ref, y)
        ix.set_bootstrap(table)
        return ix

    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)  # noqa: E731
    one = fresh()
    got = [step(one) for step in steps]
    one.close()
    assert got[0][0].shape == (nq, 4) and got[5][0].shape == (nq, 3) and np.isnan(got[3][2]).all()
    assert np.isnan(got[3][1]).any(axis=1).sum() == nq // 3 and not np.isnan(got[3][0]).any()
    for n, step in enumerate(steps):
        ix = fresh()
        want = step(ix)
        ix.close()
        assert len(want) == len(got[n])
        for a, b in zip(got[n], want):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"step {n + 1}"
    assert np.array_equal(bits(got[1][0]), bits(got[6][0]))


def test_uniform_quantile_ends_are_min_and_max(index):
    dist, idx, _ = neighbours(513, 8, "uniform", seed=3)
    for k in (8, 17):
        ii = np.ascontiguousarray(np.tile(idx, (1, 3))[:, :k])
        plan = [(j, s) for j in range(T) for s in (("quantile", 0.0), "min", ("quantile", 1.0), "max")]
        got = index.summarize_plan_from_neighbors_host(None, ii, None, 0, OP.arrays(plan))
        np.testing.assert_array_equal(got[:, 0::4], got[:, 1::4])
        np.testing.assert_array_equal(got[:, 2::4], got[:, 3::4])


def test_refusals_of_the_c_entries(index):
    """Every refusal comes before any device work, with a message naming the entry."""
    import ctypes

    from sknnr_amd import _native

    lib = _native.load()
    INV = _native.ERR_INVALID
    h = index.handle
    buf = (ctypes.c_uint64 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)  # noqa: E731
    opts = _native.Index.make_opts(3)

    def both(cols, stat, param, n_out, text):
        for rc in (lib.sknnr_summarize_plan_from_neighbors(h, p, p, None, 2, 3, 0, cols, stat, param, n_out, p, 0, None),
                   lib.sknnr_summarize_plan(h, p, 2, ctypes.byref(opts), cols, stat, param, n_out, p, None, None, 0, None)):
            assert rc == INV and text in lib.sknnr_last_error(), (text, lib.sknnr_last_error())

    ok = (i32(0, 2), i32(0, 6), f64(0.0, 0.5))
    both(None, ok[1], ok[2], 2, b"is NULL")
    both(ok[0], None, ok[2], 2, b"is NULL")
    both(ok[0], ok[1], None, 2, b"is NULL")
    both(*ok, 0, b"n_out = 0 outside [1, 1024]")
    both(*ok, 1025, b"n_out = 1025 outside [1, 1024]")
    both(i32(0, 3), ok[1], ok[2], 2, b"cols[1] = 3")
    both(i32(-1, 0), ok[1], ok[2], 2, b"cols[0] = -1")
    both(ok[0], i32(0, 7), ok[2], 2, b"stat[1] = 7 is no sknnr_statistic")
    both(ok[0], i32(-1, 6), ok[2], 2, b"stat[0] = -1 is no sknnr_statistic")
    for q in (1.5, -0.25, float("nan"), float("inf")):
        both(ok[0], ok[1], f64(0.0, q), 2, b"param[1]")
    assert lib.sknnr_summarize_plan_from_neighbors(h, p, p, None, 2, 193, 0, *ok, 2, p, 0, None) == _native.ERR_UNSUPPORTED
    assert lib.sknnr_summarize_plan_from_neighbors(h, None, p, None, 2, 3, 1, *ok, 2, p, 0, None) == INV
    assert lib.sknnr_summarize_plan_from_neighbors(h, p, p, None, 2, 3, 2, *ok, 2, p, 0, None) == INV
    # a parameter of another statistic is not read
    assert lib.sknnr_summarize_plan_from_neighbors(h, p, p, None, 0, 3, 0, ok[0], i32(0, 1), f64(9.0, -3.0), 2, p, 0, None) == 0


def test_refusals_of_the_stream_entry(index):
    from sknnr_amd import _native

    plan = OP.arrays([(0, "mean"), (0, ("quantile", 0.5))])
    stat = np.zeros(T, dtype=np.int32)
    opts = _native.Index.make_opts(3)
    with index.open_stream(opts, want_dist=False, want_pred=False) as s:
        with pytest.raises(_native.HipBackendError, match="opened without predictions"):
            s.set_plan(plan)
    with index.open_stream(opts, want_dist=False, want_pred=True) as s:
        s.set_statistics(stat)  # (an all-mean table counts: whichever comes second is refused)
        with pytest.raises(_native.HipBackendError, match="it takes no output plan"):
            s.set_plan(plan)
    with index.open_stream(opts, want_dist=False, want_pred=True) as s:
        s.set_plan(plan)
        with pytest.raises(_native.HipBackendError, match="it takes no per-target statistics"):
            s.set_statistics(stat)
        with pytest.raises(_native.HipBackendError, match=r"cols\[0\] = 5"):
            s.set_plan(OP.arrays([(5, "mean")]))
        _, _, pred = s.push(np.zeros((4, 2)), need_idx=False)
        assert pred.shape == (4, 2)
        with pytest.raises(_native.HipBackendError, match="only before the first push"):
            s.set_plan(plan)
    with index.open_stream(opts, want_dist=False, want_pred=True) as s:
        s.set_output(pred_dtype=np.int16, scale=np.ones(T), offset=np.zeros(T), fill=-1)
        with pytest.raises(_native.HipBackendError, match="comes before sknnr_stream_set_output"):
            s.set_plan(plan)
