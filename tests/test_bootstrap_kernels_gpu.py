"""The bootstrap kernel (sknnr_amd/csrc/bootstrap.hip.h) run alone through ``sknnr_bootstrap_from_neighbors`` on synthetic
``(dist, idx)`` lists -- no search runs here -- and compared with the numpy restatement (tests/_bootstrap.py) by
``assert_array_equal`` over the WHOLE output buffer: every value (NaN positions equal) and the 64 guard bytes in front of and
behind it, which must keep their pattern.  The scheme is that of test_output_plans_kernels_gpu.py; every device buffer
carries 257 rows of slack, and the two tally words sit between two guard words.

Shapes, rotated rather than crossed (``test_the_rotation_covers`` proves on the case list alone that every value meets every
weight mode): nq of {1, 63, 64, 65, 1000} x (k, kw) of {(1,1), (1,8), (5,5), (5,8), (5,20), (8,64), (9,40), (17,192),
(192,192)} x B of {1, 2, 31, 32, 33, 64, 65, 200, 257} -- one, two and four pixels per wave, one pass and several, B on both
sides of every segment width, the packed layouts met by every weight mode on lists of 8 and 20 columns -- x weights uniform, ``distance``, ``InverseDistance(1)`` and ``Triangular(4)``.  t = 3 over a
300-row ``y``; every case runs three plans that repeat and reorder targets and include ``boot_count``.  Two more cases lie
above the launch's grid cap (20001 pixels at one per wave, 40003 at four), where a workgroup takes several pixel groups.

A neighbour list never repeats a row: every pixel's list is the head of a random permutation of the rows.  Distances are
multiples of 0.5, sorted, one row in eight starting with exact zeros; ``Triangular(4)`` vanishes on part of every longer list.

Crafted rows (``test_crafted_rows``, every weight mode at B of 16, 32 and 33: four, two and one pixel per wave): every multiplicity of a pixel's list zero (count 0, NaN); ``M >= k``
on the first present neighbour; ``M = 255``; ``d == 0`` inside the taken set; ``d == 0`` only on an absent neighbour; ``m == 1``
(``boot_se`` NaN, ``boot_mean`` finite); a compact law that vanishes for ``p0``; a list that names row -1.

Without the feature every test here fails with ``AttributeError`` (``Index`` has no ``set_bootstrap``)."""

from __future__ import annotations

import numpy as np
import pytest

import _bootstrap as BS

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
SLACK_ROWS = 257
NQS = (1, 63, 64, 65, 1000)
KKS = ((1, 1), (1, 8), (5, 5), (5, 8), (5, 20), (8, 64), (9, 40), (17, 192), (192, 192))
BBS = (1, 2, 31, 32, 33, 64, 65, 200, 257)
WEIGHTS = ("uniform", "distance", "inverse", "triangular")
N_REF = 300
T = 3
N_CASES = 36


def law_of(name):
    from sknnr_amd import weights as W

    return {"uniform": "uniform", "distance": "distance", "inverse": W.InverseDistance(1.0),
            "triangular": W.Triangular(4.0)}[name]


def targets():
    rng = np.random.default_rng(91)
    levels = 3.0 * np.arange(5) - 2.0 + rng.uniform(0.05, 0.45, size=5) * np.exp2(rng.integers(-6, 2, size=5))
    return np.ascontiguousarray(np.stack([levels[rng.integers(0, 5, size=N_REF)], rng.standard_normal(N_REF) * 10.0,
                                          rng.uniform(100.0, 101.0, size=N_REF)], axis=1))


Y = targets()


def neighbours(nq, kw, seed):
    rng = np.random.default_rng(seed)
    idx = np.argsort(rng.random((nq, N_REF)), axis=1)[:, :kw].astype(np.int64)
    dist = np.sort(rng.integers(1, 13, size=(nq, kw)) * 0.5, axis=1)
    for r in np.flatnonzero(rng.integers(0, 8, size=nq) == 0):
        dist[r, : min(kw, 1 + r % 3)] = 0.0
    return dist, idx


def plans(n):
    j = n % 3
    return [
        [(j, ("boot_se", "boot_mean", "boot_bias")[(n // 3) % 3])],
        [(2, "boot_mean"), "boot_count", (0, "boot_se"), (2, "boot_se"), (1, "boot_bias"), (0, "boot_mean"), (2, "boot_mean")],
        ["boot_count"] if n % 2 else [(c, "boot_se") for c in range(T)],
    ]


def cases():
    return [(NQS[n % 5], *KKS[n % 9], BBS[(7 * n) % 9], WEIGHTS[n % 4], n) for n in range(N_CASES)]


def test_the_rotation_covers():
    """On the case list alone: every nq, every (k, kw) and every B meet every weight mode, and so do two and four pixels per
    wave on lists with something to walk (kw >= 5, B > 1)."""
    from sknnr_amd import _native

    cs = cases()
    for w in WEIGHTS:
        mine = [c for c in cs if c[4] == w]
        assert {c[0] for c in mine} == set(NQS), w
        assert {(c[1], c[2]) for c in mine} == set(KKS), w
        assert {c[3] for c in mine} == set(BBS), w
        packed = {_native.bootstrap_pixels_per_wave(c[3], c[2]) for c in mine if c[2] >= 5 and c[3] > 1}
        assert packed == {1, 2, 4}, (w, packed)


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


def modes(ix, weights):
    """``(weight_mode, weight_law)`` of the C entry, the law's parameters put on the handle."""
    from sknnr_amd import _native

    law = law_of(weights)
    if isinstance(law, str):
        return {"uniform": _native.WEIGHTS_UNIFORM, "distance": _native.WEIGHTS_DISTANCE}[law], 0
    ix.set_weight_law_params(law.code, *law.params)
    return _native.WEIGHTS_EXPLICIT, law.code


def run_and_compare(ix, dist, idx, M, k, weights, plan, msg):
    """One device-memory call over guarded buffers against the restatement, then the host-memory call: the same bits."""
    import torch

    from sknnr_amd import _native

    nq, kw = idx.shape
    B = M.shape[0]
    mode, law = modes(ix, weights)
    n_out = len(plan)
    arrays = BS.arrays(plan)
    want, want_tally, info = BS.bootstrap_of(Y, dist, idx, M, k, law_of(weights), plan, want_info=True)
    d_dist, d_idx = padded(dist, 1.0), padded(idx, 0)
    host, d_out = guarded(nq * n_out * 8, SLACK_ROWS * n_out * 8)
    tally0 = np.array([-7, 123, 456, -9], dtype=np.int64)
    d_tally = torch.from_numpy(tally0.copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ix.bootstrap_from_neighbors_device(0 if weights == "uniform" else d_dist.data_ptr(), d_idx.data_ptr(), nq, kw, k, arrays,
                                       d_out.data_ptr() + GUARD, d_tally.data_ptr() + 8, mode, law, stream)
    rec = ix.debug_last_bootstrap()
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    end = GUARD + nq * n_out * 8
    values = got[GUARD:end].view(np.float64).reshape(nq, n_out)
    np.testing.assert_array_equal(values, want, err_msg=msg)
    np.testing.assert_array_equal(got[:GUARD], host[:GUARD], err_msg="front guard: " + msg)
    np.testing.assert_array_equal(got[end:], host[end:], err_msg="back guard: " + msg)
    np.testing.assert_array_equal(d_tally.cpu().numpy(), [tally0[0], want_tally[0], want_tally[1], tally0[3]], err_msg=msg)
    assert rec == dict(rows=nq, B=B, k=k, kw=kw, n_out=n_out, pixels_per_wave=_native.bootstrap_pixels_per_wave(B, kw),
                       launches=1, reserved=0), msg
    on_host, host_tally = ix.bootstrap_from_neighbors_host(None if weights == "uniform" else dist, idx, k, arrays, mode, law)
    np.testing.assert_array_equal(on_host.view(np.uint64), np.ascontiguousarray(values).view(np.uint64), err_msg="host: " + msg)
    np.testing.assert_array_equal(host_tally, want_tally, err_msg="host tally: " + msg)
    return values, info


EDGES = {}  # case number -> (short pairs, truncated copies, pixels with m < 2) of its restatement


def edges_of(info):
    return (int(info["short"].sum()), int(((info["c"] > 0) & (info["c"] < info["mult"])).sum()), int((info["m"] < 2).sum()))


def case_inputs(nq, kw, B, n):
    dist, idx = neighbours(nq, kw, seed=nq * 1000 + kw * 7 + n)
    M = BS.draw_table(B, N_REF, seed=n)
    if n % 3 == 0:
        M[:, ::7] = np.minimum(M[:, ::7] * 100, 300)  # (multiplicities the table clamps to 255)
    return dist, idx, M


@pytest.mark.parametrize("nq, k, kw, B, weights, n", cases())
def test_bootstrap_kernel(index, nq, k, kw, B, weights, n):
    dist, idx, M = case_inputs(nq, kw, B, n)
    index.set_bootstrap(M)
    for p, plan in enumerate(plans(n)):
        _, info = run_and_compare(index, dist, idx, M, k, weights, plan, f"nq={nq} k={k} kw={kw} B={B} {weights} plan {p}")
    EDGES[n] = edges_of(info)


@pytest.mark.parametrize("nq, k, kw, B, weights", [(20001, 5, 8, 33, "distance"), (40003, 3, 8, 2, "uniform")])
def test_more_pixel_groups_than_workgroups(index, nq, k, kw, B, weights):
    """The launch caps its grid at 2048 workgroups of 4 waves: above 8192 pixel groups of one pixel per wave (32768 pixels at
    four per wave) a workgroup takes several groups in turn and carries its tallies across them."""
    from sknnr_amd import _native

    assert nq > 2048 * 4 * _native.bootstrap_pixels_per_wave(B, kw)
    dist, idx, M = case_inputs(nq, kw, B, 5)
    index.set_bootstrap(M)
    run_and_compare(index, dist, idx, M, k, weights, [(1, "boot_se"), "boot_count", (0, "boot_mean")], f"nq={nq} B={B}")


def test_every_family_met_the_edges():
    """From the restatement alone (shared with the cases above where they ran): each weight mode has a short pair, a
    truncated copy and a pixel with m < 2."""
    for w in WEIGHTS:
        seen = np.zeros(3, dtype=np.int64)
        for nq, k, kw, B, weights, n in cases():
            if weights != w:
                continue
            if n not in EDGES:
                dist, idx, M = case_inputs(nq, kw, B, n)
                EDGES[n] = edges_of(BS.bootstrap_of(Y, dist, idx, M, k, law_of(w), ["boot_count"], want_info=True)[2])
            seen += EDGES[n]
        assert (seen > 0).all(), (w, seen)


@pytest.mark.parametrize("B", [16, 32, 33])  # (four pixels per wave, two, one)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_crafted_rows(index, weights, B):
    from sknnr_amd import _native

    nq, k, kw = 64, 5, 8
    assert _native.bootstrap_pixels_per_wave(B, kw) == {16: 4, 32: 2, 33: 1}[B]
    dist, idx = neighbours(nq, kw, seed=17)
    idx = np.where(idx >= 270, idx - 100, idx)  # (rows 270 .. 299 are reserved for the crafted pixels)
    dist[:8] = np.arange(1, kw + 1) * 0.5       # (none of the crafted pixels starts with an accidental zero)
    M = BS.draw_table(B, N_REF, seed=3)
    absent = np.arange(280, 288)
    M[:, absent] = 0
    M[:, 288] = k + 2
    M[:, 289] = 255
    M[:, 279] = 0
    M[0, 279] = k
    idx[0] = absent                      # 0: every multiplicity zero
    idx[1, 0] = 288                      # 1: M >= k on the first present neighbour
    idx[2, 0] = 289                      # 2: M = 255
    idx[3, 0], dist[3, 0] = 288, 0.0     # 3: d == 0 inside the taken set
    idx[4, 0], dist[4, 0] = 280, 0.0     # 4: d == 0 only on an absent neighbour
    idx[5] = absent
    idx[5, 3] = 279                      # 5: one valid replicate
    dist[6] = 4.0 + np.arange(kw) * 0.5  # 6: Triangular(4) vanishes on the whole list
    idx[7, 2] = -1                       # 7: a blanked list
    index.set_bootstrap(M)
    plan = [(c, s) for c in range(T) for s in ("boot_se", "boot_mean", "boot_bias")] + ["boot_count"]
    v, info = run_and_compare(index, dist, idx, M, k, weights, plan, f"crafted {weights}")
    se, mean, bias, count = v[:, 0:9:3], v[:, 1:9:3], v[:, 2:9:3], v[:, 9]
    assert count[0] == 0 and np.isnan(v[0, :9]).all()
    for q in (1, 2, 3):  # every replicate is k copies of row 288 / 289: none is short, and rows 1 and 2 truncate a copy
        assert count[q] == B
        assert ((info["c"][q, :, 0] == k) & (info["mult"][q, :, 0] > k)).all()
    assert np.isfinite(v[1:4, :9]).all()
    if weights == "distance":
        np.testing.assert_array_equal(info["p0"][3], Y[288])  # (the mask of the one zero distance, in p0 and in every replicate)
        assert (np.abs(bias[3]) <= 1e-12 * np.abs(Y[288])).all()
        np.testing.assert_array_equal(info["p0"][4], Y[280])  # (p0 is the mask of the absent row; no replicate is)
        assert count[4] > 0 and (np.abs(bias[4]) > 1e-6).any()
    assert count[5] == 1 and np.isnan(se[5]).all() and np.isfinite(mean[5]).all() and np.isfinite(bias[5]).all()
    if weights == "triangular":
        assert count[6] == 0 and np.isnan(v[6, :9]).all()
    else:
        assert count[6] > 0
    assert count[7] == 0 and np.isnan(v[7, :9]).all() and info["bad"][7] and info["bad"].sum() == 1


def test_refusals_of_the_c_entries(index):
    """Every refusal comes before any device work."""
    import ctypes

    from sknnr_amd import _native

    lib = _native.load()
    INV = _native.ERR_INVALID
    h = index.handle
    buf = (ctypes.c_uint64 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    table = np.ones((4, N_REF), dtype=np.uint8)
    tp = table.ctypes.data_as(ctypes.c_void_p)

    def call(kw=8, k=5, mode=0, law=0, cols=i32(0, 2), stat=i32(0, 1), n_out=2, dist=p, idx=p, out=p, mem=0):
        return lib.sknnr_bootstrap_from_neighbors(h, dist, idx, 2, kw, k, mode, law, cols, stat, n_out, out, None, mem, None)

    assert lib.sknnr_index_set_bootstrap(h, None, 0, 0) == 0
    assert call() == INV and b"no bootstrap table" in lib.sknnr_last_error()
    assert lib.sknnr_index_set_bootstrap(h, tp, 0, N_REF) == INV
    assert lib.sknnr_index_set_bootstrap(h, tp, 4097, N_REF) == INV
    assert lib.sknnr_index_set_bootstrap(h, tp, 4, N_REF - 1) == INV and b"reference rows" in lib.sknnr_last_error()
    assert lib.sknnr_index_set_bootstrap(h, tp, 4, N_REF) == 0
    for kwargs in (dict(k=0), dict(k=9), dict(kw=193, k=5), dict(kw=0, k=0), dict(n_out=0), dict(n_out=1025),
                   dict(cols=i32(0, 3)), dict(cols=i32(-1, 0)), dict(stat=i32(0, 4)), dict(stat=i32(-1, 0)), dict(cols=None),
                   dict(stat=None), dict(mode=2), dict(mode=3), dict(mode=0x100), dict(mode=1, dist=None), dict(idx=None),
                   dict(out=None), dict(mem=7), dict(law=9, mode=2)):
        assert call(**kwargs) == INV, kwargs
    small = _native.Index(np.zeros((6, 2)) + np.arange(6)[:, None], np.zeros((6, 1)))
    try:
        small.set_bootstrap(np.ones((2, 6), dtype=np.uint8))
        rc = lib.sknnr_bootstrap_from_neighbors(small.handle, p, p, 2, 7, 5, 0, 0, i32(0), i32(0), 1, p, None, 0, None)
        assert rc == INV and b"exceeds the handle's 6 reference rows" in lib.sknnr_last_error()
    finally:
        small.close()
    # a boot_count entry's column is not read; nq == 0 is fine
    assert lib.sknnr_bootstrap_from_neighbors(h, p, p, 0, 8, 5, 0, 0, i32(99), i32(3), 1, p, None, 0, None) == 0
    opts = _native.Index.make_opts(3)
    with index.open_stream(opts, want_dist=False, want_pred=True):
        assert lib.sknnr_index_set_bootstrap(h, tp, 4, N_REF) == INV and b"a stream is open" in lib.sknnr_last_error()


def test_attribute_only_handles_take_a_table():
    from sknnr_amd import _native

    tix = _native.TargetIndex(Y)
    try:
        dist, idx = neighbours(65, 8, seed=2)
        M = BS.draw_table(31, N_REF, seed=8)
        tix.set_bootstrap(M)
        plan = [(1, "boot_se"), "boot_count"]
        got, tally = tix.bootstrap_from_neighbors_host(dist, idx, 5, BS.arrays(plan), _native.WEIGHTS_DISTANCE, 0)
        want, want_tally = BS.bootstrap_of(Y, dist, idx, M, 5, "distance", plan)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(tally, want_tally)
    finally:
        tix.close()
