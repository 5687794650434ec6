"""The host restatement of the query preparation and bucketing kernels (tests/_query_prep.py), checked against exact
rational arithmetic (fractions.Fraction) at a few dozen rows, and its dispatch table at the edges of launch_prep.  No GPU.

``float(Fraction)`` rounds the exact value to the nearest float64 (ties to even), so ``float(a * b + c)`` is a correctly
rounded fma and ``float(a - b)``, ``float(a / b)`` are the IEEE operations.
"""

from __future__ import annotations

from fractions import Fraction as F

import numpy as np
import pytest

import _query_prep as Q


# ---------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_dispatch_edges():
    """launch_prep: the direct kernel up to four K-steps (d <= 64) unless SKNNR_PREP_LDS is set, else rows per block by
    (d_in | 1) * 8 * BT <= 150 KiB, refusal from d_in = 300; who names the cells."""
    assert Q.expected_prep(64, 100)["kernel"] == Q.KERNEL_DIRECT
    assert Q.expected_prep(65, 100) == dict(kernel=Q.KERNEL_LDS, rows_per_block=256, x_dtype=0, nq=100, nq_pad=6144,
                                            xt_written=0, cells_by=0, affine_bits=0)
    assert Q.expected_prep(64, 100, prep_lds=True)["kernel"] == Q.KERNEL_LDS
    for d_in, rows in ((75, 256), (76, 128), (149, 128), (150, 64), (299, 64)):
        rec = Q.expected_prep(70, 6145, d_in=d_in, center=True, proj=True)
        assert (rec["kernel"], rec["rows_per_block"]) == (Q.KERNEL_LDS, rows), d_in
        assert (rec["nq"], rec["nq_pad"], rec["xt_written"], rec["affine_bits"]) == (6145, 12288, 1, 5)
    assert Q.expected_prep(70, 10, d_in=300, proj=True) is None
    assert Q.expected_prep(13, 10, d_in=300, proj=True)["kernel"] == Q.KERNEL_DIRECT  # (the direct kernel has no such limit)
    assert Q.expected_prep(13, 10, d_in=300, proj=True, prep_lds=True) is None
    # the tile of the LDS kernel at its edges, in bytes
    assert [bt * (d_in | 1) * 8 <= 150 * 1024 for bt, d_in in ((256, 75), (256, 76), (128, 149), (128, 150), (64, 299), (64, 300))] == [
        True, False, True, False, True, False]
    # cells: the direct kernel names them itself, behind the LDS kernel cell_assign_kernel does
    assert Q.expected_prep(13, 10, bucketed=True)["cells_by"] == Q.CELLS_BY_PREP
    assert Q.expected_prep(13, 10, bucketed=True, prep_lds=True)["cells_by"] == Q.CELLS_BY_ASSIGN
    assert Q.expected_prep(13, 10, x_dtype=4)["xt_written"] == 1
    assert [Q.padded_rows(n) for n in (1, 6143, 6144, 6145)] == [6144, 6144, 6144, 12288]


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [1, 3, 8])
def test_image_layout(ks):
    """qimg_index enumerates [row][hi | lo][K-step][K half] without gaps, and image_bytes puts columns 16 step + 8 kh .. + 7
    of the part into that piece: a row is its 16 ks hi halves followed by its 16 ks lo halves."""
    rows = 5
    seen = [Q.qimg_index(r, part, ks, step, kh) for r in range(rows) for part in range(2) for step in range(ks) for kh in range(2)]
    assert seen == list(range(rows * 4 * ks))
    rng = np.random.default_rng(ks)
    b = np.zeros((rows, 16 * ks))
    b[:, :16 * ks - 3] = rng.standard_normal((rows, 16 * ks - 3)) * 100.0
    hi, lo = Q.split_f16(b)
    img = Q.image_bytes(b)
    assert img.shape == (rows, 64 * ks) and img.dtype == np.uint8
    halves = img.view(np.float16).reshape(rows, 2, 16 * ks)
    np.testing.assert_array_equal(halves[:, 0].view(np.uint16), hi.view(np.uint16))
    np.testing.assert_array_equal(halves[:, 1].view(np.uint16), lo.view(np.uint16))
    piece = img.reshape(rows, 4 * ks, 16)
    for r, part, step, kh in ((0, 0, 0, 1), (3, 1, ks - 1, 0), (4, 1, ks - 1, 1)):
        k0 = 16 * step + 8 * kh
        want = (hi, lo)[part][r, k0:k0 + 8].view(np.uint8)
        np.testing.assert_array_equal(piece[r, Q.qimg_index(0, part, ks, step, kh)], want)
    assert (halves[:, :, 16 * ks - 3:].view(np.uint16) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _exact_affine(x, center, scale, proj):
    out = []
    for row in x:
        v = [float(xv) for xv in row]
        if center is not None:
            v = [float(F(a) - F(c)) for a, c in zip(v, center)]
        if scale is not None:
            v = [float(F(a) / F(sc)) for a, sc in zip(v, scale)]
        if proj is None:
            out.append(v)
            continue
        acc = [0.0] * proj.shape[1]
        for c, a in enumerate(v):
            acc = [float(F(a) * F(float(proj[c, j])) + F(acc[j])) for j in range(proj.shape[1])]
        out.append(acc)
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("parts", ["csp", "p", "cs", "c", "s"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16, np.uint8])
def test_transformed_rows_against_exact_arithmetic(parts, dtype):
    """xt: widen exactly, subtract, divide, then one k-ordered fma chain per output (36 rows, d_in 7 -> d 5)."""
    rng = np.random.default_rng(11)
    n, d_in, d = 36, 7, 5
    x = (rng.standard_normal((n, d_in)) * 50.0 + 100.0).astype(dtype)
    center = rng.standard_normal(d_in) * 30.0 + 90.0 if "c" in parts else None
    scale = rng.uniform(0.3, 7.0, d_in) if "s" in parts else None
    proj = rng.standard_normal((d_in, d)) if "p" in parts else None
    got = Q.transformed_rows(x, center, scale, proj)
    np.testing.assert_array_equal(got, _exact_affine(Q.widen(x), center, scale, proj))


def test_query_norm_against_exact_arithmetic():
    """qnc: the fma chain of b * b over all 16 ks columns in ascending order; +inf when any !(|b| < 32768); 0 on padding."""
    rng = np.random.default_rng(12)
    b = np.zeros((40, 32))
    b[:30, :19] = rng.standard_normal((30, 19)) * rng.uniform(1e-3, 3e3, (30, 1))
    b[3, 18], b[4, 0], b[5, 7], b[6, 2] = 32768.0, -32768.0, np.nextafter(32768.0, 0.0), 40000.0
    want = np.zeros(40)
    for i in range(40):
        acc = 0.0
        for v in b[i]:
            acc = float(F(float(v)) * F(float(v)) + F(acc))
        want[i] = acc
    want[[3, 4, 6]] = np.inf
    got = Q.query_norms(b)
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(got[5]) and (got[30:] == 0).all()


def test_scaled_rows_and_padding():
    rng = np.random.default_rng(13)
    xt, mu, s = rng.standard_normal((7, 13)), np.zeros(16), 0.25
    mu[:13] = rng.standard_normal(13)
    b = Q.scaled_rows(xt, mu, s, 12)
    want = np.array([[float(F(s) * F(float(F(float(xt[i, k])) - F(float(mu[k]))))) for k in range(13)] for i in range(7)])
    np.testing.assert_array_equal(b[:7, :13], want)
    assert (b[7:] == 0).all() and (b[:, 13:] == 0).all()


def test_split_reproduces_b_within_the_formats_bound():
    """hi + lo against b, exactly.  Rounding x to float32 and then to float16 moves it by at most
    E(x) = |x| 2^-24 + |x| (1 + 2^-24) 2^-11 + 2^-25 (half an ulp of each format: 24 and 11 significand bits; half the smallest
    float16 subnormal 2^-24 where the result is subnormal).  b - f64(hi) is exact in float64 (both are multiples of b's last
    place and the difference is no larger than b), so |b - hi - lo| <= E(E(|b|)) for |b| < 32768."""
    rng = np.random.default_rng(14)
    mag = 2.0 ** rng.uniform(-30, 15, (48, 16))
    b = np.minimum(mag, np.nextafter(32768.0, 0.0)) * rng.choice([-1.0, 1.0], (48, 16))
    b[0, :6] = [0.0, 2.0 ** -25, 2.0 ** -24, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, np.nextafter(32768.0, 0.0)]
    hi, lo = Q.split_f16(b)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()

    def bound(x):
        return x * F(1, 2 ** 24) + x * (1 + F(1, 2 ** 24)) * F(1, 2 ** 11) + F(1, 2 ** 25)

    for bv, h, l in zip(b.ravel(), hi.ravel(), lo.ravel()):
        exact = F(float(bv))
        assert float(np.float64(bv) - np.float64(h)) == float(exact - F(float(h)))  # (the subtraction is exact)
        assert abs(exact - F(float(h)) - F(float(l))) <= bound(bound(abs(exact)))
    # the two roundings of a tie: 1 + 2^-11 lies half way between two float16 values and goes to the even one
    assert float(hi[0, 3]) == 1.0 and float(lo[0, 3]) == 2.0 ** -11
    assert float(hi[0, 4]) == 1.0 + 2.0 ** -9 and float(lo[0, 4]) == -(2.0 ** -11)
    assert float(hi[0, 1]) == 0.0 and float(lo[0, 1]) == 0.0  # 2^-25: a tie between 0 and the smallest subnormal, to even
    assert float(hi[0, 2]) == 2.0 ** -24


def _round_to_f32(x: F) -> np.float32:
    """The float32 nearest to the exact value x, ties to even."""
    c = np.float32(float(x))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    best = min(cands, key=lambda v: (abs(F(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def test_cells_against_exact_fmaf_chains():
    """oracle.cell_assign: z_l is a chain of correctly rounded float32 fmaf (one rounding each, not a float64 product
    rounded twice), the descent is `>=`.  A one-level tree whose split value is exactly a row's z, and one float32 step to
    either side: the row falls right, right and left."""
    from oracle import oracle

    rng = np.random.default_rng(15)
    n, d = 24, 13
    x = rng.standard_normal((n, d)) * 3.0
    axes = rng.standard_normal((1, d)).astype(np.float32)
    centre = rng.standard_normal(d).astype(np.float32)
    for i in range(n):
        z = np.float32(0.0)
        for k in range(d):
            v = _round_to_f32(F(float(np.float32(x[i, k]))) - F(float(centre[k])))
            z = _round_to_f32(F(float(v)) * F(float(axes[0, k])) + F(float(z)))
        for thr, want in ((z, 1), (np.nextafter(z, np.float32(-np.inf)), 1), (np.nextafter(z, np.float32(np.inf)), 0)):
            got = oracle.cell_assign(x[i:i + 1], axes, centre, np.array([thr], dtype=np.float32))
            assert got[0] == want, (i, float(z), float(thr))
    nan_row = np.full((1, d), np.nan)
    assert oracle.cell_assign(nan_row, axes, centre, np.zeros(1, np.float32))[0] == 0  # NaN: the false branch


def test_cells_against_a_float64_classification():
    """Depth 3: equal to the float64 classification on every row that no split value comes near in float32 terms.  The
    float32 chain of d terms differs from the exact sum by at most (d + 2) 2^-24 sum_k (|x_k| + |c_k|) |a_k| (one rounding
    of x, one of the difference, one per fmaf, first order)."""
    rng = np.random.default_rng(16)
    n, d, depth = 48, 13, 3
    x = rng.standard_normal((n, d)) * 2.0
    axes = np.linalg.qr(rng.standard_normal((d, d)))[0][:depth].astype(np.float32)
    centre = (rng.standard_normal(d) * 0.1).astype(np.float32)
    thr = (rng.standard_normal(7) * 0.5).astype(np.float32)
    consts = dict(cell_depth=depth, axes=axes, centre=centre, thr=thr)
    got = Q.cells(x, consts, 50)
    assert (got[n:] == 7).all()
    a64, c64 = axes.astype(np.float64), centre.astype(np.float64)
    z = (x - c64) @ a64.T
    margin = (d + 2) * 2.0 ** -24 * ((np.abs(x) + np.abs(c64)) @ np.abs(a64).T) * 1.01
    checked = 0
    for i in range(n):
        node, clear = 0, True
        for l in range(depth):
            t = float(thr[(1 << l) - 1 + node])
            clear = clear and abs(z[i, l] - t) > margin[i, l]
            node = 2 * node + (1 if z[i, l] >= t else 0)
        if clear:
            checked += 1
            assert got[i] == node, i
    assert checked >= n - 2


def test_check_bucketing_has_teeth():
    cell = np.array([2, 0, 1, 0, 3, 3], dtype=np.uint8)  # 4 live rows, 2 padding rows, depth 2
    perm = np.array([1, 3, 2, 0, 4, 5], dtype=np.int32)
    qnc = np.arange(6, dtype=np.float64)
    Q.check_bucketing(perm, cell, 4, 2, qnc, qnc[perm])
    Q.check_bucketing(np.array([3, 1, 2, 0, 4, 5], dtype=np.int32), cell, 4, 2)  # the order inside a cell is free
    for bad_perm, bad_cell, bad_pos in ((np.array([1, 3, 0, 2, 4, 5]), cell, None),         # cells out of order
                                        (np.array([1, 3, 2, 2, 4, 5]), cell, None),         # not a permutation
                                        (np.array([1, 3, 2, 0, 5, 4]), cell, None),         # padding moved
                                        (perm, np.array([2, 0, 1, 0, 3, 0], np.uint8), None),  # padding row in a wrong cell
                                        (perm, cell, qnc)):                                  # qnc_pos not permuted
        with pytest.raises(AssertionError):
            Q.check_bucketing(np.asarray(bad_perm, dtype=np.int32), bad_cell, 4, 2, qnc, bad_pos)
