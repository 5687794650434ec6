// bootstrap.hip.h -- bootstrap standard errors per pixel: B replicates of the plots, all reduced from ONE neighbour list of
// kw > k columns (sknnr_bootstrap_from_neighbors).  The kernel is defined in k_bootstrap.hip only.
//
// The contract is stated in include/sknnr_hip.h ("Bootstrap") and restated in numpy in tests/_bootstrap.py; this header
// only says how the device gets those bits.
//
// Shape.  One replicate per lane.  A wave owns `ppw` pixels (1, 2 or 4): each pixel has a segment of seg = 64 / ppw lanes
// and walks the replicates b = pass * seg + lane-of-segment, pass = 0 .. ceil(B / seg) - 1.  Several pixels share a wave
// only when B <= seg (one pass) and their lists fit the wave's LDS slots (ppw * kw <= kBootMaxKw).
//   table   the multiplicities are kept transposed, (n_ref, bpad) bytes with bpad = B rounded up to 64 and the padding
//           zero: the seg multiplicities of neighbour r_j for one pass are seg consecutive bytes -- one coalesced load --
//           and a lane past B reads a zero, so no load needs a bounds test of its own.
//   staging per pixel the kw rows r_j and weights w_j, and per chunk of kBootCols distinct target columns the values
//           y[r_j, col], go to the wave's LDS slots once; every pass reads them back as broadcasts (the addresses are
//           uniform over a segment).  The distinct columns of the plan are worked out on the host (BootstrapArgs::ucols);
//           an entry names its column by its place in that list.
//   walk    kBootUnroll table bytes are loaded ahead of the dependent chain that consumes them (the addresses depend on
//           r_j only, never on what is left to take); a wave-wide vote between the groups ends the walk when no lane has
//           copies left to take.
//   sums    the 64 partials of the contract are the lanes: lane l adds its replicates in pass order, and the fold
//           P[l] += P[l + s], s = seg / 2 .. 1 is a shuffle-down ladder.  With B <= seg < 64 the partials a shorter
//           segment leaves out are +0.0, and no partial can be -0.0 (x - x and +0.0 + -0.0 are +0.0 in round to nearest),
//           so the shorter ladder gives the 64-lane ladder's bits.
//   grid    a workgroup takes groups of kBootWaves * ppw pixels grid-stride (bootstrap_grid caps the grid at a few
//           workgroups per CU) and keeps the two tallies in registers on the way: one integer atomic add per wave and word
//           at the very end.  (One add per pixel group was measured first: 24 ms per 1M-pixel tile whatever B was.  Two
//           million device-scope adds on two addresses in that time are 12 ns each, which fits adds that serialise beyond
//           the XCDs' L2s; that cause is supposed, not isolated -- the change that removed the adds also capped the grid.)
//   fences  the LDS slots are private to a wave, so staging and walks are ordered by a wave-level fence (boot_sync), not a
//           workgroup barrier: the four waves of a workgroup walk lists of different lengths and need not wait for one
//           another.  -DSKNNR_BOOT_WG_BARRIER=1 builds the workgroup barrier instead, for the A/B.
// Every product is rounded before it is added (-ffp-contract=off); the divisions and the square root are IEEE-exact.
//
// A pixel whose list names a row outside [0, n_ref), or that BootstrapArgs::skip flags, is written as NaN with count 0 and
// enters neither tally; in a stream those are the pixels the blanking pass owns (a replayed tile decodes them to row 0
// provisionally, so its flags say which they are).  No access leaves the arrays for any input.
#pragma once
#include <hip/hip_runtime.h>

#include "weights.hip.h"

namespace sknnr {

// sknnr_bootstrap_statistic (include/sknnr_hip.h)
constexpr int kBootSe = 0, kBootMean = 1, kBootBias = 2, kBootCount = 3;
constexpr int kBootStatCount = 4;
constexpr int kBootMaxB = 4096;    // replicates
constexpr int kBootMaxKw = 192;    // columns of the list (the search's own limit); also the LDS slots of a wave
constexpr int kBootMaxOut = 1024;  // entries of a plan
constexpr int kBootCols = 4;       // distinct target columns accumulated per walk
constexpr int kBootUnroll = 8;     // table bytes in flight per lane
constexpr int kBootWaves = 4;      // waves per workgroup
constexpr long kBootMaxGrid = 2048;  // workgroups of a launch: 256 CUs x 4 resident (LDS) x 2

struct BootstrapArgs {
    const double* y;          // (n_ref, t)
    const double* dist;       // (nq, kw), or null (uniform)
    const long* idx;          // (nq, kw)
    const unsigned char* mt;  // (n_ref, bpad) transposed multiplicities, zero padded
    const unsigned char* skip;  // (nq) or null: pixels with a non-zero flag are treated as if their list named no row
    long nq, n_ref;
    int kw, k, t;
    int mode;                 // 0 uniform, 1 distance, 2 a law of weights.hip.h
    int law;
    double p0, p1;
    int B, bpad;
    const int* ucols;         // (n_u) device: the distinct target columns of the plan
    const int* uidx;          // (n_out) device: place of every entry's column in ucols (kBootCount entries: 0)
    const int* codes;         // (n_out) device: its statistic
    int n_u, n_out;
    double* out;              // (nq, n_out)
    unsigned long long* tally;  // (2) device: pixels reduced, valid replicates over them; added to
    int ppw;                  // pixels per wave: bootstrap_ppw(B, kw)
};

// pixels per wave for a table of B replicates and lists of kw columns
__host__ __device__ __forceinline__ int bootstrap_ppw(int B, int kw) {
    if (B <= 16 && 4 * kw <= kBootMaxKw) return 4;
    if (B <= 32 && 2 * kw <= kBootMaxKw) return 2;
    return 1;
}

// LDS of one wave: rows, weights, the d == 0 mask (distance weights) and kBootCols value columns, kBootMaxKw slots each
struct BootstrapWaveLds {
    double w[kBootMaxKw];
    double z[kBootMaxKw];
    double v[kBootCols][kBootMaxKw];
    int r[kBootMaxKw];
};

#ifdef SKNNR_KERNELS_BOOTSTRAP
#ifndef SKNNR_BOOT_WG_BARRIER
#define SKNNR_BOOT_WG_BARRIER 0
#endif
// Orders a wave's LDS writes in front of its own later LDS reads by other lanes (and the reverse): the LDS executes one
// wave's instructions in order, so it is enough that the writes are issued and counted down and that the compiler moves
// nothing across.
__device__ __forceinline__ void boot_sync() {
#if SKNNR_BOOT_WG_BARRIER
    __syncthreads();
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

__device__ __forceinline__ double boot_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// DIST: distance weights (the second accumulator set holds the 0 / 1 mask of d == 0 over the taken columns)
template <bool DIST>
__global__ void __launch_bounds__(64 * kBootWaves) bootstrap_kernel(BootstrapArgs a) {
    __shared__ BootstrapWaveLds lds_all[kBootWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    BootstrapWaveLds& L = lds_all[wave];
    const int ppw = a.ppw, seg = 64 / ppw;
    const int sid = lane / seg, sl = lane - sid * seg;  // the lane's segment and its place in it
    const int slot0 = sid * a.kw;                       // the segment's first LDS slot (ppw * kw <= kBootMaxKw)
    const unsigned long long seg_mask = (seg == 64 ? ~0ull : ((1ull << seg) - 1ull)) << (sid * seg);
    const int kw = a.kw, k = a.k;
    const int n_pass = (a.B + seg - 1) / seg;
    const long per_wg = (long)kBootWaves * ppw;
    const long n_groups = (a.nq + per_wg - 1) / per_wg;
    unsigned long long px_acc = 0ull, mm_acc = 0ull;  // this lane's share of the tallies (segment leaders only)
    for (long g = blockIdx.x; g < n_groups; g += gridDim.x) {  // (uniform over the workgroup, which a workgroup barrier in boot_sync would need)
    const long q = (g * kBootWaves + wave) * ppw + sid;
    const bool live = q < a.nq;  // (a dead segment stages nothing, walks nothing and writes nothing)

    // ---- the pixel's rows and weights -----------------------------------------------------------------------------------
    bool bad_lane = live && a.skip && a.skip[q] != 0;
    if (live) {
        for (int j = sl; j < kw; j += seg) {
            const long r = a.idx[q * kw + j];
            const bool ok = r >= 0 && r < a.n_ref;
            bad_lane |= !ok;
            L.r[slot0 + j] = ok ? (int)r : 0;
            double w = 1.0, z = 0.0;
            if (a.mode != 0) {
                const double d = a.dist[q * kw + j];
                if (DIST) {
                    w = 1.0 / d;
                    z = d == 0.0 ? 1.0 : 0.0;
                } else {
                    w = weight_law_value(a.law, a.p0, a.p1, d);
                }
            }
            L.w[slot0 + j] = w;
            L.z[slot0 + j] = z;
        }
    }
    const bool bad = (__ballot(bad_lane) & seg_mask) != 0ull;

    const int n_chunk = (a.n_u + kBootCols - 1) / kBootCols;
    for (int ch = 0; ch < n_chunk; ++ch) {
        boot_sync();  // (the previous chunk's walks are done with L.v; on the first pass: nothing)
        if (live) {
            for (int j = sl; j < kw; j += seg) {
                const long r = L.r[slot0 + j];  // (written by this very lane above)
#pragma unroll
                for (int c = 0; c < kBootCols; ++c) {
                    const int u = ch * kBootCols + c;
                    L.v[c][slot0 + j] = u < a.n_u ? a.y[r * a.t + a.ucols[u]] : 0.0;
                }
            }
        }
        boot_sync();

        // ---- the point value: one copy of each of the first k columns ---------------------------------------------------
        double p0v[kBootCols];
        bool p0_ok;
        {
            double den = 0.0, denz = 0.0, num[kBootCols], numz[kBootCols];
#pragma unroll
            for (int c = 0; c < kBootCols; ++c) num[c] = numz[c] = 0.0;
            bool anyz = false;
            for (int j = 0; j < k; ++j) {
                const double w = L.w[slot0 + j];
                den = den + w;
#pragma unroll
                for (int c = 0; c < kBootCols; ++c) num[c] = num[c] + w * L.v[c][slot0 + j];
                if (DIST) {
                    const double z = L.z[slot0 + j];
                    anyz |= z != 0.0;
                    denz = denz + z;
#pragma unroll
                    for (int c = 0; c < kBootCols; ++c) numz[c] = numz[c] + z * L.v[c][slot0 + j];
                }
            }
            if (DIST && anyz) {
                den = denz;
#pragma unroll
                for (int c = 0; c < kBootCols; ++c) num[c] = numz[c];
            }
            p0_ok = den > 0.0 && !bad;
#pragma unroll
            for (int c = 0; c < kBootCols; ++c) p0v[c] = num[c] / den;
        }

        // ---- the replicates -----------------------------------------------------------------------------------------------
        double s1[kBootCols], s2[kBootCols];
#pragma unroll
        for (int c = 0; c < kBootCols; ++c) s1[c] = s2[c] = 0.0;
        int m_lane = 0;
        for (int pass = 0; pass < n_pass; ++pass) {
            const int b = pass * seg + sl;  // (< bpad: the table's padding answers for b >= B)
            int left = live && !bad && b < a.B ? k : 0;
            double den = 0.0, denz = 0.0, num[kBootCols], numz[kBootCols];
#pragma unroll
            for (int c = 0; c < kBootCols; ++c) num[c] = numz[c] = 0.0;
            bool anyz = false;
            for (int j0 = 0; j0 < kw && __any(left > 0); j0 += kBootUnroll) {
                int mult[kBootUnroll];
#pragma unroll
                for (int u = 0; u < kBootUnroll; ++u) {
                    const int j = j0 + u;
                    // (a dead segment has no staged rows: its lanes read nothing)
                    mult[u] = j < kw && live ? (int)a.mt[(long)L.r[slot0 + j] * a.bpad + b] : 0;
                }
#pragma unroll
                for (int u = 0; u < kBootUnroll; ++u) {
                    const int j = j0 + u;
                    const int c_j = mult[u] < left ? mult[u] : left;
                    if (c_j > 0) {  // (only taken columns count: j < kw here, mult is 0 behind the list)
                        left -= c_j;
                        const double cd = (double)c_j;
                        const double cw = cd * L.w[slot0 + j];
                        den = den + cw;
#pragma unroll
                        for (int c = 0; c < kBootCols; ++c) num[c] = num[c] + cw * L.v[c][slot0 + j];
                        if (DIST) {
                            const double z = L.z[slot0 + j];
                            const double cz = cd * z;
                            anyz |= z != 0.0;
                            denz = denz + cz;
#pragma unroll
                            for (int c = 0; c < kBootCols; ++c) numz[c] = numz[c] + cz * L.v[c][slot0 + j];
                        }
                    }
                }
            }
            if (DIST && anyz) {
                den = denz;
#pragma unroll
                for (int c = 0; c < kBootCols; ++c) num[c] = numz[c];
            }
            const bool valid = live && !bad && b < a.B && left == 0 && den > 0.0 && p0_ok;
            m_lane += valid ? 1 : 0;
#pragma unroll
            for (int c = 0; c < kBootCols; ++c) {
                const double ab = valid ? num[c] / den - p0v[c] : 0.0;
                s1[c] = s1[c] + ab;
                s2[c] = s2[c] + ab * ab;
            }
        }

        // ---- fold the partials: P[l] += P[l + s], s = seg / 2 .. 1; the segment's lane 0 holds the result --------------------
        for (int s = seg >> 1; s >= 1; s >>= 1) {
#pragma unroll
            for (int c = 0; c < kBootCols; ++c) {
                s1[c] = s1[c] + __shfl_down(s1[c], s, seg);
                s2[c] = s2[c] + __shfl_down(s2[c], s, seg);
            }
            m_lane += __shfl_down(m_lane, s, seg);
        }
        const int m = __shfl(m_lane, 0, seg);
#pragma unroll
        for (int c = 0; c < kBootCols; ++c) {
            s1[c] = __shfl(s1[c], 0, seg);
            s2[c] = __shfl(s2[c], 0, seg);
        }

        // ---- the entries of this chunk's columns ----------------------------------------------------------------------------
        if (live) {
            const double md = (double)m;
            for (int e = sl; e < a.n_out; e += seg) {
                const int code = a.codes[e], u = a.uidx[e];
                if (code == kBootCount) {
                    if (ch == 0) a.out[q * a.n_out + e] = p0_ok ? md : 0.0;
                    continue;
                }
                if (u / kBootCols != ch) continue;
                const int c = u - ch * kBootCols;
                double S1 = s1[0], S2 = s2[0], P0 = p0v[0];
#pragma unroll
                for (int cc = 1; cc < kBootCols; ++cc) {
                    if (c == cc) {
                        S1 = s1[cc];
                        S2 = s2[cc];
                        P0 = p0v[cc];
                    }
                }
                double r;
                if (!p0_ok || m == 0) {
                    r = boot_nan();
                } else if (code == kBootBias) {
                    r = S1 / md;
                } else if (code == kBootMean) {
                    r = P0 + S1 / md;
                } else if (m < 2) {
                    r = boot_nan();
                } else {
                    const double var = (S2 - S1 * (S1 / md)) / (md - 1.0);
                    r = __dsqrt_rn(weight_law_floor(var));
                }
                a.out[q * a.n_out + e] = r;
            }
        }
        // ---- tallies: once per pixel, from the segment's first lane ----------------------------------------------------------
        if (ch == 0 && live && !bad && sl == 0) {
            px_acc += 1ull;
            mm_acc += p0_ok ? (unsigned long long)m : 0ull;
        }
    }
    boot_sync();  // (the next group's staging overwrites the slots this group's walks read)
    }
    for (int s = 32; s >= 1; s >>= 1) {
        px_acc += __shfl_down(px_acc, s, 64);
        mm_acc += __shfl_down(mm_acc, s, 64);
    }
    if (lane == 0 && px_acc) {
        atomicAdd(a.tally, px_acc);
        if (mm_acc) atomicAdd(a.tally + 1, mm_acc);
    }
}
#endif  // SKNNR_KERNELS_BOOTSTRAP

}  // namespace sknnr
