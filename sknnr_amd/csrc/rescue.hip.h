// rescue.hip.h -- the rescue re-sweep: rows the finalisers could not certify, answered from the few reference rows under a
// known bound instead of a float64 pass over all of them.
//
// A finaliser that lists a row for the exact scan has usually re-scored kk candidates in float64 and so holds tau, an exact
// upper bound on the row's true kk-th distance; beside the row it files t_resc (exact.hip.h, rescue_threshold), the pre-filter
// value from which on the certificate's own inequality puts a reference row beyond tau.  rescue_kernel sweeps the f16 hi image
// once more for the listed rows only, with that FIXED threshold: the main value of every (row, reference) unit is computed
// exactly as coarse2_kernel computes it (v_mfma_f32_32x32x16_f16, C operand |r'|^2, K-steps ascending -- bit-identical, so the
// error bound of DESIGN.md section 2.1 applies verbatim), and every reference with
//     main < t_resc + margin          (margin = skip_scale * |q'|, the pre-filter's)
// is collected, up to kRescueCap per query.  A row that is not collected has corrected value >= t_resc (the skip guarantee),
// hence float64 distance > tau: it can neither be among the kk nearest nor tie with them.  The collected rows then go through
// finalize_core -- the finalisers' own ranking, certificate (t_min = t_resc), tie test, drop-self, sqrt and reorder -- and its
// outputs overwrite the provisional ones.  What it still does not certify (exact ties at the boundary, more than kRescueCap
// rows under the bound, rows without a threshold) is filed on a second list, the only one the exact scan sees.
//
// No corrections, no lists, no threshold tightening, no hand scheduling: 0.1 % of the bulk launch's arithmetic.
#pragma once
#include "coarse2.hip.h"
#include "exact.hip.h"

namespace sknnr {

constexpr int kRescueCap = 16;    // candidates per listed row = lanes per row of the finish
constexpr int kRescueWaves = 8;   // one workgroup: 32 listed rows; its waves split the reference tiles, then finish 4 rows each
constexpr int kRescueGrid = 512;  // workgroups of the launch (blocks of 32 listed rows are strided over them)
constexpr int kRescueMaxKK = kRescueCap - 4;  // neighbours searched that the 16-lane finish serves

// device words of one call (zeroed at its start)
enum : int {
    kRescueCursor = 0,    // fail-list entries already offered (earlier device chunks of the call)
    kRescueHanded = 1,    // rows on the second list: the exact scan's count
    kRescueNoThr = 2,     // rows without a threshold
    kRescueOverflow = 3,  // rows with more than kRescueCap references under the bound
    kRescueOffered = 4,   // rows offered over the call
    kRescueDone = 5,      // workgroups of the current launch that have finished
    kRescueWords = 8
};

struct RescueArgs {
    FinalizeArgs f;      // the CALL's window (rows, outputs, row_offset of the whole call; fail_base 0); fail_list / fail_count:
                         // the second list and its count; fail_thr null
    const char* rhi;     // coarse2_kernel's image: n_tiles records [hi: KS KiB][|r'|^2: 128 B]
    int n_tiles;
    const int* perm;     // image position -> reference row
    const uint4* qimg;   // query image and |q'|^2 of the current device chunk, by row of the chunk
    const double* qnc;
    int row0;            // call-relative id of the chunk's row 0
    float skip_scale;
    const int* list;     // what the finalisers listed: call-relative rows, their thresholds, the running count
    const float* thr;
    const int* count;
    int* state;          // kRescueWords device words
};

// workgroup LDS: cnt[32] | cand[32][kRescueCap] | the 32 query rows of the finish (finalize_row_bytes apart)
__host__ __device__ constexpr size_t rescue_lds_bytes(int d) { return 32 * 4 + 32 * kRescueCap * 4 + 32 * finalize_row_bytes(d); }

// (4 waves per SIMD = two workgroups per CU: 123 .. 128 VGPRs, 8 bytes of scratch at four K-steps; left to itself the
//  compiler takes 129 .. 157 and one workgroup per CU, and a launch of 257 .. 512 blocks runs two rounds)
template <int KS>
__global__ void __launch_bounds__(kRescueWaves * 64, 4) rescue_kernel(RescueArgs a) {
    constexpr int TB = tile2_bytes(KS);
    constexpr int LPQ = kRescueCap;
    static_assert(kRescueWaves * 64 == 32 * LPQ, "the finish gives every listed row of a block its group of lanes");
    extern __shared__ __attribute__((aligned(16))) char resc_lds[];
    int* cnt = (int*)resc_lds;
    int* cand = cnt + 32;
    char* xrows = (char*)(cand + 32 * kRescueCap);
    const SelectArgs& s = a.f.s;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;

    const int begin = a.state[kRescueCursor], end = *a.count;
    const int n_blocks = (end - begin + 31) / 32;
    for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int item0 = begin + blk * 32;
        __syncthreads();  // the previous block's finish is done with the LDS
        if (tid < 32) cnt[tid] = 0;
        __syncthreads();

        // ---- the sweep: this lane's column is listed row item0 + col, its K half the lane's half --------------------
        {
            const int item = item0 + col;
            const bool on = item < end;
            const float t = on ? a.thr[item] : __builtin_nanf("");
            const bool swept = t == t;
            const int r = swept ? a.list[item] - a.row0 : 0;
            half8 bh[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bh[ks] = __builtin_bit_cast(half8, a.qimg[qimg_index(r, 0, KS, ks, half)]);
            const float margin = a.skip_scale * (float)sqrt(a.qnc[r]) + 1e-30f;
            float loose = swept ? t + margin : __builtin_nanf("");  // (nothing is below NaN)
            auto unit = [&](int tile, const half8 (&ah)[KS], const floatx4 (&c0)[4]) {
                floatx16 acc;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i] = c0[0][i];
                    acc[4 + i] = c0[1][i];
                    acc[8 + i] = c0[2][i];
                    acc[12 + i] = c0[3][i];
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ks], bh[ks], acc, 0, 0, 0);
                bool any = false;
#pragma unroll
                for (int i = 0; i < 16; ++i) any |= acc[i] < loose;
                if (__builtin_amdgcn_ballot_w64(any) == 0) return;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (acc[i] < loose) {
                        const int pos = tile * 32 + acc_row(i, half);
                        const int at = atomicAdd(&cnt[col], 1);
                        if (at < kRescueCap) cand[col * kRescueCap + at] = pos < s.n_ref ? a.perm[pos] : -1;
                        if (at >= kRescueCap) loose = __builtin_nanf("");  // overflowed: the row is the scan's
                    }
                }
            };
            auto load_tile = [&](int tile, half8 (&ah)[KS], floatx4 (&c0)[4]) {
                const char* tb = a.rhi + (size_t)tile * TB;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) ah[ks] = *(const half8*)(tb + ks * 1024 + lane * 16);
                const floatx4* cp = (const floatx4*)(tb + KS * 1024 + half * 64);
#pragma unroll
                for (int i = 0; i < 4; ++i) c0[i] = cp[i];
            };
            // wave w takes tiles w, w + W, ... two per trip (both tiles' loads go out before the first product); a wave
            // whose 32 rows are all skipped or overflowed leaves
            int tile = wave;
            for (int trip = 0; tile < a.n_tiles; tile += 2 * kRescueWaves, ++trip) {
                if ((trip & 7) == 0) {
                    if (loose == loose && cnt[col] > kRescueCap) loose = __builtin_nanf("");
                    if (__builtin_amdgcn_ballot_w64(loose == loose) == 0) break;
                }
                const int tile_b = tile + kRescueWaves;
                half8 ah0[KS], ah1[KS];
                floatx4 c00[4], c01[4];
                load_tile(tile, ah0, c00);
                if (tile_b < a.n_tiles) load_tile(tile_b, ah1, c01);
                unit(tile, ah0, c00);
                if (tile_b < a.n_tiles) unit(tile_b, ah1, c01);
            }
        }
        __syncthreads();

        // ---- the finish: LPQ lanes per listed row on its collected rows, through the finalisers' own core ------------
        {
            const int qi = tid / LPQ, c = tid % LPQ;
            const int item = item0 + qi;
            const bool live = item < end;
            const int it = live ? item : end - 1;  // (keeps the lane for the exchanges; it writes nothing)
            const long q = a.list[it];
            const float t = a.thr[it];
            const int n = cnt[qi];
            double* xrow = (double*)(xrows + (size_t)qi * finalize_row_bytes(s.d));
            for (int e = c; e < s.d; e += LPQ) xrow[e] = s.xq[q * s.d + e];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // (a group lies inside one wave; DS operations of a wave execute in order)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int id = c < (n < kRescueCap ? n : kRescueCap) ? cand[qi * kRescueCap + c] : -1;
            const bool valid = id >= 0;
            const bool overflowed = n > kRescueCap;
            const unsigned long long head = __builtin_amdgcn_ballot_w64(live && c == 0);
            const int n_nothr = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live && c == 0 && !(t == t)));
            const int n_over = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live && c == 0 && overflowed));
            if (lane == 0 && head != 0) {
                if (n_nothr) atomicAdd(a.state + kRescueNoThr, n_nothr);
                if (n_over) atomicAdd(a.state + kRescueOverflow, n_over);
            }
            // every collected row is re-scored (tau_c = +inf); an overflowed row has no bound on what it did not collect
            finalize_core<LPQ, false>(a.f, q, c, live, xrow, id, valid, 0.f, a.qnc[q - a.row0], (double)INFINITY,
                                      overflowed ? (double)__builtin_nanf("") : (double)t);
        }
    }
    // the last workgroup to finish moves the cursor behind what this launch offered (every workgroup has read it by then)
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(a.state + kRescueDone, 1) == (int)gridDim.x - 1) {
            a.state[kRescueCursor] = end;
            a.state[kRescueOffered] += end - begin;
            a.state[kRescueDone] = 0;
        }
    }
}

// End of a call: the running totals of the handle -- rows the finalisers listed, rows the rescue answered.
#ifdef SKNNR_KERNELS_EXACT
__global__ void rescue_account_kernel(const int* __restrict__ listed, const int* __restrict__ state, long long* __restrict__ total) {
    total[0] += *listed;
    total[1] += state[kRescueOffered] - state[kRescueHanded];
}
#endif  // SKNNR_KERNELS_EXACT

}  // namespace sknnr
