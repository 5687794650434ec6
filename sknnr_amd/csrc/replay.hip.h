// replay.hip.h -- neighbour replay: a tile of STORED neighbours (plot ids or row positions, with or without distances, in
// the raster's own narrow types and layout) decoded into the pipeline's full-layout tile -- int64 idx (n, k), float64
// dist (n, k) -- exactly as a search followed by the nodata expansion leaves it, so that every later stage of the host
// pipeline runs unchanged and nothing of the search runs at all.  The contract is stated once in include/sknnr_hip.h
// ("Neighbour replay"); tests/_replay.py restates it in numpy.  The kernels are defined in k_replay.hip only.
//
// Per pixel i, with s[j] its j-th stored value (j < ks) and the leading k <= ks columns in use:
//   s[0] == fill_index                         -> masked   (tested on the stored value, before any lookup; only column 0 decides)
//   else, for j < k:  r[j] = s[j]              (row positions)   or   perm[c] where sorted[c] == s[j]   (ids)
//         any r[j] missing or outside [0, n_ref) -> unknown  (columns >= k are never looked at)
//   masked / unknown pixel -> bad[i] = 1, index -1, distance NaN;  else bad[i] = 0, idx = r (int32 widened exactly),
//   dist = the stored distances (float32 widened exactly; no stored distances: none written)
// Counters per tile: pixels, masked, unknown (pixels, not values).  Integer adds only: they do not depend on the launch
// geometry, on the tile cuts of a stream or on the order in which workgroups arrive.
//
// Bad pixels and the reused reductions.  The predict, summary and plan kernels gather y[idx] and must never see -1, and
// their weights must never see a NaN distance (no search hands them one: the nodata path compacts masked rows away).  This
// header takes the first of the two routes: DECODE TO A VALID ROW, BLANK AFTERWARDS.  With a.provisional the decode gives
// a bad pixel row 0 and distance 0.0 -- values a search can return -- and replay_blank_kernel, one pass behind the
// reduction, writes the final state: -1 indices, NaN distances, NaN in every prediction plane.  The tally, the domain
// and the zonal kernels run behind that pass and drop the pixel by their own rules (negative index, NaN distance, NaN
// prediction).  Without predictions (a.provisional = 0) the decode writes the final state itself and no pass follows.
//
// Form.  A workgroup of kReplayThreads takes kReplayWgPixels consecutive pixels, kReplayThreads at a time, one pixel per
// lane.  Band-first planes are read with unit stride.  Row tiles are read at a stride of ks elements per lane: the 64
// pixels of a wave cover one contiguous stretch of 64 * ks elements and every column pass reads within those lines, so
// each stored byte crosses from L2 once.  For k <= kReplayStageK the decoded values of the 256 pixels are staged in LDS
// and leave as 16-byte stores (the workgroup's stretch of the full-layout tile is contiguous and 16-byte aligned); wider
// rows leave as 8-byte stores, one column at a time.
// Ids.  As domain.hip.h does for its table: a skeleton of the sorted id table -- every replay_stride(m)-th entry, at most
// kReplaySkel of them (8 KB) -- sits in LDS; the lower-bound search takes its first (at most ten) steps there and ends in
// the one stretch the skeleton names, through L2; perm[c] is the row position.
// The three counters live in LDS and are flushed with at most one global add per counter per workgroup
// (global_atomic_add_x2, device scope, no return value).
//
// Built for gfx950 (hipcc -O3), every instantiation with distances: 44 VGPRs, 82 SGPRs, no scratch, 40,976 bytes of LDS
// (8 KB skeleton, 2 x 16 KB staging, 16 bytes of counters) -- the LDS holds the occupancy at 3 waves per SIMD; without
// distances: 36 VGPRs, 74 SGPRs, 24,592 bytes of LDS, 6 waves per SIMD.  replay_blank_kernel: 8 VGPRs, 16 SGPRs, no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace sknnr {

constexpr int kReplayThreads = 256;
constexpr int kReplayWgPixels = 2048;   // pixels a workgroup takes
constexpr int kReplaySkel = 1024;       // most skeleton entries (8 bytes of LDS each)
constexpr int kReplayStageK = 8;        // widest row staged in LDS for 16-byte stores
// words of the per-tile record
constexpr int kReplayRecPixels = 0, kReplayRecMasked = 1, kReplayRecUnknown = 2, kReplayRecWords = 4;
// stored distance types
constexpr int kReplayDistNone = 0, kReplayDistF32 = 1, kReplayDistF64 = 2;

// table entries between two skeleton entries: the smallest stride at which kReplaySkel entries span the table
__host__ __device__ constexpr long replay_stride(long m) { return (m + kReplaySkel - 1) / kReplaySkel; }
__host__ __device__ constexpr long replay_skel_entries(long m) { return m < 1 ? 0 : (m + replay_stride(m) - 1) / replay_stride(m); }
// the instantiation a launch takes: stored index bytes (4 / 8), stored distance type, planes
__host__ __device__ constexpr int replay_instance(int idx_bytes, int dist_kind, bool planes) {
    return (idx_bytes == 8 ? 6 : 0) + 2 * dist_kind + (planes ? 1 : 0);
}

struct ReplayArgs {
    const void* idx;          // stored values: rows (n, ks), or planes j at idx + j * in_stride elements
    const void* dist;         // stored distances in the same layout, or null
    long n;                   // pixels
    int ks, k;                // stored columns, columns in use (1 <= k <= ks)
    long in_stride;           // planes: elements between two planes (>= n)
    long fill_index;          // the stored value that marks a masked pixel
    long n_ref;
    const long* id_sorted;    // ids: the sorted id table (m), else null: the stored values are row positions
    const int* id_perm;       // ids: the row position of every sorted entry
    long m;
    int provisional;          // bad pixels get row 0 / distance 0.0 here and their final state from replay_blank_kernel
    long* out_idx;            // (n, k)
    double* out_dist;         // (n, k), with dist
    uint8_t* bad;             // (n)
    unsigned long long* rec;  // kReplayRecWords
};

struct ReplayBlankArgs {
    const uint8_t* bad;  // (n)
    long n;
    int k, pred_cols;
    long* idx;      // (n, k)
    double* dist;   // (n, k), or null
    double* pred;   // (n, pred_cols), or null
};

#ifdef SKNNR_KERNELS_REPLAY
struct ReplayNoDist {};

template <typename I, typename D, bool PLANES>
__global__ void __launch_bounds__(kReplayThreads) replay_kernel(ReplayArgs a) {
    constexpr bool kDist = !std::is_same_v<D, ReplayNoDist>;
    __shared__ long skel[kReplaySkel];
    __shared__ __attribute__((aligned(16))) long st_idx[kReplayThreads * kReplayStageK];
    __shared__ __attribute__((aligned(16))) double st_dist[kDist ? kReplayThreads * kReplayStageK : 1];
    __shared__ unsigned wg_rec[kReplayRecWords];
    const int tid = threadIdx.x;
    const bool ids = a.id_sorted != nullptr;
    const long stride = replay_stride(a.m);
    const int n_skel = ids ? (int)replay_skel_entries(a.m) : 0;
    for (int j = tid; j < n_skel; j += kReplayThreads) skel[j] = a.id_sorted[(long)j * stride];
    if (tid < kReplayRecWords) wg_rec[tid] = 0u;
    __syncthreads();

    const I* sidx = static_cast<const I*>(a.idx);
    const D* sdist = static_cast<const D*>(a.dist);
    const long p0 = (long)blockIdx.x * kReplayWgPixels;
    const long p1 = p0 + kReplayWgPixels < a.n ? p0 + kReplayWgPixels : a.n;
    const int k = a.k;
    const bool staged = k <= kReplayStageK;
    const double nan = __builtin_nan("");
    unsigned masked = 0, unknown = 0;
    for (long b0 = p0; b0 < p1; b0 += kReplayThreads) {  // (uniform: every lane reaches the barriers)
        const long q = b0 + tid;
        const bool live = q < p1;
        // where the pixel's column j is stored
        const long at0 = PLANES ? q : q * a.ks, step = PLANES ? a.in_stride : 1;
        int state = 0;  // 1 masked, 2 unknown
        if (live) {
            if ((long)sidx[at0] == a.fill_index) state = 1;
            long* oi = staged ? st_idx + tid * k : a.out_idx + q * k;
            for (int j = 0; j < k && state != 1; ++j) {
                const long v = (long)sidx[at0 + j * step];
                long r = v;
                if (ids) {
                    // skeleton entries below v: none -> sorted[0] >= v; else the position lies in ((lo - 1) * stride, lo * stride]
                    int lo = 0, hi = n_skel;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (skel[mid] < v) lo = mid + 1;
                        else hi = mid;
                    }
                    long c = 0;
                    if (lo > 0) {
                        long t0 = (long)(lo - 1) * stride + 1;
                        long t1 = (long)lo * stride < a.m ? (long)lo * stride : a.m;
                        while (t0 < t1) {
                            const long mid = t0 + ((t1 - t0) >> 1);
                            if (a.id_sorted[mid] < v) t0 = mid + 1;
                            else t1 = mid;
                        }
                        c = t0;
                    }
                    r = (c < a.m && a.id_sorted[c] == v) ? (long)a.id_perm[c] : -1;
                }
                if (r < 0 || r >= a.n_ref) state = 2;
                oi[j] = r;
            }
            if constexpr (kDist) {
                double* od = staged ? st_dist + tid * k : a.out_dist + q * k;
                for (int j = 0; j < k; ++j) od[j] = state ? 0.0 : (double)sdist[at0 + j * step];
            }
            if (state) {
                const long bi = a.provisional ? 0 : -1;
                for (int j = 0; j < k; ++j) oi[j] = bi;
                if constexpr (kDist) {
                    double* od = staged ? st_dist + tid * k : a.out_dist + q * k;
                    const double bd = a.provisional ? 0.0 : nan;
                    for (int j = 0; j < k; ++j) od[j] = bd;
                }
            }
            a.bad[q] = state ? 1 : 0;
            masked += state == 1;
            unknown += state == 2;
        }
        if (staged) {
            __syncthreads();
            // the pass's stretch of the full-layout tile: elements [b0 * k, b0 * k + cnt * k), 16-byte aligned at its start
            const long cnt = p1 - b0 < kReplayThreads ? p1 - b0 : kReplayThreads;
            const long e0 = b0 * k;
            const int n_el = (int)(cnt * k), n_pair = n_el >> 1;
            for (int e = tid; e < n_pair; e += kReplayThreads) {
                *reinterpret_cast<longlong2*>(a.out_idx + e0 + 2 * e) = *reinterpret_cast<const longlong2*>(st_idx + 2 * e);
                if constexpr (kDist)
                    *reinterpret_cast<double2*>(a.out_dist + e0 + 2 * e) = *reinterpret_cast<const double2*>(st_dist + 2 * e);
            }
            if ((n_el & 1) && tid == 0) {
                a.out_idx[e0 + n_el - 1] = st_idx[n_el - 1];
                if constexpr (kDist) a.out_dist[e0 + n_el - 1] = st_dist[n_el - 1];
            }
            __syncthreads();
        }
    }
    if (tid == 0) wg_rec[kReplayRecPixels] = (unsigned)(p1 - p0);
    if (masked) atomicAdd(wg_rec + kReplayRecMasked, masked);
    if (unknown) atomicAdd(wg_rec + kReplayRecUnknown, unknown);
    __syncthreads();
    if (tid < kReplayRecWords && wg_rec[tid]) atomicAdd(a.rec + tid, (unsigned long long)wg_rec[tid]);
}

// the final state of the bad pixels of a tile decoded with a.provisional, behind the reduction
__global__ void __launch_bounds__(kReplayThreads) replay_blank_kernel(ReplayBlankArgs a) {
    const long q = (long)blockIdx.x * kReplayThreads + threadIdx.x;
    if (q >= a.n || !a.bad[q]) return;
    const double nan = __builtin_nan("");
    for (int j = 0; j < a.k; ++j) a.idx[q * a.k + j] = -1;
    if (a.dist)
        for (int j = 0; j < a.k; ++j) a.dist[q * a.k + j] = nan;
    if (a.pred)
        for (int j = 0; j < a.pred_cols; ++j) a.pred[q * a.pred_cols + j] = nan;
}
#endif  // SKNNR_KERNELS_REPLAY

}  // namespace sknnr
