// domain.hip.h -- distance domain: where every pixel's r-th neighbour distance falls within a sorted table of
// reference-to-reference distances, as one uint8 percentile per pixel, an exact histogram of those percentiles and a count
// of the pixels beyond a threshold.  The contract is stated once in include/sknnr_hip.h ("Distance domain");
// tests/_domain.py restates it in numpy.  The kernels are defined in k_domain.hip only.
//
// Per pixel i with s = dist[i * k + rank - 1]:
//   NaN s           -> code 255, acc[102] += 1, nothing else
//   otherwise       -> c = #{ j : T[j] < s }, code = (100 * c) / m (64-bit integers), acc[code] += 1,
//                      and with a threshold and s > theta: acc[101] += 1 and, with a prediction tile, its row becomes NaN
// The table holds finite values >= 0 in non-decreasing order (the host refuses anything else), so s <= 0 gives c = 0 and
// s = +inf gives c = m without a special case.  Integer adds only: the accumulators do not depend on the launch geometry,
// on the tile cuts of a stream or on the order in which workgroups arrive.
//
// Form.  A workgroup of kDomainThreads takes kDomainWgPixels consecutive pixels, each lane four neighbouring ones at a
// time, so that their codes leave as one 4-byte store where the code plane is 4-byte aligned.  The workgroup first
// stages a skeleton of the table in LDS -- every domain_stride(m)-th entry, at most kDomainSkel of them (8 KB) -- and
// searches that (ten steps in LDS for a full skeleton); the search ends in the one stretch of the table the skeleton
// names, through L2 (six steps at m = 50,000).  The 103 counters live in LDS and take LDS adds; when the pixels are done
// every non-zero counter is flushed with one global add (global_atomic_add_x2, device scope, no return value), at most
// 103 per workgroup against one or two per pixel.
// -DSKNNR_DOMAIN_PLAIN builds the plain form for comparison: the whole search in the table itself, and one or two global
// adds per pixel; no skeleton, no LDS counters.
//
// The mask writes its NaN with plain 8-byte stores, pred_cols per beyond pixel.  Each workgroup adds its four counters to
// a device record once (threads 0 .. 3): pixels, nodata pixels, global atomics issued on the accumulators, rows blanked.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace sknnr {

constexpr int kDomainThreads = 256;
constexpr int kDomainLanePixels = 4;     // neighbouring pixels a lane takes at a time: one 4-byte store of codes
constexpr int kDomainWgPixels = 4096;    // pixels a workgroup takes
constexpr int kDomainSkel = 1024;        // most skeleton entries (8 bytes of LDS each)
constexpr int kDomainAcc = 103;          // words of the accumulators: codes 0 .. 100, beyond, nodata
constexpr int kDomainAccBeyond = 101, kDomainAccNodata = 102;
constexpr int kDomainNodataCode = 255;
// words of the device record
constexpr int kDomainRecPixels = 0, kDomainRecNodata = 1, kDomainRecAtomics = 2, kDomainRecBlanked = 3, kDomainRecWords = 4;

// table entries between two skeleton entries: the smallest stride at which kDomainSkel entries span the table
__host__ __device__ constexpr long domain_stride(long m) { return (m + kDomainSkel - 1) / kDomainSkel; }
// skeleton entries in use: T[0], T[stride], ... below m
__host__ __device__ constexpr long domain_skel_entries(long m) { return (m + domain_stride(m) - 1) / domain_stride(m); }

struct DomainArgs {
    const double* dist;        // (n, k) distances
    long n;                    // pixels
    int k;
    int rank0;                 // rank - 1: the column of the score
    const double* table;       // (m) on the device: finite, >= 0, non-decreasing
    long m;                    // 1 <= m <= 2^31 - 1
    int has_threshold;
    double threshold;
    uint8_t* codes;            // (n), or null: tallies only
    unsigned long long* acc;   // kDomainAcc
    double* pred;              // (n, pred_cols) prediction tile whose beyond rows become NaN, or null: no mask
    int pred_cols;
    unsigned long long* rec;   // kDomainRecWords
};

// the contract's code of a count c of table entries below the score
__host__ __device__ __forceinline__ int domain_code(long c, long m) { return (int)(((long long)100 * c) / m); }

// #{ j in [lo, hi) : T[j] < s } + lo for a non-decreasing T: the first position in [lo, hi] whose entry is not below s
__host__ __device__ __forceinline__ long domain_lower_bound(const double* T, long lo, long hi, double s) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (T[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the contract on the host (the one-shot entry's checks; tests/_domain.py is the numpy form): the code of one score
inline int domain_code_host(const double* T, long m, double s) {
    if (std::isnan(s)) return kDomainNodataCode;
    return domain_code(domain_lower_bound(T, 0, m, s), m);
}

#ifdef SKNNR_KERNELS_DOMAIN
struct DomainCounters {
    unsigned nodata = 0, atomics = 0, blanked = 0;
};

__global__ void __launch_bounds__(kDomainThreads) domain_kernel(DomainArgs a) {
    __shared__ unsigned wg_rec[kDomainRecWords];
#ifndef SKNNR_DOMAIN_PLAIN
    __shared__ double skel[kDomainSkel];
    __shared__ unsigned bins[kDomainAcc + 1];
#endif
    const int tid = threadIdx.x;
    const long stride = domain_stride(a.m);
    const int n_skel = (int)domain_skel_entries(a.m);
#ifndef SKNNR_DOMAIN_PLAIN
    for (int j = tid; j < n_skel; j += kDomainThreads) skel[j] = a.table[(long)j * stride];
    if (tid <= kDomainAcc) bins[tid] = 0u;
#else
    (void)stride;
    (void)n_skel;
#endif
    if (tid < kDomainRecWords) wg_rec[tid] = 0u;
    __syncthreads();

    const long p0 = (long)blockIdx.x * kDomainWgPixels;
    const long p1 = p0 + kDomainWgPixels < a.n ? p0 + kDomainWgPixels : a.n;
    const bool wide = a.codes && ((uintptr_t)a.codes & 3) == 0;  // (p0 is a multiple of 4)
    DomainCounters c;
    for (long q = p0 + (long)tid * kDomainLanePixels; q < p1; q += (long)kDomainThreads * kDomainLanePixels) {
        const int cnt = p1 - q < kDomainLanePixels ? (int)(p1 - q) : kDomainLanePixels;
        double s[kDomainLanePixels];
#pragma unroll
        for (int u = 0; u < kDomainLanePixels; ++u) s[u] = u < cnt ? a.dist[(q + u) * a.k + a.rank0] : 0.0;
        uint32_t packed = 0u;
#pragma unroll
        for (int u = 0; u < kDomainLanePixels; ++u) {
            if (u >= cnt) break;
            int code;
            if (s[u] != s[u]) {
                code = kDomainNodataCode;
                ++c.nodata;
#ifndef SKNNR_DOMAIN_PLAIN
                atomicAdd(bins + kDomainAccNodata, 1u);
#else
                atomicAdd(a.acc + kDomainAccNodata, 1ull);
                ++c.atomics;
#endif
            } else {
#ifndef SKNNR_DOMAIN_PLAIN
                // skeleton entries below s: none -> T[0] >= s; else the count ends in (T[(cs - 1) * stride], T[cs * stride]]
                int lo = 0, hi = n_skel;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (skel[mid] < s[u]) lo = mid + 1;
                    else hi = mid;
                }
                long cbelow = 0;
                if (lo > 0) {
                    const long t0 = (long)(lo - 1) * stride + 1;
                    const long t1 = (long)lo * stride < a.m ? (long)lo * stride : a.m;
                    cbelow = domain_lower_bound(a.table, t0, t1, s[u]);
                }
#else
                const long cbelow = domain_lower_bound(a.table, 0, a.m, s[u]);
#endif
                code = domain_code(cbelow, a.m);
                const bool beyond = a.has_threshold && s[u] > a.threshold;
#ifndef SKNNR_DOMAIN_PLAIN
                atomicAdd(bins + code, 1u);
                if (beyond) atomicAdd(bins + kDomainAccBeyond, 1u);
#else
                atomicAdd(a.acc + code, 1ull);
                ++c.atomics;
                if (beyond) {
                    atomicAdd(a.acc + kDomainAccBeyond, 1ull);
                    ++c.atomics;
                }
#endif
                if (beyond && a.pred) {
                    double* row = a.pred + (q + u) * a.pred_cols;
                    for (int j = 0; j < a.pred_cols; ++j) row[j] = __builtin_nan("");
                    ++c.blanked;
                }
            }
            packed |= (uint32_t)code << (8 * u);
        }
        if (a.codes) {
            if (wide && cnt == kDomainLanePixels) {
                *reinterpret_cast<uint32_t*>(a.codes + q) = packed;
            } else {
                for (int u = 0; u < cnt; ++u) a.codes[q + u] = (uint8_t)(packed >> (8 * u));
            }
        }
    }
#ifndef SKNNR_DOMAIN_PLAIN
    __syncthreads();
    // flush: one global add per counter that saw a pixel
    if (tid < kDomainAcc && bins[tid]) {
        atomicAdd(a.acc + tid, (unsigned long long)bins[tid]);
        ++c.atomics;
    }
#endif
    if (tid == 0) wg_rec[kDomainRecPixels] = (unsigned)(p1 - p0);
    if (c.nodata) atomicAdd(wg_rec + kDomainRecNodata, c.nodata);
    if (c.atomics) atomicAdd(wg_rec + kDomainRecAtomics, c.atomics);
    if (c.blanked) atomicAdd(wg_rec + kDomainRecBlanked, c.blanked);
    __syncthreads();
    if (tid < kDomainRecWords && wg_rec[tid]) atomicAdd(a.rec + tid, (unsigned long long)wg_rec[tid]);
}
#endif  // SKNNR_KERNELS_DOMAIN

}  // namespace sknnr
