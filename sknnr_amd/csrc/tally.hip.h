// tally.hip.h -- neighbour usage: how often every reference row served as j-th neighbour, and the farthest distance it was
// imputed over, tallied from the (n, k) indices / distances a search just wrote.  The contract is stated once in
// include/sknnr_hip.h ("Neighbour usage"); tests/_usage.py restates it in numpy.  The kernels are defined in k_tally.hip only.
//
// tally_kernel adds into accumulators it never zeroes:
//   cnt[r * k + j]  += rows whose j-th entry is r                                   (unsigned 64-bit adds)
//   maxbits[r]       = max(maxbits[r], bits(d)) over every entry (r, d) with d > 0   (unsigned 64-bit max on the bit pattern)
// A distance that is not > 0 (0.0, -0.0, negative, NaN) counts as +0.0, whose pattern is 0: the max of the patterns of
// non-negative, non-NaN doubles is the pattern of their max, and a max with 0 changes nothing, so it is not even issued.
// Integer adds and an integer max commute: the result does not depend on the launch geometry, on the tile cuts of a
// stream or on the order in which workgroups arrive.  An entry < 0 or >= n_ref is never used as an address: it is
// skipped and counted.
//
// Form.  A workgroup of kTallyThreads takes tally_rows_per_wg(k) consecutive rows -- about kTallyWgEntries entries --
// and aggregates them in an LDS open-addressed table of kTallySlots slots keyed by r * k + j (32 bits: the host refuses
// n_ref * k >= 2^32; 0xffffffff marks a free slot).  A slot is claimed by LDS compare-and-swap (after a plain look, which
// spares the hot bins of a coherent raster the swap), counted in by an LDS add and its maximum kept by an LDS 64-bit max.
// The probe sequence is kTallyProbes consecutive slots from a multiplicative hash; an entry that finds none of them free
// or its own goes straight to the global accumulators.  When the rows are done every occupied slot is flushed with one
// global add and, where its maximum is not 0, one global max on maxbits[key / k].  Spatially coherent tiles put most of
// a workgroup's entries on a few keys: the global atomics drop from one (two) per entry to one (two) per distinct key
// and workgroup.  Random queries overflow the table and cost what the plain form costs plus the LDS traffic.
// -DSKNNR_TALLY_PLAIN builds the plain form for comparison: every entry goes to the global accumulators, no table.
//
// Every global write is a vector atomic (global_atomic_add_x2 / global_atomic_umax_x2, device scope, no return value).
// Indices and distances are loaded 16 bytes per lane -- entries 2p and 2p + 1 of the whole array -- when both arrays
// are 16-byte aligned; a workgroup whose range begins or ends on an odd entry takes that one alone.
//
// Each workgroup adds its four counters to a device record once (threads 0 .. 3): entries tallied, entries skipped,
// global atomics issued on the accumulators, entries that found no slot.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sknnr {

constexpr int kTallyThreads = 256;
constexpr int kTallyWgEntries = 8192;  // entries a workgroup takes (whole rows: tally_rows_per_wg)
#ifdef SKNNR_TALLY_PLAIN
constexpr int kTallySlots = 0;
#else
constexpr int kTallySlots = 2048;      // a power of two; 16 bytes of LDS each
#endif
constexpr int kTallySlotBits = 11;
constexpr int kTallyProbes = 4;
constexpr uint32_t kTallyFree = 0xffffffffu;
// words of the device record
constexpr int kTallyRecTallied = 0, kTallyRecSkipped = 1, kTallyRecAtomics = 2, kTallyRecOverflow = 3, kTallyRecWords = 4;

__host__ __device__ constexpr int tally_rows_per_wg(int k) { return k >= kTallyWgEntries ? 1 : kTallyWgEntries / k; }

struct TallyArgs {
    const long* idx;               // (n, k) neighbour indices
    const double* dist;            // (n, k) distances, or null: counts only
    long n;                        // rows
    int k;
    long n_ref;                    // n_ref * k < 2^32
    unsigned long long* cnt;       // (n_ref, k)
    unsigned long long* maxbits;   // (n_ref), or null with dist
    unsigned long long* rec;       // kTallyRecWords
};

// the contract's bit rule: the pattern of d where d > 0, else (0.0, -0.0, negative, NaN) the pattern of +0.0
__host__ __device__ __forceinline__ unsigned long long tally_dist_bits(double d) {
    union { double f; unsigned long long u; } c;
    c.f = d;
    return d > 0.0 ? c.u : 0ull;
}

#ifdef SKNNR_KERNELS_TALLY
struct TallyCounters {
    unsigned tallied = 0, skipped = 0, atomics = 0, overflow = 0;
};

__device__ __forceinline__ void tally_global(const TallyArgs& a, uint32_t key, long r, unsigned long long bits, unsigned add,
                                             TallyCounters& c) {
    atomicAdd(a.cnt + key, (unsigned long long)add);
    ++c.atomics;
    if (bits) {
        atomicMax(a.maxbits + r, bits);
        ++c.atomics;
    }
}

// One entry: `rel` its position among the workgroup's entries (rel % k is its rank), v the index, bits the distance's
// pattern under the bit rule (0 without distances).
__device__ __forceinline__ void tally_entry(const TallyArgs& a, uint32_t* keys, uint32_t* counts, unsigned long long* maxes,
                                            uint32_t rel, long v, unsigned long long bits, TallyCounters& c) {
    if (v < 0 || v >= a.n_ref) {
        ++c.skipped;
        return;
    }
    ++c.tallied;
    const uint32_t key = (uint32_t)v * (uint32_t)a.k + rel % (uint32_t)a.k;
#ifndef SKNNR_TALLY_PLAIN
    uint32_t s = (key * 2654435761u) >> (32 - kTallySlotBits);
    for (int p = 0; p < kTallyProbes; ++p, s = (s + 1) & (kTallySlots - 1)) {
        uint32_t seen = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (seen == kTallyFree) seen = atomicCAS(keys + s, kTallyFree, key);
        if (seen == kTallyFree || seen == key) {
            atomicAdd(counts + s, 1u);
            if (bits) atomicMax(maxes + s, bits);
            return;
        }
    }
    ++c.overflow;
#endif
    tally_global(a, key, v, bits, 1u, c);
}

template <bool WIDE>
__global__ void __launch_bounds__(kTallyThreads) tally_kernel(TallyArgs a) {
    // (one array: the maxima first, for their alignment)
    __shared__ unsigned long long lds[(kTallySlots * 16 + 64) / 8];
    unsigned long long* maxes = lds;
    uint32_t* keys = (uint32_t*)(lds + kTallySlots);
    uint32_t* counts = keys + kTallySlots;
    uint32_t* wg_rec = counts + kTallySlots;  // kTallyRecWords
    const int tid = threadIdx.x;
    for (int s = tid; s < kTallySlots; s += kTallyThreads) {
        maxes[s] = 0ull;
        keys[s] = kTallyFree;
        counts[s] = 0u;
    }
    if (tid < kTallyRecWords) wg_rec[tid] = 0u;
    __syncthreads();

    const long rows = tally_rows_per_wg(a.k);
    const long row0 = (long)blockIdx.x * rows;
    const long row1 = row0 + rows < a.n ? row0 + rows : a.n;
    const long e0 = row0 * a.k, e1 = row1 * a.k;  // the workgroup's entries
    TallyCounters c;
    if (WIDE) {
        // pairs (2p, 2p + 1) of the whole array inside [e0, e1); thread 0 takes an odd first or last entry alone
        const long p0 = (e0 + 1) >> 1, p1 = e1 >> 1;
        for (long p = p0 + tid; p < p1; p += kTallyThreads) {
            const longlong2 v = *reinterpret_cast<const longlong2*>(a.idx + 2 * p);
            unsigned long long b0 = 0ull, b1 = 0ull;
            if (a.dist) {
                const double2 d = *reinterpret_cast<const double2*>(a.dist + 2 * p);
                b0 = tally_dist_bits(d.x);
                b1 = tally_dist_bits(d.y);
            }
            const uint32_t rel = (uint32_t)(2 * p - e0);
            tally_entry(a, keys, counts, maxes, rel, v.x, b0, c);
            tally_entry(a, keys, counts, maxes, rel + 1, v.y, b1, c);
        }
        if (tid == 0 && e0 < e1) {
            if (e0 & 1) tally_entry(a, keys, counts, maxes, 0u, a.idx[e0], a.dist ? tally_dist_bits(a.dist[e0]) : 0ull, c);
            if (e1 & 1)  // (even, so never the odd first entry)
                tally_entry(a, keys, counts, maxes, (uint32_t)(e1 - 1 - e0), a.idx[e1 - 1],
                            a.dist ? tally_dist_bits(a.dist[e1 - 1]) : 0ull, c);
        }
    } else {
        for (long e = e0 + tid; e < e1; e += kTallyThreads)
            tally_entry(a, keys, counts, maxes, (uint32_t)(e - e0), a.idx[e], a.dist ? tally_dist_bits(a.dist[e]) : 0ull, c);
    }
    __syncthreads();
    // flush: one global add per occupied slot, one global max where the slot saw a positive distance
    for (int s = tid; s < kTallySlots; s += kTallyThreads) {
        const uint32_t key = keys[s];
        if (key != kTallyFree) tally_global(a, key, (long)(key / (uint32_t)a.k), maxes[s], counts[s], c);
    }
    if (c.tallied) atomicAdd(wg_rec + kTallyRecTallied, c.tallied);
    if (c.skipped) atomicAdd(wg_rec + kTallyRecSkipped, c.skipped);
    if (c.atomics) atomicAdd(wg_rec + kTallyRecAtomics, c.atomics);
    if (c.overflow) atomicAdd(wg_rec + kTallyRecOverflow, c.overflow);
    __syncthreads();
    if (tid < kTallyRecWords && wg_rec[tid]) atomicAdd(a.rec + tid, (unsigned long long)wg_rec[tid]);
}

// accumulate = 1 on a caller's max_dist: every value through the bit rule before the kernel takes maxima of patterns
__global__ void __launch_bounds__(256) tally_clean_kernel(double* max_dist, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !(max_dist[i] > 0.0)) max_dist[i] = 0.0;
}
#endif  // SKNNR_KERNELS_TALLY

}  // namespace sknnr
