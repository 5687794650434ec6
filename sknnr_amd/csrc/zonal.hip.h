// zonal.hip.h -- zonal statistics of a prediction tile: per zone and column the count, sum, sum of squares, minimum and
// maximum of the STORED integer values of a typed output, and per zone the class counts of class planes, tallied from the
// (n, c) float64 tile a reduction just wrote and the (n) zone codes beside it.  The contract is stated once in
// include/sknnr_hip.h ("Zonal statistics"); tests/_zonal.py restates it in numpy.  The kernels are defined in k_zonal.hip only.
//
// zonal_kernel<D> adds into accumulators it never initialises (zonal_init_kernel does):
//   acc[(z * c + j) * 6 + 0 .. 5]  count, sum q, sum (q^2 mod 2^32), sum (q^2 >> 32), min q, max q     (int64)
//   hist[hist_off[j] + z * n_classes[j] + q] += 1   for every column j with n_classes[j] > 0 and 0 <= q < n_classes[j]
// where q = narrow_one<D>(v[i, j], j) -- the very device function the narrow kernels store with (narrow.hip.h), without a
// fill -- of every entry that is not NaN, in every pixel whose zone code lies in [0, n_zones).  Integer adds, a signed
// 64-bit min and max: the result does not depend on the launch geometry, on the tile cuts of a stream or on the order in
// which workgroups arrive.  A zone code outside [0, n_zones) is never used as an address: the pixel is skipped and counted.
//
// Form (tally.hip.h's, measured in DESIGN section 17).  A workgroup of kZonalThreads takes zonal_pixels_per_wg(c)
// consecutive pixels -- about kZonalWgEntries entries, a lane per (pixel, column) entry, loaded coalesced -- and
// aggregates them in an LDS open-addressed table of kZonalSlots slots keyed by z * c + j (32 bits: the host refuses
// n_zones * c >= 2^32; 0xffffffff marks a free slot).  A slot is claimed by LDS compare-and-swap after a plain look and
// holds the six partial accumulators: 32-bit count, min and max, 64-bit sum and the two limbs of the sum of squares -- a
// workgroup's partial sums need the limbs too (8,192 squares of 2^62 do not fit 64 bits; 8,192 limbs below 2^32 do).  Class
// values go to a second table of kZonalHistSlots slots keyed by (j << 32) | (z * n_classes[j] + q), claimed by a 64-bit
// LDS compare-and-swap.  The probe sequence is kZonalProbes consecutive slots from a multiplicative hash; an entry that
// finds none of them free or its own goes straight to the global accumulators.  When the pixels are done every occupied
// slot is flushed with one global atomic per accumulator (the high limb only where it is not 0).  Raster zones are
// spatially coherent: a workgroup's entries fall on a few keys, and the global atomics drop from five per entry to five
// per distinct key and workgroup.  -DSKNNR_ZONAL_PLAIN builds the plain form: every entry to the global accumulators.
//
// Every global write is a vector atomic without return value (global_atomic_add_x2 / smin_x2 / smax_x2, device scope).
// Each workgroup adds its six counters to a device record once: entries tallied, NaN entries, pixels outside the zones,
// class values outside their range, global atomics issued on the accumulators, entries that found no slot.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "narrow.hip.h"

namespace sknnr {

constexpr int kZonalThreads = 256;
constexpr int kZonalWgEntries = 8192;  // entries a workgroup takes (whole pixels: zonal_pixels_per_wg)
#ifdef SKNNR_ZONAL_PLAIN
constexpr int kZonalSlots = 0;
constexpr int kZonalHistSlots = 0;
#else
constexpr int kZonalSlots = 1024;      // powers of two; 40 bytes of LDS each
constexpr int kZonalHistSlots = 1024;  //                12 bytes each
#endif
constexpr int kZonalSlotBits = 10;
constexpr int kZonalHistSlotBits = 10;
constexpr int kZonalProbes = 4;
constexpr uint32_t kZonalFree = 0xffffffffu;
constexpr unsigned long long kZonalHistFree = ~0ull;
constexpr int kZonalFields = 6;  // count, sum, sq_lo, sq_hi, min, max
constexpr int kZonalCount = 0, kZonalSum = 1, kZonalSqLo = 2, kZonalSqHi = 3, kZonalMin = 4, kZonalMax = 5;
// words of the device record
constexpr int kZonalRecTallied = 0, kZonalRecNan = 1, kZonalRecOutside = 2, kZonalRecOther = 3, kZonalRecAtomics = 4,
              kZonalRecOverflow = 5, kZonalRecWords = 6;

__host__ __device__ constexpr int zonal_pixels_per_wg(int c) { return c >= kZonalWgEntries ? 1 : kZonalWgEntries / c; }

struct ZonalArgs {
    const double* v;        // (n, c) float64 values
    const int* zones;       // (n) zone codes
    long n;                 // pixels
    int c;
    int n_zones;            // n_zones * c < 2^32
    NarrowArgs na;          // the conversion: scale / offset (device, (c) each, or null); no fill, no table
    const int* n_classes;   // (c) device, or null: no class planes; n_zones * n_classes[j] < 2^32
    const long* hist_off;   // (c) device: where column j's block begins in hist (elements); with n_classes
    long long* acc;         // (n_zones, c, 6)
    long long* hist;        // the blocks, or null with n_classes
    unsigned long long* rec;  // kZonalRecWords
};

#ifdef SKNNR_KERNELS_ZONAL
struct ZonalCounters {
    unsigned tallied = 0, nan = 0, outside = 0, other = 0, atomics = 0, overflow = 0;
};

// the LDS tables of one workgroup
struct ZonalTables {
    unsigned long long *sum, *sq_lo, *sq_hi, *hkeys;
    uint32_t *keys, *counts, *hcounts;
    int *mins, *maxs;
};

// `count` values of one key into the global accumulators: sum and the limbs as 64-bit patterns (two's complement adds)
__device__ __forceinline__ void zonal_global(const ZonalArgs& a, uint32_t key, unsigned count, unsigned long long sum,
                                             unsigned long long lo, unsigned long long hi, long long mn, long long mx,
                                             ZonalCounters& c) {
    unsigned long long* p = (unsigned long long*)(a.acc + (size_t)key * kZonalFields);
    atomicAdd(p + kZonalCount, (unsigned long long)count);
    atomicAdd(p + kZonalSum, sum);
    atomicAdd(p + kZonalSqLo, lo);
    c.atomics += 5;
    if (hi) {
        atomicAdd(p + kZonalSqHi, hi);
        ++c.atomics;
    }
    atomicMin((long long*)p + kZonalMin, mn);
    atomicMax((long long*)p + kZonalMax, mx);
}

__device__ __forceinline__ void zonal_hist_global(const ZonalArgs& a, int j, uint32_t low, unsigned count, ZonalCounters& c) {
    atomicAdd((unsigned long long*)(a.hist + a.hist_off[j]) + low, (unsigned long long)count);
    ++c.atomics;
}

// One entry: column j of a pixel of zone z (the caller has tested the zone), value v.
template <typename D>
__device__ __forceinline__ void zonal_entry(const ZonalArgs& a, const ZonalTables& t, int z, int j, double v,
                                            ZonalCounters& c) {
    if (v != v) {  // NaN first, whatever fill the lane has: a nodata pixel
        ++c.nan;
        return;
    }
    ++c.tallied;
    const long long q = (long long)narrow_one<D>(v, j, a.na);
    const unsigned long long sq = (unsigned long long)(q * q);  // (|q| <= 2^31: below 2^63)
    const unsigned long long lo = sq & 0xffffffffull, hi = sq >> 32;
    const uint32_t key = (uint32_t)z * (uint32_t)a.c + (uint32_t)j;
    bool placed = false;
#ifndef SKNNR_ZONAL_PLAIN
    uint32_t s = (key * 2654435761u) >> (32 - kZonalSlotBits);
    for (int p = 0; p < kZonalProbes; ++p, s = (s + 1) & (kZonalSlots - 1)) {
        uint32_t seen = __hip_atomic_load(t.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (seen == kZonalFree) seen = atomicCAS(t.keys + s, kZonalFree, key);
        if (seen == kZonalFree || seen == key) {
            atomicAdd(t.counts + s, 1u);
            atomicAdd(t.sum + s, (unsigned long long)q);
            atomicAdd(t.sq_lo + s, lo);
            if (hi) atomicAdd(t.sq_hi + s, hi);
            atomicMin(t.mins + s, (int)q);
            atomicMax(t.maxs + s, (int)q);
            placed = true;
            break;
        }
    }
    if (!placed) ++c.overflow;
#endif
    if (!placed) zonal_global(a, key, 1u, (unsigned long long)q, lo, hi, q, q, c);
    const int ncls = a.n_classes ? a.n_classes[j] : 0;
    if (ncls <= 0) return;
    if (q < 0 || q >= ncls) {
        ++c.other;
        return;
    }
    const uint32_t low = (uint32_t)z * (uint32_t)ncls + (uint32_t)q;
#ifndef SKNNR_ZONAL_PLAIN
    const unsigned long long hkey = ((unsigned long long)(uint32_t)j << 32) | low;
    uint32_t h = ((low + (uint32_t)j * 0x9e3779b9u) * 2654435761u) >> (32 - kZonalHistSlotBits);
    for (int p = 0; p < kZonalProbes; ++p, h = (h + 1) & (kZonalHistSlots - 1)) {
        unsigned long long seen = __hip_atomic_load(t.hkeys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (seen == kZonalHistFree) seen = atomicCAS(t.hkeys + h, kZonalHistFree, hkey);
        if (seen == kZonalHistFree || seen == hkey) {
            atomicAdd(t.hcounts + h, 1u);
            return;
        }
    }
    ++c.overflow;
#endif
    zonal_hist_global(a, j, low, 1u, c);
}

template <typename D>
__global__ void __launch_bounds__(kZonalThreads) zonal_kernel(ZonalArgs a) {
    // (one array: the 64-bit words first, for their alignment)
    __shared__ unsigned long long lds[(kZonalSlots * 40 + kZonalHistSlots * 12 + 64) / 8];
    ZonalTables t;
    t.sum = lds;
    t.sq_lo = t.sum + kZonalSlots;
    t.sq_hi = t.sq_lo + kZonalSlots;
    t.hkeys = t.sq_hi + kZonalSlots;
    t.keys = (uint32_t*)(t.hkeys + kZonalHistSlots);
    t.counts = t.keys + kZonalSlots;
    t.mins = (int*)(t.counts + kZonalSlots);
    t.maxs = t.mins + kZonalSlots;
    t.hcounts = (uint32_t*)(t.maxs + kZonalSlots);
    uint32_t* wg_rec = t.hcounts + kZonalHistSlots;  // kZonalRecWords
    const int tid = threadIdx.x;
    for (int s = tid; s < kZonalSlots; s += kZonalThreads) {
        t.sum[s] = t.sq_lo[s] = t.sq_hi[s] = 0ull;
        t.keys[s] = kZonalFree;
        t.counts[s] = 0u;
        t.mins[s] = 0x7fffffff;
        t.maxs[s] = (int)0x80000000;
    }
    for (int s = tid; s < kZonalHistSlots; s += kZonalThreads) {
        t.hkeys[s] = kZonalHistFree;
        t.hcounts[s] = 0u;
    }
    if (tid < kZonalRecWords) wg_rec[tid] = 0u;
    __syncthreads();

    const long pixels = zonal_pixels_per_wg(a.c);
    const long pix0 = (long)blockIdx.x * pixels;
    const long pix1 = pix0 + pixels < a.n ? pix0 + pixels : a.n;
    const uint32_t n_el = (uint32_t)((pix1 - pix0) * a.c);  // the workgroup's entries (at most max(c, kZonalWgEntries))
    const double* __restrict__ v = a.v + pix0 * a.c;
    const int* __restrict__ zones = a.zones + pix0;
    ZonalCounters c;
    for (uint32_t e = tid; e < n_el; e += kZonalThreads) {
        const uint32_t pix = e / (uint32_t)a.c;
        const int j = (int)(e - pix * (uint32_t)a.c);
        const int z = zones[pix];
        if (z < 0 || z >= a.n_zones) {
            if (j == 0) ++c.outside;
            continue;
        }
        zonal_entry<D>(a, t, z, j, v[e], c);
    }
    __syncthreads();
    // flush: every occupied slot, one global atomic per accumulator
    for (int s = tid; s < kZonalSlots; s += kZonalThreads) {
        const uint32_t key = t.keys[s];
        if (key != kZonalFree) zonal_global(a, key, t.counts[s], t.sum[s], t.sq_lo[s], t.sq_hi[s], t.mins[s], t.maxs[s], c);
    }
    for (int s = tid; s < kZonalHistSlots; s += kZonalThreads) {
        const unsigned long long hkey = t.hkeys[s];
        if (hkey != kZonalHistFree) zonal_hist_global(a, (int)(hkey >> 32), (uint32_t)hkey, t.hcounts[s], c);
    }
    if (c.tallied) atomicAdd(wg_rec + kZonalRecTallied, c.tallied);
    if (c.nan) atomicAdd(wg_rec + kZonalRecNan, c.nan);
    if (c.outside) atomicAdd(wg_rec + kZonalRecOutside, c.outside);
    if (c.other) atomicAdd(wg_rec + kZonalRecOther, c.other);
    if (c.atomics) atomicAdd(wg_rec + kZonalRecAtomics, c.atomics);
    if (c.overflow) atomicAdd(wg_rec + kZonalRecOverflow, c.overflow);
    __syncthreads();
    if (tid < kZonalRecWords && wg_rec[tid]) atomicAdd(a.rec + tid, (unsigned long long)wg_rec[tid]);
}

// accumulate = 0: count, sum and the limbs 0, min INT64_MAX, max INT64_MIN for every (zone, column)
__global__ void __launch_bounds__(256) zonal_init_kernel(long long* acc, long n_keys) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_keys * kZonalFields) return;
    const int f = (int)(i % kZonalFields);
    acc[i] = f == kZonalMin ? 0x7fffffffffffffffLL : (f == kZonalMax ? (long long)0x8000000000000000ull : 0LL);
}
#endif  // SKNNR_KERNELS_ZONAL

}  // namespace sknnr
