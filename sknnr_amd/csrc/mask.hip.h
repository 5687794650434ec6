// mask.hip.h -- nodata pixels of streamed raster tiles, handled on the device: which rows of a tile are valid, the valid
// rows packed densely for the search, and the search's results spread back over the full tile.
//
// A row is MASKED when any of its columns equals that column's nodata value; the comparison is made on the element
// widened to float64 (exact for every sknnr_dtype), and a NaN nodata value means "NaN in that column".  Everything else
// is VALID.  The search between the compaction and the expansion is the ordinary device-memory call on the packed rows:
// row positions (key 2 of the reorder, REF _base.py:171) therefore count valid rows only, which is what the reference
// returns to a user who drops the nodata pixels first (X[valid]), and no search kernel changes.
//
// Three memory-bound stages, all in blocks of kMaskRows rows (wave64, 4 waves):
//   row_mask_kernel     reads the block's kMaskRows * d_in elements as one flat, coalesced stream at the element's own
//                       width (rows of 7 uint8 are 7 bytes: nothing is assumed about a row's alignment), raises a flag
//                       per masked row in LDS, then writes one uint8 per row (1 = valid) and the block's valid count.
//   mask_scan_kernel    one workgroup: exclusive scan of the block counts (in place) and the tile's n_valid.
//   row_compact_kernel  rank of every valid row = block offset + waves before it (LDS) + lanes before it (ballot and
//                       popcount): stable and deterministic, no atomics.  Writes rank[row] and copies the row's bytes
//                       to position rank, in units of U bytes (the largest power of two up to 16 that divides the row
//                       size and both base addresses), again over the block's flat stream.
//   row_expand_kernel   for every row of the full tile: a valid row takes its k indices, k distances and t predictions
//                       from position rank[row] of the packed results, a masked row the fills (fill_index, NaN, NaN).
//                       Any output may be absent; writes are coalesced over the flat outputs.  valid == nullptr: every
//                       row is masked (the fill alone).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact.hip.h"

namespace sknnr {

constexpr int kMaskRows = 256;       // rows (and lanes) per workgroup of the three stages
constexpr int kMaskScanLanes = 1024; // lanes of the single scan workgroup
constexpr int kMaskLdsCols = 512;    // nodata values staged in LDS (wider rows read them through L1)

struct MaskArgs {
    const void* x;          // (nq, d_in) rows of x_dtype
    int x_dtype;
    long nq;
    int d_in;
    const double* nodata;   // (d_in)
    unsigned char* valid;   // (nq) 1 = valid
    int* blk;               // (ceil(nq / kMaskRows)) valid rows per block
};

struct CompactArgs {
    const void* x;          // (nq, row_bytes) the tile
    void* out;              // the packed rows
    long nq;
    int row_units;          // row bytes / U
    const unsigned char* valid;
    const int* blk_off;     // exclusive scan of the block counts
    int* rank;              // (nq) valid rows before this one
};

struct ExpandArgs {
    long nq;
    int k, t;
    const unsigned char* valid;  // null: every row is masked
    const int* rank;
    const long* c_idx;     // packed results (n_valid, k) / (n_valid, k) / (n_valid, t)
    const double* c_dist;
    const double* c_pred;
    long* idx;             // full outputs; each may be null
    double* dist;
    double* pred;
    long fill_index;
};

__host__ __device__ constexpr long mask_blocks(long nq) { return (nq + kMaskRows - 1) / kMaskRows; }

#if defined(SKNNR_KERNELS_MASK)
__global__ void __launch_bounds__(kMaskRows) row_mask_kernel(MaskArgs a) {
    __shared__ double nd_s[kMaskLdsCols];
    __shared__ int bad_s[kMaskRows];
    __shared__ int wave_s[kMaskRows / 64];
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kMaskRows;
    const int rows = (int)(a.nq - q0 < kMaskRows ? a.nq - q0 : kMaskRows);
    const int d_in = a.d_in, dt = a.x_dtype;
    const bool staged = d_in <= kMaskLdsCols;
    const double* __restrict__ nodata = a.nodata;
    if (staged)
        for (int c = tid; c < d_in; c += kMaskRows) nd_s[c] = nodata[c];
    bad_s[tid] = 0;
    __syncthreads();
    const void* __restrict__ x = a.x;
    const long e0 = q0 * d_in;
    const int n_el = rows * d_in;  // (the host refuses d_in above 2^16)
#pragma unroll 4
    for (int e = tid; e < n_el; e += kMaskRows) {
        const int r = e / d_in, c = e - r * d_in;
        const double v = load_as_f64(x, dt, e0 + e);
        const double nd = staged ? nd_s[c] : nodata[c];
        if (v == nd || (nd != nd && v != v)) bad_s[r] = 1;  // (every writer stores the same value)
    }
    __syncthreads();
    const bool ok = tid < rows && bad_s[tid] == 0;
    if (tid < rows) a.valid[q0 + tid] = ok ? 1 : 0;
    const unsigned long long m = __ballot(ok);
    if ((tid & 63) == 0) wave_s[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kMaskRows / 64; ++w) s += wave_s[w];
        a.blk[blockIdx.x] = s;
    }
}

// one workgroup: blk[i] <- sum of blk[0 .. i - 1], *n_valid <- the total
__global__ void __launch_bounds__(kMaskScanLanes) mask_scan_kernel(int* blk, long n_blk, long* n_valid) {
    __shared__ long part_s[kMaskScanLanes];
    const int tid = threadIdx.x;
    const long per = (n_blk + kMaskScanLanes - 1) / kMaskScanLanes;
    const long b0 = (long)tid * per, b1 = b0 + per < n_blk ? b0 + per : n_blk;
    long s = 0;
    for (long b = b0; b < b1; ++b) s += blk[b];
    part_s[tid] = s;
    __syncthreads();
    // Hillis-Steele inclusive scan of the lanes' sums
    for (int off = 1; off < kMaskScanLanes; off <<= 1) {
        const long v = tid >= off ? part_s[tid - off] : 0;
        __syncthreads();
        part_s[tid] += v;
        __syncthreads();
    }
    long run = part_s[tid] - s;  // exclusive
    for (long b = b0; b < b1; ++b) {
        const int c = blk[b];
        blk[b] = (int)run;
        run += c;
    }
    if (tid == kMaskScanLanes - 1) *n_valid = part_s[tid];
}
#endif  // SKNNR_KERNELS_MASK

// (a template: instantiated in k_mask.hip for U = 1, 2, 4, 8, 16 bytes)
template <typename Unit>
__global__ void __launch_bounds__(kMaskRows) row_compact_kernel(CompactArgs a) {
    __shared__ int dst_s[kMaskRows];
    __shared__ int wave_s[kMaskRows / 64];
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kMaskRows;
    const int rows = (int)(a.nq - q0 < kMaskRows ? a.nq - q0 : kMaskRows);
    const bool ok = tid < rows && a.valid[q0 + tid] != 0;
    const unsigned long long m = __ballot(ok);
    const int lane = tid & 63, wave = tid >> 6;
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_s[wave] = __popcll(m);
    __syncthreads();
    int base = a.blk_off[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wave_s[w];
    const int rank = base + before;
    if (tid < rows) a.rank[q0 + tid] = rank;
    dst_s[tid] = ok ? rank : -1;
    __syncthreads();
    const int ru = a.row_units;
    const Unit* __restrict__ src = (const Unit*)a.x + q0 * ru;
    Unit* __restrict__ out = (Unit*)a.out;
    const int n_un = rows * ru;  // (at most the row's bytes: below 2^19)
#pragma unroll 4
    for (int e = tid; e < n_un; e += kMaskRows) {
        const int r = e / ru, c = e - r * ru;
        const int p = dst_s[r];
        if (p >= 0) out[(long)p * ru + c] = src[e];
    }
}

#if defined(SKNNR_KERNELS_MASK)
__global__ void __launch_bounds__(kMaskRows) row_expand_kernel(ExpandArgs a) {
    __shared__ int src_s[kMaskRows];
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kMaskRows;
    const int rows = (int)(a.nq - q0 < kMaskRows ? a.nq - q0 : kMaskRows);
    src_s[tid] = (a.valid && tid < rows && a.valid[q0 + tid]) ? a.rank[q0 + tid] : -1;
    __syncthreads();
    const int k = a.k, t = a.t;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (a.idx || a.dist) {
        long* __restrict__ idx = a.idx ? a.idx + q0 * k : nullptr;
        double* __restrict__ dist = a.dist ? a.dist + q0 * k : nullptr;
        const int n_el = rows * k;
        for (int e = tid; e < n_el; e += kMaskRows) {
            const int r = e / k, j = e - r * k;
            const int p = src_s[r];
            if (idx) idx[e] = p >= 0 ? a.c_idx[(long)p * k + j] : a.fill_index;
            if (dist) dist[e] = p >= 0 ? a.c_dist[(long)p * k + j] : nan;
        }
    }
    if (a.pred) {
        double* __restrict__ pred = a.pred + q0 * t;
        const int n_el = rows * t;
        for (int e = tid; e < n_el; e += kMaskRows) {
            const int r = e / t, j = e - r * t;
            const int p = src_s[r];
            pred[e] = p >= 0 ? a.c_pred[(long)p * t + j] : nan;
        }
    }
}
#endif  // SKNNR_KERNELS_MASK

}  // namespace sknnr
