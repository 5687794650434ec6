// narrow.hip.h -- typed raster outputs: a packed (n, c) float64 or int64 result tile converted on the device to the type
// the raster is stored in, so that only the narrow bytes cross PCIe.  The destination is packed (n, c) rows (stride 0) or
// c planes `stride` elements apart; the plane form IS rows_to_planes_kernel (planes.hip.h) with the conversion between the
// LDS tile and the store, so a typed band-first result takes one pass.
//
// The conversions are the contract (tests/_narrow.py restates them in numpy; every result is compared bit for bit):
//   values -> float32   x = v, or v * scale[j] + offset[j] as TWO float64 roundings (__dmul_rn, __dadd_rn: never an fma);
//                       NaN with a fill gives (float)fill; everything else is the C cast, round to nearest even --
//                       overflow gives +-inf, NaN stays NaN, subnormal results are kept, and without scale / offset no
//                       arithmetic touches the value, so -0.0 keeps its sign.
//   values -> integers  x as above; NaN is tested FIRST and gives fill (0 without one: the host requires a fill wherever
//                       NaN can occur); otherwise rint(x) (half to even), then the clamp to the type's [min, max] (so
//                       +-inf clamp), then the cast.  The clamp does not step around the fill value.
//   indices -> int32    plain narrowing of int64; the host guarantees that every value fits.
//   indices, id table   (NarrowArgs::table: the dataframe ids of the reference rows) v < 0 ? fill_id : table[v] FIRST -- the
//                       sign is tested before the load, on the int64 source value, and without has_fill a negative
//                       passes through as it is -- then the plain narrowing, or none at all: with a table the destination
//                       may be int64 too (lookup only), so that an untyped id output takes the same single pass.  A
//                       non-negative value at or above the table's length is a caller error that no kernel tests for.
//                       The table is read through plain global loads: n_ref int64, a few hundred KB, resident in L2.
//                       tests/_id_table.py restates the lookup.
//
// Access width.  The element path handles one element per lane and is right at any element-aligned address, as the
// kernels of planes.hip.h are.  The wide path has a lane convert 4 consecutive destination elements: packed, two 16-byte
// loads and one store of 4 * sizeof(D) bytes; planes, 4 consecutive pixels of one plane (a wave writes 256 consecutive
// pixels of a plane).  The HOST chooses it from the addresses, the stride and the count (narrow_wide_ok, as compact_unit
// does for the compaction); inside a wide launch the last, incomplete group of 4 goes element by element.
// An int64 destination (id table only) takes the wide path under the same rule with 8-byte elements: 32 bytes per lane,
// which gfx950 writes as two global_store_dwordx4, and a 32-byte aligned destination.
// Offsets into global memory are 64-bit throughout.  LDS of the plane form: 256 rows x 16 columns of 8 bytes at a pitch
// of 17, 34 KiB, as rows_to_planes_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "planes.hip.h"

namespace sknnr {

constexpr int kNarrowValue = 0;  // source kind: float64 values
constexpr int kNarrowIndex = 1;  //              int64 indices
constexpr int kNarrowLanes = 256;
constexpr long kNarrowMaxBlocks = 1L << 20;  // the packed kernels stride over the grid beyond that

struct NarrowArgs {
    const void* src;  // packed (n, c) float64 / int64
    void* dst;
    long n;
    int c;
    long stride;           // 0: packed (n, c) rows; else elements between the starts of two planes (>= n)
    const double* scale;   // (c) each, device memory; both null or both set
    const double* offset;
    int has_fill;
    double fill;  // representable in the destination type (the host checks)
    // index sources only: the id table (device, or null: no lookup) and what a negative index becomes when has_fill
    const long* table;
    long fill_id;
};

// The host's choice of the wide path: every 4-element store must be aligned to its own size.
//   packed: the flat element i of both buffers is element i of the tile, so src must be 16-byte aligned for the two
//           loads, dst 4 * dst_bytes aligned, and there must be one full group;
//   planes: a workgroup starts at a multiple of 256 pixels, so plane j's groups are aligned when dst and the stride are.
inline bool narrow_wide_ok(const void* src, const void* dst, int dst_bytes, long n, int c, long stride) {
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    if (d % (uintptr_t)(4 * dst_bytes)) return false;
    if (stride == 0) return s % 16 == 0 && n * (long)c >= 4;
    return stride % 4 == 0 && n >= 4;
}

#if defined(SKNNR_KERNELS_NARROW) || defined(SKNNR_KERNELS_ZONAL)  // (zonal.hip.h converts with narrow_one too)
extern __shared__ __attribute__((aligned(16))) unsigned long long narrow_lds[];

template <typename D>
struct alignas(4 * sizeof(D)) NarrowQuad {
    D v[4];
};
template <typename S>
struct alignas(16) NarrowPair {
    S v[2];
};

template <typename D>
struct NarrowRange;
template <> struct NarrowRange<int16_t> { static constexpr double lo = -32768.0, hi = 32767.0; };
template <> struct NarrowRange<uint16_t> { static constexpr double lo = 0.0, hi = 65535.0; };
template <> struct NarrowRange<uint8_t> { static constexpr double lo = 0.0, hi = 255.0; };
template <> struct NarrowRange<int32_t> { static constexpr double lo = -2147483648.0, hi = 2147483647.0; };

// one element of column j
template <typename D>
__device__ __forceinline__ D narrow_one(double v, int j, const NarrowArgs& a) {
    double x = v;
    if (a.scale) x = __dadd_rn(__dmul_rn(v, a.scale[j]), a.offset[j]);
    if constexpr (std::is_floating_point<D>::value) {  // float32
        if (a.has_fill && x != x) return (D)a.fill;
        return (D)x;
    } else {
        if (x != x) return a.has_fill ? (D)a.fill : (D)0;
        x = rint(x);
        x = x < NarrowRange<D>::lo ? NarrowRange<D>::lo : (x > NarrowRange<D>::hi ? NarrowRange<D>::hi : x);
        return (D)x;
    }
}
template <typename D>
__device__ __forceinline__ D narrow_one(long v, int, const NarrowArgs& a) {
    if (a.table) v = v < 0 ? (a.has_fill ? a.fill_id : v) : a.table[v];
    return (D)v;
}

// packed rows, one element per lane
template <typename S, typename D>
__global__ void __launch_bounds__(kNarrowLanes) narrow_rows_kernel(NarrowArgs a) {
    const S* __restrict__ src = (const S*)a.src;
    D* __restrict__ dst = (D*)a.dst;
    const long total = a.n * a.c, step = (long)gridDim.x * kNarrowLanes;
    for (long i = (long)blockIdx.x * kNarrowLanes + threadIdx.x; i < total; i += step)
        dst[i] = narrow_one<D>(src[i], a.scale ? (int)(i % a.c) : 0, a);
}

// packed rows, 4 consecutive elements per lane (narrow_wide_ok)
template <typename S, typename D>
__global__ void __launch_bounds__(kNarrowLanes) narrow_rows_wide_kernel(NarrowArgs a) {
    const S* __restrict__ src = (const S*)a.src;
    D* __restrict__ dst = (D*)a.dst;
    const long total = a.n * a.c, groups = (total + 3) / 4, step = (long)gridDim.x * kNarrowLanes;
    for (long g = (long)blockIdx.x * kNarrowLanes + threadIdx.x; g < groups; g += step) {
        const long i = 4 * g;
        int j = a.scale ? (int)(i % a.c) : 0;  // (the column of element i, carried along the group below)
        if (i + 4 <= total) {
            const NarrowPair<S> p0 = *(const NarrowPair<S>*)(src + i), p1 = *(const NarrowPair<S>*)(src + i + 2);
            const S in[4] = {p0.v[0], p0.v[1], p1.v[0], p1.v[1]};
            NarrowQuad<D> q;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                q.v[e] = narrow_one<D>(in[e], j, a);
                if (a.scale && ++j >= a.c) j = 0;
            }
            *(NarrowQuad<D>*)(dst + i) = q;
        } else {
            for (long e = i; e < total; ++e) {
                dst[e] = narrow_one<D>(src[e], j, a);
                if (a.scale && ++j >= a.c) j = 0;
            }
        }
    }
}

// planes: rows_to_planes_kernel with the conversion on the way out of the LDS tile.  WIDE: lane = (plane of a group of
// four, 4 consecutive pixels) -- one wave per plane, 256 pixels; else lane = pixel.
template <typename S, typename D, bool WIDE>
__global__ void __launch_bounds__(kPlanesRows) narrow_planes_kernel(NarrowArgs a) {
    S* tile = (S*)narrow_lds;
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kPlanesRows;
    const int rows = (int)(a.n - q0 < kPlanesRows ? a.n - q0 : kPlanesRows);
    const int chunk = planes_chunk_cols((int)sizeof(S));
    const int cc0 = (int)blockIdx.y * chunk;
    const int cw = a.c - cc0 < chunk ? a.c - cc0 : chunk;
    const int pitch = planes_pitch(cw, (int)sizeof(S));
    const S* __restrict__ src = (const S*)a.src + q0 * a.c + cc0;
    const int n_el = rows * cw;
#pragma unroll 4
    for (int e = tid; e < n_el; e += kPlanesRows) {
        const int r = e / cw, j = e - r * cw;
        tile[r * pitch + j] = src[(long)r * a.c + j];
    }
    __syncthreads();
    D* __restrict__ dst = (D*)a.dst + (long)cc0 * a.stride + q0;
    if constexpr (!WIDE) {
        if (tid < rows) {
#pragma unroll 4
            for (int j = 0; j < cw; ++j) dst[(long)j * a.stride + tid] = narrow_one<D>(tile[tid * pitch + j], cc0 + j, a);
        }
    } else {
        const int r0 = 4 * (tid & 63);
        for (int j = tid >> 6; j < cw; j += kPlanesRows / 64) {
            D* out = dst + (long)j * a.stride + r0;
            if (r0 + 4 <= rows) {
                NarrowQuad<D> q;
#pragma unroll
                for (int e = 0; e < 4; ++e) q.v[e] = narrow_one<D>(tile[(r0 + e) * pitch + j], cc0 + j, a);
                *(NarrowQuad<D>*)out = q;
            } else {
                for (int e = 0; r0 + e < rows; ++e) out[e] = narrow_one<D>(tile[(r0 + e) * pitch + j], cc0 + j, a);
            }
        }
    }
}
#endif  // SKNNR_KERNELS_NARROW || SKNNR_KERNELS_ZONAL

}  // namespace sknnr
