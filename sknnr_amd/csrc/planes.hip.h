// planes.hip.h -- band-first raster tiles, transposed on the device in both directions: `c` planes of `n` elements (what a
// raster reader delivers and a raster writer wants) <-> packed (n, c) rows (what every search kernel reads and writes).
//
// Both kernels are raw moves of 1-, 2-, 4- or 8-byte elements: nothing is widened and no value is looked at, so NaN
// payloads and -0.0 pass bit for bit.  A workgroup of kPlanesRows lanes takes kPlanesRows consecutive pixels and a chunk
// of at most planes_chunk_cols(esz) columns (blockIdx.y), and goes through an LDS tile of rows x columns:
//   planes_to_rows_kernel  fill: column by column, lane = pixel -- each plane segment is one contiguous, coalesced stream;
//                          drain: the block's rows x columns elements in row-major order, lane = element -- ONE flat
//                          contiguous stream when the chunk covers all columns, contiguous row pieces otherwise.
//   rows_to_planes_kernel  the same two loops with global memory and LDS exchanged.
// Every global access is one element wide, so any element-aligned address is served: rows of 7 uint8 are 7 bytes, plane
// bases and strides may be odd multiples of the element size.  The host makes no choice of a wider unit: measured, a
// 1M x 32 int16 tile takes planes_to_rows 350 us (365 GB/s) and three float64 planes take rows_to_planes 9 us, beside
// 5.8 ms of search (profiles/r10_raster_layout.txt); wider accesses for the narrow types are the open improvement.
//
// LDS: the tile's row pitch is padded (planes_pitch) so that the column-wise side, where a wave's lanes are a pitch apart,
// spreads over the banks (MI355X: 4-byte banks; 32 lanes per group for 4-byte accesses, 16 for 8-byte stores): the pitch
// in dwords is odd for elements up to 4 bytes, the pitch in elements odd for 8-byte ones.  The row-wise side then walks
// the tile contiguously except for one pad per row.  The padding is performance only: pitch = columns is as correct.
// A chunk is 128 bytes of a row, so a workgroup holds at most 256 x 136 = 34 KiB and four or more fit a CU.
// Offsets into global memory are 64-bit throughout: n * c passes 2^31 long before n does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sknnr {

constexpr int kPlanesRows = 256;        // pixels (and lanes) per workgroup
constexpr int kPlanesChunkBytes = 128;  // bytes of a row one workgroup handles

struct PlanesArgs {
    const void* src;
    void* dst;
    long n;       // pixels
    int c;        // columns (planes)
    long stride;  // elements between the starts of two planes (>= n): of src in planes_to_rows, of dst in rows_to_planes
};

__host__ __device__ constexpr int planes_chunk_cols(int elem_bytes) { return kPlanesChunkBytes / elem_bytes; }
// elements between two rows of the LDS tile of a chunk of cw columns
__host__ __device__ constexpr int planes_pitch(int cw, int elem_bytes) {
    return elem_bytes >= 4 ? (cw | 1) : (4 / elem_bytes) * (((cw + 4 / elem_bytes - 1) / (4 / elem_bytes)) | 1);
}
__host__ __device__ constexpr long planes_blocks(long n) { return (n + kPlanesRows - 1) / kPlanesRows; }

#if defined(SKNNR_KERNELS_PLANES)
extern __shared__ unsigned long long planes_lds[];

// (templates: instantiated in k_planes.hip for 1-, 2-, 4- and 8-byte elements)
template <typename E>
__global__ void __launch_bounds__(kPlanesRows) planes_to_rows_kernel(PlanesArgs a) {
    E* tile = (E*)planes_lds;
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kPlanesRows;
    const int rows = (int)(a.n - q0 < kPlanesRows ? a.n - q0 : kPlanesRows);
    const int chunk = planes_chunk_cols((int)sizeof(E));
    const int cc0 = (int)blockIdx.y * chunk;
    const int cw = a.c - cc0 < chunk ? a.c - cc0 : chunk;
    const int pitch = planes_pitch(cw, (int)sizeof(E));
    if (tid < rows) {
        const E* __restrict__ src = (const E*)a.src + (long)cc0 * a.stride + q0 + tid;
#pragma unroll 4
        for (int j = 0; j < cw; ++j) tile[tid * pitch + j] = src[(long)j * a.stride];
    }
    __syncthreads();
    E* __restrict__ dst = (E*)a.dst + q0 * a.c + cc0;
    const int n_el = rows * cw;  // (at most 256 * 128)
#pragma unroll 4
    for (int e = tid; e < n_el; e += kPlanesRows) {
        const int r = e / cw, j = e - r * cw;
        dst[(long)r * a.c + j] = tile[r * pitch + j];
    }
}

template <typename E>
__global__ void __launch_bounds__(kPlanesRows) rows_to_planes_kernel(PlanesArgs a) {
    E* tile = (E*)planes_lds;
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kPlanesRows;
    const int rows = (int)(a.n - q0 < kPlanesRows ? a.n - q0 : kPlanesRows);
    const int chunk = planes_chunk_cols((int)sizeof(E));
    const int cc0 = (int)blockIdx.y * chunk;
    const int cw = a.c - cc0 < chunk ? a.c - cc0 : chunk;
    const int pitch = planes_pitch(cw, (int)sizeof(E));
    const E* __restrict__ src = (const E*)a.src + q0 * a.c + cc0;
    const int n_el = rows * cw;
#pragma unroll 4
    for (int e = tid; e < n_el; e += kPlanesRows) {
        const int r = e / cw, j = e - r * cw;
        tile[r * pitch + j] = src[(long)r * a.c + j];
    }
    __syncthreads();
    if (tid < rows) {
        E* __restrict__ dst = (E*)a.dst + (long)cc0 * a.stride + q0 + tid;
#pragma unroll 4
        for (int j = 0; j < cw; ++j) dst[(long)j * a.stride] = tile[tid * pitch + j];
    }
}
#endif  // SKNNR_KERNELS_PLANES

}  // namespace sknnr
