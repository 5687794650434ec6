// buffer.hip.h -- buffered leave-out: how many rows the masks of a grouped search exclude for every reference row.
//
// Contract (include/sknnr_hip.h, sknnr_index_set_buffer, states it once): row r is excluded for row i when
//   g(i, r) = ((xi - xr)*(xi - xr) + (yi - yr)*(yi - yr)) + (zi - zr)*(zi - zr) <= r2
// on the rows' positions, every operation a separately rounded float64 operation (the library is built with
// -ffp-contract=off), and, with group codes set as well, when codes[r] == codes[i].  excluded[i] counts those rows, row i
// among them.  group_scan_kernel (groups.hip.h) evaluates the same expression on the same operands, so a row has exactly
// n_ref - excluded[i] candidates there.
//
// buffer_count_kernel is an n_ref x n_ref sweep over the (3, n_ref) positions and the codes; it never touches the feature
// rows.  A thread owns one row i (its position and code in registers); the workgroup passes tiles of kCountTile rows r
// through LDS, every lane reading the same r at a time (a broadcast read).  blockIdx.x names the 256 rows, blockIdx.y a
// share of the tiles, taken with stride gridDim.y, so that a small problem still fills the device; the shares meet in one
// integer atomic per row and share on `out`, which the launcher zeroes first.  Integer sums: the result does not depend on
// the order.
#pragma once
#include "groups.hip.h"

namespace sknnr {

struct BufferCountArgs {
    const double* pos;   // (3, n_ref) positions, column-major; nullptr: no buffer
    const int* codes;    // (n_ref) group codes; nullptr: no groups
    double r2;
    long n_ref;
    unsigned long long* out;  // (n_ref) excluded[], zeroed before the launch
};

constexpr int kCountThreads = 256;  // rows of a workgroup, one per thread
constexpr int kCountTile = 512;     // rows r of one LDS tile
constexpr int kCountGridWg = 1024;  // workgroups the launcher aims for when it splits the tiles
// LDS: x[kCountTile] | y | z | code[kCountTile]
constexpr size_t kCountLdsBytes = (size_t)kCountTile * (kPosCols * sizeof(double) + sizeof(int));

struct BufferCountGrid {
    long row_blocks, splits;
};
// blockIdx.y shares: enough to reach kCountGridWg workgroups, never more than there are tiles
__host__ __device__ constexpr BufferCountGrid buffer_count_grid(long n_ref) {
    BufferCountGrid g{};
    g.row_blocks = (n_ref + kCountThreads - 1) / kCountThreads;
    const long tiles = (n_ref + kCountTile - 1) / kCountTile;
    long s = g.row_blocks > 0 ? (kCountGridWg + g.row_blocks - 1) / g.row_blocks : 1;
    s = s < tiles ? s : tiles;
    g.splits = s > 1 ? s : 1;
    return g;
}

#ifdef SKNNR_KERNELS_BUFFER
__global__ void __launch_bounds__(kCountThreads) buffer_count_kernel(BufferCountArgs a) {
    __shared__ double tp[kPosCols][kCountTile];
    __shared__ int tc[kCountTile];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * kCountThreads + tid;
    const long n = a.n_ref;
    const bool live = i < n;
    const bool by_buffer = a.pos != nullptr, by_group = a.codes != nullptr;
    const long ic = live ? i : n - 1;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (by_buffer) {
        px = a.pos[ic];
        py = a.pos[(size_t)n + ic];
        pz = a.pos[2 * (size_t)n + ic];
    }
    const int ci = by_group ? a.codes[ic] : -1;
    const double r2 = a.r2;
    unsigned long long cnt = 0;
    for (long r0 = (long)blockIdx.y * kCountTile; r0 < n; r0 += (long)gridDim.y * kCountTile) {
        const int nt = (int)((n - r0) < kCountTile ? (n - r0) : kCountTile);
        __syncthreads();  // the previous tile is read
        for (int e = tid; e < nt; e += kCountThreads) {
            if (by_buffer) {
                tp[0][e] = a.pos[r0 + e];
                tp[1][e] = a.pos[(size_t)n + r0 + e];
                tp[2][e] = a.pos[2 * (size_t)n + r0 + e];
            }
            tc[e] = by_group ? a.codes[r0 + e] : -2;  // (-2: equal to no row's code, -1 included)
        }
        __syncthreads();
        int c = 0;
        if (by_buffer) {
            for (int e = 0; e < nt; ++e) {
                const double dx = px - tp[0][e], dy = py - tp[1][e], dz = pz - tp[2][e];
                const double g = (dx * dx + dy * dy) + dz * dz;
                c += (g <= r2 || tc[e] == ci) ? 1 : 0;
            }
        } else {
            for (int e = 0; e < nt; ++e) c += tc[e] == ci ? 1 : 0;
        }
        cnt += (unsigned long long)c;
    }
    if (live && cnt) atomicAdd(a.out + i, cnt);
}
#endif  // SKNNR_KERNELS_BUFFER

}  // namespace sknnr
