// forest.hip.h -- the query-time forest map of RFNN / GBNN: raw feature rows -> the node id every tree sends them to.
//
// The reference maps query rows through scikit-learn's forests on the host (REF transformers/_tree_node_transformer.py
// transform -> RandomForest*.apply / GradientBoosting*.apply -> Tree._apply_dense, SKL/tree/_tree.pyx:956-995):
//     node = 0;  while left[node] != -1:  node = X32[i, feature[node]] <= threshold[node] ? left[node] : right[node]
// with X32 the rows converted to float32 (apply validates with dtype=np.float32: SKL/ensemble/_forest.py:628-645,
// SKL/ensemble/_gb.py:1085) and threshold a float64 (SKL/tree/_splitter.pyx:456-466 stores f32/2 + f32/2 in double).
// forest_apply_kernel writes those ids as float64, row-major (nq, n_trees) -- the query rows the weighted-Hamming
// kernels (hamming.hip.h, exact_scan_kernel<2>) read -- so nothing downstream changes.
//
// Forest image (built and checked by sknnr_index_set_forest on the host):
//   nodes      int4 per node {threshold' (float32 bits), feature, left, right}; child ids are tree-local, leaves have
//              left = right = -1 (their feature and threshold are never read).  Trees one after another.
//   tree_off   int64 [n_trees]: first node of tree t.
//   tree_depth int32 [n_trees]: longest root-to-leaf path of tree t, in edges.  The host checked that every child id
//              is greater than its parent's and below the tree's node count, and every feature below d_in, so every
//              walk reaches a leaf within tree_depth steps; the device loop is bounded by it as well.
//
// Exactness of the float32 compare.  threshold' = the largest float32 <= threshold (host: round, step down if above).
// x is a float32 and the reference compares (double)x <= threshold exactly.  If x <= threshold, x is a float32 not above
// threshold, so x <= threshold' (threshold' is the largest such); conversely x <= threshold' <= threshold.  Hence
// x <= threshold' (float32 compare) == (double)x <= threshold for every float32 x, +-0 and thresholds beyond the
// float32 range included (threshold' is then +-FLT_MAX or -inf).
//
// Rows: any sknnr_dtype.  Every one converts to float64 exactly, and float64 -> float32 is one round-to-nearest-even:
// numpy's astype(np.float32), which is what apply does.  A finite value whose float32 is infinite (|v| >= 2^128 - 2^103)
// sets status bit 2 (apply raises "... too large for dtype('float32')"); so does infinity in float32 rows (the
// transformer's own validation names the rows' dtype).  NaN sets bit 0, infinity in other rows bit 1.
//
// Geometry: a lane per query row, 256 rows per workgroup.  The rows are staged in LDS as float32 (row stride d_in | 1:
// the walk's reads x[feature] are conflict-free), the lanes walk kFtInter trees at a time (independent load chains), and
// the ids of kFtGroup trees are staged in LDS and written out row by row: kFtGroup consecutive float64 of a row per
// kFtGroup consecutive lanes, instead of one 8-byte store every n_trees x 8 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact.hip.h"

namespace sknnr {

constexpr int kFtRows = 256;   // query rows (lanes) per workgroup
constexpr int kFtGroup = 16;   // trees per output stage (16 float64 of a row: 128-byte stores)
constexpr int kFtInter = 8;    // trees walked side by side per lane (independent node loads in flight)
constexpr int kFtMaxDin = 64;  // d_in staged in LDS (wider rows are read from global memory, through L1)
static_assert(kFtGroup % kFtInter == 0, "whole interleave groups per stage");

struct ForestArgs {
    const void* x;         // (nq, d_in) rows of x_dtype
    int x_dtype;
    long nq;
    int d_in;
    const int4* nodes;
    const long* tree_off;
    const int* tree_depth;
    int n_trees;
    double* out;           // (nq, n_trees) float64 node ids
    int* status;           // non-finite / float32-overflow flags, or null
};

__host__ __device__ constexpr size_t forest_lds_bytes(int d_in) {
    return (size_t)kFtRows * (d_in <= kFtMaxDin ? (d_in | 1) : 0) * sizeof(float) + (size_t)kFtRows * (kFtGroup + 1) * sizeof(int);
}

// v as float32 (one round-to-nearest-even); `bits` collects the status bits of the header (1 NaN, 2 infinity, 4 float32
// overflow: |v| >= 2^128 - 2^103 rounds to infinity, or infinity in float32 rows)
__device__ __forceinline__ float forest_f32(double v, int dt, int& bits) {
    const double m = fabs(v);
    bits |= (v != v ? 1 : 0) | (m == INFINITY && dt != kDtypeF32 ? 2 : 0) |
            (m >= 0x1.ffffffp+127 && (m != INFINITY || dt == kDtypeF32) ? 4 : 0);
    return (float)v;
}

#if defined(SKNNR_KERNELS_FOREST)
__global__ void __launch_bounds__(kFtRows) forest_apply_kernel(ForestArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const bool staged = a.d_in <= kFtMaxDin;
    const int ldx = a.d_in | 1;
    float* xs = (float*)smem_raw;
    int* ids = (int*)(smem_raw + (staged ? (size_t)kFtRows * ldx * sizeof(float) : 0));
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * kFtRows;
    const int rows = (int)(a.nq - q0 < kFtRows ? a.nq - q0 : kFtRows);
    const bool live = tid < rows;
    const void* __restrict__ x = a.x;
    const int dt = a.x_dtype, d_in = a.d_in, n_trees = a.n_trees;
    const int4* __restrict__ nodes = a.nodes;
    const long* __restrict__ tree_off = a.tree_off;
    const int* __restrict__ tree_depth = a.tree_depth;

    // rows -> float32, checked; staged: coalesced reads of the block's contiguous elements
    int bits = 0;
    if (staged) {
        const long e0 = q0 * d_in;
        const int n_el = rows * d_in;
        for (int e = tid; e < n_el; e += kFtRows) {
            const int r = e / d_in, c = e - r * d_in;
            xs[r * ldx + c] = forest_f32(load_as_f64(x, dt, e0 + e), dt, bits);
        }
    } else if (live) {
        for (int c = 0; c < d_in; ++c) (void)forest_f32(load_as_f64(x, dt, (q0 + tid) * d_in + c), dt, bits);
    }
    if (a.status && bits) atomicOr(a.status, bits);
    __syncthreads();

    const float* xrow = xs + tid * ldx;
    const long grow = (q0 + tid) * (long)d_in;
    for (int t0 = 0; t0 < n_trees; t0 += kFtGroup) {
        const int tg = n_trees - t0 < kFtGroup ? n_trees - t0 : kFtGroup;
        if (live) {
            for (int j0 = 0; j0 < tg; j0 += kFtInter) {
                const int4* tn[kFtInter];
                int node[kFtInter];
                int depth = 0;
#pragma unroll
                for (int u = 0; u < kFtInter; ++u) {
                    const int t = t0 + (j0 + u < tg ? j0 + u : tg - 1);  // (a short last group repeats its last tree)
                    tn[u] = nodes + tree_off[t];
                    depth = max(depth, tree_depth[t]);
                    node[u] = 0;
                }
                for (int s = 0; s < depth; ++s) {
                    int4 nd[kFtInter];
#pragma unroll
                    for (int u = 0; u < kFtInter; ++u) nd[u] = tn[u][node[u]];
                    bool any = false;
#pragma unroll
                    for (int u = 0; u < kFtInter; ++u) {
                        if (nd[u].z >= 0) {
                            const float xv = staged ? xrow[nd[u].y] : (float)load_as_f64(x, dt, grow + nd[u].y);
                            node[u] = xv <= __int_as_float(nd[u].x) ? nd[u].z : nd[u].w;
                            any = true;
                        }
                    }
                    if (!any) break;
                }
#pragma unroll
                for (int u = 0; u < kFtInter; ++u)
                    if (j0 + u < tg) ids[tid * (kFtGroup + 1) + j0 + u] = node[u];
            }
        }
        __syncthreads();
        double* out = a.out + q0 * (long)n_trees + t0;
        for (int e = tid; e < rows * tg; e += kFtRows) {
            const int r = e / tg, j = e - r * tg;
            out[(long)r * n_trees + j] = (double)ids[r * (kFtGroup + 1) + j];
        }
        __syncthreads();
    }
}
#endif  // SKNNR_KERNELS_FOREST

}  // namespace sknnr
