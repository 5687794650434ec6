// k_mask.hip -- kernel translation unit: nodata masking, compaction and expansion (mask.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_MASK 1  // this unit defines the kernels of mask.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

hipError_t row_mask(const MaskArgs& a, long* n_valid, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const long nb = mask_blocks(a.nq);
    row_mask_kernel<<<dim3((unsigned)nb), dim3(kMaskRows), 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    mask_scan_kernel<<<dim3(1), dim3(kMaskScanLanes), 0, st>>>(a.blk, nb, n_valid);
    return hipGetLastError();
}

int compact_unit(const void* x, const void* out, size_t row_bytes) {
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)out | (uintptr_t)row_bytes | 16u;
    return (int)(bits & (~bits + 1));  // lowest set bit: 1, 2, 4, 8 or 16
}

hipError_t row_compact(const CompactArgs& a0, size_t row_bytes, hipStream_t st) {
    if (a0.nq <= 0) return hipSuccess;
    CompactArgs a = a0;
    const int unit = compact_unit(a.x, a.out, row_bytes);
    a.row_units = (int)(row_bytes / unit);
    const dim3 grid((unsigned)mask_blocks(a.nq)), block(kMaskRows);
    switch (unit) {
        case 16: row_compact_kernel<uint4><<<grid, block, 0, st>>>(a); break;
        case 8: row_compact_kernel<uint2><<<grid, block, 0, st>>>(a); break;
        case 4: row_compact_kernel<uint32_t><<<grid, block, 0, st>>>(a); break;
        case 2: row_compact_kernel<uint16_t><<<grid, block, 0, st>>>(a); break;
        default: row_compact_kernel<uint8_t><<<grid, block, 0, st>>>(a); break;
    }
    return hipGetLastError();
}

hipError_t row_expand(const ExpandArgs& a, hipStream_t st) {
    if (a.nq <= 0 || (!a.idx && !a.dist && !a.pred)) return hipSuccess;
    // every output that is asked for needs packed results to expand from (unless every row is masked)
    if (a.valid && (!a.rank || (a.idx && !a.c_idx) || (a.dist && !a.c_dist) || (a.pred && !a.c_pred))) return hipErrorInvalidValue;
    row_expand_kernel<<<dim3((unsigned)mask_blocks(a.nq)), dim3(kMaskRows), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
