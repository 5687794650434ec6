// k_summary.hip -- kernel translation unit: per-target neighbour summaries (summary.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_SUMMARY 1  // this unit defines the kernels of summary.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

hipError_t summary(const SummaryArgs& a, hipStream_t st) {
    if (a.nq < 0 || a.nc < 0 || a.nc > a.t || a.k < 1 || a.k > kSummaryMaxK || !a.y || !a.idx || !a.out ||
        (a.nc > 0 && !a.tab) || (a.mode == 1 && !a.dist) || (a.mode == 2 && !a.w))
        return hipErrorInvalidValue;
    const long total = a.nq * a.nc;
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (a.k <= kSummarySmallK) summary_kernel<<<grid, block, 0, st>>>(a);
    else summary_wide_kernel<<<grid, block, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
