// k_plan.hip -- kernel translation unit: output plans (plan.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_PLAN 1  // this unit defines the kernels of plan.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

hipError_t plan(const PlanArgs& a, hipStream_t st) {
    if (a.nq < 0 || a.n_out < 1 || a.n_out > kPlanMaxOut || a.t < 1 || a.k < 1 || a.k > kSummaryMaxK || !a.y || !a.idx ||
        !a.out || !a.cols || !a.codes || !a.param || (a.mode == 1 && !a.dist) || (a.mode == 2 && !a.w))
        return hipErrorInvalidValue;
    const long total = a.nq * a.n_out;
    if (total == 0) return hipSuccess;
    if ((total + 255) / 256 > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (a.k <= kSummarySmallK) plan_kernel<<<grid, block, 0, st>>>(a);
    else plan_wide_kernel<<<grid, block, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
