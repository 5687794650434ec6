// k_weights.hip -- kernel translation unit: distance-weight laws (weights.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_WEIGHTS 1  // this unit defines the kernel of weights.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

hipError_t weight_law(const WeightLawArgs& a, hipStream_t st) {
    if (a.n < 0 || a.law <= kLawNone || a.law >= kLawCount || (a.n > 0 && (!a.dist || !a.w))) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const long blocks = (a.n + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;  // (2^39 elements: no call comes near)
    weight_law_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
