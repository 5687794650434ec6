// k_forest.hip -- kernel translation unit: the query-time forest map (forest.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_FOREST 1  // this unit defines the kernel of forest.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

hipError_t forest_apply(const ForestArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const size_t sh = forest_lds_bytes(a.d_in);
    hipError_t e = hipFuncSetAttribute((const void*)forest_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return e;
    forest_apply_kernel<<<dim3((unsigned)((a.nq + kFtRows - 1) / kFtRows)), dim3(kFtRows), sh, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
