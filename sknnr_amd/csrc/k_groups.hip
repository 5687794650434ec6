// k_groups.hip -- kernel translation unit: the leave-group-out scan (groups.hip.h), behind the launcher of launch.hip.h.
#include <cstdint>

#include "launch.hip.h"

namespace sknnr {
namespace {
template <int FORMULA>
hipError_t group_scan_f(bool chunked, const GroupScanArgs& a, long blocks, size_t sh, hipStream_t st) {
    auto kern = chunked ? group_scan_kernel<FORMULA, true> : group_scan_kernel<FORMULA, false>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return e;
    kern<<<dim3((unsigned)blocks), dim3(kScanWaves * 64), sh, st>>>(a);
    return hipGetLastError();
}
}  // namespace

namespace launch {

hipError_t group_scan(int formula, bool chunked, const GroupScanArgs& a, long blocks, size_t lds_bytes, hipStream_t st) {
    switch (formula) {
        case 0: return group_scan_f<0>(chunked, a, blocks, lds_bytes, st);
        case 1: return group_scan_f<1>(chunked, a, blocks, lds_bytes, st);
        default: return group_scan_f<2>(chunked, a, blocks, lds_bytes, st);
    }
}

}  // namespace launch
}  // namespace sknnr
