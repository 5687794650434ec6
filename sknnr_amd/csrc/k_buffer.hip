// k_buffer.hip -- kernel translation unit: buffered leave-out (buffer.hip.h, and the buffer instantiations of
// group_scan_kernel in groups.hip.h), behind the launchers of launch.hip.h.
#define SKNNR_KERNELS_BUFFER 1  // this unit defines the kernels of buffer.hip.h
#include <cstdint>

#include "launch.hip.h"

namespace sknnr {
namespace {
template <int FORMULA, int MASK>
hipError_t buffer_scan_f(bool chunked, const GroupScanArgs& a, long blocks, size_t sh, hipStream_t st) {
    auto kern = chunked ? group_scan_kernel<FORMULA, true, MASK> : group_scan_kernel<FORMULA, false, MASK>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return e;
    kern<<<dim3((unsigned)blocks), dim3(kScanWaves * 64), sh, st>>>(a);
    return hipGetLastError();
}
template <int MASK>
hipError_t buffer_scan_m(int formula, bool chunked, const GroupScanArgs& a, long blocks, size_t sh, hipStream_t st) {
    switch (formula) {
        case 0: return buffer_scan_f<0, MASK>(chunked, a, blocks, sh, st);
        case 1: return buffer_scan_f<1, MASK>(chunked, a, blocks, sh, st);
        default: return buffer_scan_f<2, MASK>(chunked, a, blocks, sh, st);
    }
}
}  // namespace

namespace launch {

hipError_t buffer_scan(int mask, int formula, bool chunked, const GroupScanArgs& a, long blocks, size_t lds_bytes,
                       hipStream_t st) {
    if (!a.pos || (mask == kMaskBoth && !a.codes)) return hipErrorInvalidValue;
    if (mask == kMaskBuffer) return buffer_scan_m<kMaskBuffer>(formula, chunked, a, blocks, lds_bytes, st);
    if (mask == kMaskBoth) return buffer_scan_m<kMaskBoth>(formula, chunked, a, blocks, lds_bytes, st);
    return hipErrorInvalidValue;
}

hipError_t buffer_count(const BufferCountArgs& a, hipStream_t st) {
    if (a.n_ref < 1 || !a.out || (!a.pos && !a.codes)) return hipErrorInvalidValue;
    const BufferCountGrid g = buffer_count_grid(a.n_ref);
    if (g.row_blocks > 0x7fffffffL || g.splits > 65535) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.out, 0, (size_t)a.n_ref * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    buffer_count_kernel<<<dim3((unsigned)g.row_blocks, (unsigned)g.splits), dim3(kCountThreads), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
