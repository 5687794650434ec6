// k_narrow.hip -- kernel translation unit: result tiles to the raster's storage type (narrow.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_NARROW 1  // this unit defines the kernels of narrow.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

namespace {
template <typename S, typename D>
hipError_t narrow_launch(const NarrowArgs& a, bool wide, hipStream_t st) {
    if (a.stride == 0) {
        const long total = a.n * a.c, work = wide ? (total + 3) / 4 : total;
        const long blocks = std::min((work + kNarrowLanes - 1) / kNarrowLanes, kNarrowMaxBlocks);
        if (wide) narrow_rows_wide_kernel<S, D><<<dim3((unsigned)blocks), dim3(kNarrowLanes), 0, st>>>(a);
        else narrow_rows_kernel<S, D><<<dim3((unsigned)blocks), dim3(kNarrowLanes), 0, st>>>(a);
        return hipGetLastError();
    }
    const int chunk = planes_chunk_cols((int)sizeof(S));
    const int widest = a.c < chunk ? a.c : chunk;  // (the widest chunk of the launch sizes every workgroup's tile)
    const size_t lds = (size_t)kPlanesRows * planes_pitch(widest, (int)sizeof(S)) * sizeof(S);
    const dim3 grid((unsigned)planes_blocks(a.n), (unsigned)((a.c + chunk - 1) / chunk)), block(kPlanesRows);
    if (wide) narrow_planes_kernel<S, D, true><<<grid, block, lds, st>>>(a);
    else narrow_planes_kernel<S, D, false><<<grid, block, lds, st>>>(a);
    return hipGetLastError();
}
}  // namespace

int narrow_dst_bytes(int kind, int dst_dtype, bool table) {
    if (kind == kNarrowIndex) return dst_dtype == 5 ? 4 : (dst_dtype == 0 && table ? 8 : 0);  // (int64: lookup only)
    if (kind != kNarrowValue) return 0;
    switch (dst_dtype) {
        case 1: return 4;  // float32
        case 2: return 2;  // int16
        case 3: return 2;  // uint16
        case 4: return 1;  // uint8
        case 5: return 4;  // int32
        default: return 0;
    }
}

hipError_t narrow(const NarrowArgs& a, int kind, int dst_dtype, bool wide, hipStream_t st) {
    if (a.table && kind != kNarrowIndex) return hipErrorInvalidValue;
    const int esz = narrow_dst_bytes(kind, dst_dtype, a.table != nullptr);
    if (!esz || a.n < 0 || a.c < 1 || (a.stride != 0 && a.stride < a.n) || !a.src || !a.dst || !a.scale != !a.offset)
        return hipErrorInvalidValue;
    if (wide && !narrow_wide_ok(a.src, a.dst, esz, a.n, a.c, a.stride)) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    if (kind == kNarrowIndex)
        return dst_dtype == 0 ? narrow_launch<long, long>(a, wide, st) : narrow_launch<long, int32_t>(a, wide, st);
    switch (dst_dtype) {
        case 1: return narrow_launch<double, float>(a, wide, st);
        case 2: return narrow_launch<double, int16_t>(a, wide, st);
        case 3: return narrow_launch<double, uint16_t>(a, wide, st);
        case 4: return narrow_launch<double, uint8_t>(a, wide, st);
        default: return narrow_launch<double, int32_t>(a, wide, st);
    }
}

}  // namespace launch
}  // namespace sknnr
