// k_zonal.hip -- kernel translation unit: zonal statistics of a prediction tile (zonal.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_ZONAL 1  // this unit defines the kernels of zonal.hip.h (and sees narrow.hip.h's narrow_one)
#include "launch.hip.h"

namespace sknnr {
namespace launch {

long zonal_blocks(long n, int c) {
    const long pixels = zonal_pixels_per_wg(c);
    return (n + pixels - 1) / pixels;
}

hipError_t zonal(const ZonalArgs& a, int dst_dtype, hipStream_t st) {
    if (a.n < 0 || a.c < 1 || a.n_zones < 1 || (double)a.n_zones * (double)a.c >= 4294967296.0) return hipErrorInvalidValue;
    if (dst_dtype < 2 || dst_dtype > 5) return hipErrorInvalidValue;  // (int16, uint16, uint8, int32)
    if (!a.acc || !a.rec || (a.n > 0 && (!a.v || !a.zones))) return hipErrorInvalidValue;
    if (!a.na.scale != !a.na.offset || a.na.has_fill || a.na.table) return hipErrorInvalidValue;
    if (a.n_classes && (!a.hist || !a.hist_off)) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const long blocks = zonal_blocks(a.n, a.c);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kZonalThreads);
    switch (dst_dtype) {
        case 2: zonal_kernel<int16_t><<<grid, block, 0, st>>>(a); break;
        case 3: zonal_kernel<uint16_t><<<grid, block, 0, st>>>(a); break;
        case 4: zonal_kernel<uint8_t><<<grid, block, 0, st>>>(a); break;
        default: zonal_kernel<int32_t><<<grid, block, 0, st>>>(a); break;
    }
    return hipGetLastError();
}

hipError_t zonal_init(long long* acc, long n_keys, hipStream_t st) {
    if (n_keys < 0 || (n_keys > 0 && !acc)) return hipErrorInvalidValue;
    if (n_keys == 0) return hipSuccess;
    const long blocks = (n_keys * kZonalFields + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    zonal_init_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(acc, n_keys);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
