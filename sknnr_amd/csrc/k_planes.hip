// k_planes.hip -- kernel translation unit: band-first tiles <-> packed rows (planes.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_PLANES 1  // this unit defines the kernels of planes.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

namespace {
template <typename E>
hipError_t planes_launch(bool to_rows, const PlanesArgs& a, hipStream_t st) {
    const int chunk = planes_chunk_cols((int)sizeof(E));
    const int widest = a.c < chunk ? a.c : chunk;  // (the widest chunk of the launch sizes every workgroup's tile)
    const size_t lds = (size_t)kPlanesRows * planes_pitch(widest, (int)sizeof(E)) * sizeof(E);
    const dim3 grid((unsigned)planes_blocks(a.n), (unsigned)((a.c + chunk - 1) / chunk)), block(kPlanesRows);
    if (to_rows) planes_to_rows_kernel<E><<<grid, block, lds, st>>>(a);
    else rows_to_planes_kernel<E><<<grid, block, lds, st>>>(a);
    return hipGetLastError();
}
}  // namespace

hipError_t planes_to_rows(const PlanesArgs& a, int elem_bytes, hipStream_t st) {
    if (a.n < 0 || a.c < 1 || a.stride < a.n || !a.src || !a.dst) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    switch (elem_bytes) {
        case 1: return planes_launch<uint8_t>(true, a, st);
        case 2: return planes_launch<uint16_t>(true, a, st);
        case 4: return planes_launch<uint32_t>(true, a, st);
        case 8: return planes_launch<unsigned long long>(true, a, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t rows_to_planes(const PlanesArgs& a, hipStream_t st) {
    if (a.n < 0 || a.c < 1 || a.stride < a.n || !a.src || !a.dst) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    return planes_launch<unsigned long long>(false, a, st);
}

}  // namespace launch
}  // namespace sknnr
