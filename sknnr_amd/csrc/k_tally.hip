// k_tally.hip -- kernel translation unit: neighbour usage (tally.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_TALLY 1  // this unit defines the kernels of tally.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

bool tally_wide_ok(const TallyArgs& a) { return (((uintptr_t)a.idx | (uintptr_t)a.dist) & 15) == 0; }

long tally_blocks(long n, int k) {
    const long rows = tally_rows_per_wg(k);
    return (n + rows - 1) / rows;
}

hipError_t tally(const TallyArgs& a, hipStream_t st) {
    if (a.n < 0 || a.k < 1 || a.n_ref < 1 || (double)a.n_ref * (double)a.k >= 4294967296.0) return hipErrorInvalidValue;
    if (!a.cnt || !a.rec || !a.dist != !a.maxbits || (a.n > 0 && !a.idx)) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const long blocks = tally_blocks(a.n, a.k);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (tally_wide_ok(a)) tally_kernel<true><<<dim3((unsigned)blocks), dim3(kTallyThreads), 0, st>>>(a);
    else tally_kernel<false><<<dim3((unsigned)blocks), dim3(kTallyThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t tally_clean(double* max_dist, long n, hipStream_t st) {
    if (n < 0 || (n > 0 && !max_dist)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    tally_clean_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(max_dist, n);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
