// k_bootstrap.hip -- kernel translation unit: bootstrap standard errors per pixel (bootstrap.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_BOOTSTRAP 1  // this unit defines the kernel of bootstrap.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

long bootstrap_blocks(long n, int ppw) {
    const long per_wg = (long)kBootWaves * ppw;
    return std::min((n + per_wg - 1) / per_wg, kBootMaxGrid);
}

hipError_t bootstrap(const BootstrapArgs& a, hipStream_t st) {
    if (a.nq < 0 || a.n_ref < 1 || a.t < 1 || a.B < 1 || a.B > kBootMaxB || a.k < 1 || a.k > a.kw || a.kw > kBootMaxKw ||
        a.n_out < 1 || a.n_out > kBootMaxOut || a.n_u < 1 || a.n_u > a.n_out || a.mode < 0 || a.mode > 2 ||
        (a.mode == 2 && (a.law <= kLawNone || a.law >= kLawCount)) || (a.mode != 0 && !a.dist) || !a.y || !a.idx || !a.mt ||
        !a.ucols || !a.uidx || !a.codes || !a.out || !a.tally || a.bpad < a.B || (a.bpad & 63) ||
        a.ppw != bootstrap_ppw(a.B, a.kw))
        return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    const long blocks = bootstrap_blocks(a.nq, a.ppw);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(64 * kBootWaves);
    if (a.mode == 1) bootstrap_kernel<true><<<grid, block, 0, st>>>(a);
    else bootstrap_kernel<false><<<grid, block, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
