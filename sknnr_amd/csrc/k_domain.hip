// k_domain.hip -- kernel translation unit: distance domain of a tile's neighbour distances (domain.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_DOMAIN 1  // this unit defines the kernels of domain.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

long domain_blocks(long n) { return (n + kDomainWgPixels - 1) / kDomainWgPixels; }

hipError_t domain(const DomainArgs& a, hipStream_t st) {
    if (a.n < 0 || a.k < 1 || a.rank0 < 0 || a.rank0 >= a.k || a.m < 1 || a.m > 0x7fffffffL) return hipErrorInvalidValue;
    if (!a.table || !a.acc || !a.rec || (a.n > 0 && !a.dist)) return hipErrorInvalidValue;
    if (a.pred && (a.pred_cols < 1 || !a.has_threshold)) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const long blocks = domain_blocks(a.n);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    domain_kernel<<<dim3((unsigned)blocks), dim3(kDomainThreads), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
