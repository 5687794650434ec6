// weights.hip.h -- distance-weight laws: w[e] = law(dist[e]) over the (nq, k) distances a search just wrote, so that the
// reductions of exact.hip.h / summary.hip.h run their explicit-weights path (mode 2) on a weight array the device made
// itself (sknnr_weight_law, sknnr_index_set_weight_law_params).  The kernel is defined in k_weights.hip only.
//
// The laws (sknnr_amd/weights.py states the same expressions in numpy; d the distance, p0 the law's parameter, p1 unused
// so far), all float64:
//   inverse          1.0 / (p0 + d)
//   inverse squared  1.0 / (p0 + d * d)
//   triangular       max(0.0, 1.0 - d / p0)
//   epanechnikov     u = d / p0;  max(0.0, 1.0 - u * u)
// Exactness: each law is a chain of at most four + - * / on float64, every one of them correctly rounded by the
// hardware as IEEE 754 demands and numpy's loops deliver.  The build's -ffp-contract=off (and no fast-math) keeps every
// product and sum a rounding of its own -- p0 + d * d is never fused into an fma -- and the division is the compiler's
// IEEE-exact one, so the device writes the bits numpy writes.  d * d may overflow to +inf: 1 / inf = 0, and
// 1 - inf = -inf clamps to 0, as in numpy.  The clamp is np.maximum(0.0, x) written out: x where x > 0, NaN where x is
// NaN (numpy propagates it; a search never writes a NaN distance), else +0.0.
//
// The law is a kernel of its own, not a branch of the reductions: predict_kernel's register budget is priced in
// exact.hip.h (eight more VGPRs cost 19 %), and with w in hand the explicit path already is numpy's reduction.  One
// thread per element, consecutive lanes on consecutive elements: both the load and the store are coalesced, and the
// element index is 64-bit.
#pragma once
#include <hip/hip_runtime.h>

namespace sknnr {

// sknnr_weight_law (include/sknnr_hip.h)
constexpr int kLawNone = 0, kLawInverse = 1, kLawInverseSquared = 2, kLawTriangular = 3, kLawEpanechnikov = 4;
constexpr int kLawCount = 5;

struct WeightLawArgs {
    const double* dist;  // (n) distances
    double* w;           // (n) weights
    long n;              // nq * k elements
    int law;             // kLawInverse .. kLawEpanechnikov
    double p0, p1;       // the law's parameters
};

// np.maximum(0.0, x)
__host__ __device__ __forceinline__ double weight_law_floor(double x) { return x > 0.0 ? x : (x != x ? x : 0.0); }

// One element.  Host code calls it too (the stand-alone check of the four laws against numpy's values).
__host__ __device__ __forceinline__ double weight_law_value(int law, double p0, double p1, double d) {
    (void)p1;
    switch (law) {
        case kLawInverse:
            return 1.0 / (p0 + d);
        case kLawInverseSquared:
            return 1.0 / (p0 + d * d);
        case kLawTriangular:
            return weight_law_floor(1.0 - d / p0);
        default: {  // kLawEpanechnikov
            const double u = d / p0;
            return weight_law_floor(1.0 - u * u);
        }
    }
}

#ifdef SKNNR_KERNELS_WEIGHTS
__global__ void __launch_bounds__(256) weight_law_kernel(WeightLawArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    a.w[e] = weight_law_value(a.law, a.p0, a.p1, a.dist[e]);
}
#endif

}  // namespace sknnr
