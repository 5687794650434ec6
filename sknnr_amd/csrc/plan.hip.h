// plan.hip.h -- output plans: n_out planes per query, each one statistic of one target column, reduced from the (dist, idx) a
// search just wrote (sknnr_summarize_plan*, sknnr_stream_set_plan).  Kernels are defined in k_plan.hip only.
//
// A plan is three device arrays of n_out entries: the target column (it may repeat, in any order), the sknnr_statistic
// code, and a float64 parameter (the quantile's q; 0 otherwise).  One thread per (query, entry); a query's entries sit on
// neighbouring lanes, so its gathers y[idx_i * t + j] hit the same few lines.  out is (nq, n_out).
//
// The six statistics of summary.hip.h keep their definitions and their code: `mean` is copied from the (nq, t) staging
// buffer the unchanged predict kernels filled (PlanArgs::mean), the other five are summary_small_stat / summary_wide_stat.
// New here:
//   quantile  numpy's weighted inverted_cdf, np.quantile(v, q, method="inverted_cdf", weights=w):
//             1. order the k pairs (v_i, w_i) by (v_i, i) ascending (a stable sort by value; -0.0 == 0.0)
//             2. c_0 = w_(0), c_a = c_(a-1) + w_(a): a sequential float64 running sum in sorted order; total = c_(k-1)
//             3. cdf_a = c_a / total, one division each
//             4. the result is v_(a*), a* the first a with cdf_a != 0.0 and cdf_a >= q, or k - 1 when there is none
//             5. total not > 0: NaN (as `mean` gives there)
//             w_i are the weights predict uses (summary.hip.h).  A NaN among the values leaves the result unspecified.
// k <= kSummarySmallK sorts the 8 register-held (value, position, weight) triples with a fixed 19-comparator network
// (slots i >= k hold +inf at position i and weight 0: they sort last and add nothing); above it the sorted order is walked
// by repeated selection -- the next element is the smallest (v, i) above the last one taken -- once for the total and once
// up to a*: O(k^2) re-reads from L2 per thread, the trade summary_wide_kernel makes for `mode`.
#pragma once
#include <hip/hip_runtime.h>

#include "summary.hip.h"

namespace sknnr {

constexpr int kStatQuantile = 6;
constexpr int kPlanStatCount = 7;
constexpr int kPlanMaxOut = 1024;  // a sanity cap on the prediction lane's width

struct PlanArgs {
    const double* y;     // (n_ref, t)
    const double* dist;  // (nq, k) or null (uniform)
    const long* idx;     // (nq, k)
    const double* w;     // (nq, k) explicit weights or null
    long nq;
    int k;               // at most kSummaryMaxK
    int t;
    int mode;            // 0 uniform, 1 distance, 2 explicit (as PredictArgs)
    const int* cols;     // (n_out) device: target column of every entry
    const int* codes;    // (n_out) device: its statistic
    const double* param; // (n_out) device: its parameter
    int n_out;
    const double* mean;  // (nq, t) the predict kernels' output, read by the kStatMean entries; null: the plan has none
    double* out;         // (nq, n_out)
};

// (v, position) order of two slots: a goes behind b
__device__ __forceinline__ bool plan_after(double va, int pa, double vb, int pb) {
    return va > vb || (va == vb && pa > pb);
}
__device__ __forceinline__ void plan_cx(double& va, int& pa, double& wa, double& vb, int& pb, double& wb) {
    if (plan_after(va, pa, vb, pb)) {
        const double tv = va, tw = wa;
        const int tp = pa;
        va = vb, pa = pb, wa = wb;
        vb = tv, pb = tp, wb = tw;
    }
}

// The quantile of the registers summary_small_load filled; wv already are predict's weights (summary_small_weights).
__device__ __forceinline__ double plan_small_quantile(double q, int k, double (&yv)[8], double (&wv)[8]) {
    int pv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        pv[i] = i;
        if (i >= k) {
            yv[i] = __longlong_as_double(0x7ff0000000000000LL);
            wv[i] = 0.0;
        }
    }
#define SKNNR_PLAN_CX(i, j) plan_cx(yv[i], pv[i], wv[i], yv[j], pv[j], wv[j])
    SKNNR_PLAN_CX(0, 2); SKNNR_PLAN_CX(1, 3); SKNNR_PLAN_CX(4, 6); SKNNR_PLAN_CX(5, 7);
    SKNNR_PLAN_CX(0, 4); SKNNR_PLAN_CX(1, 5); SKNNR_PLAN_CX(2, 6); SKNNR_PLAN_CX(3, 7);
    SKNNR_PLAN_CX(0, 1); SKNNR_PLAN_CX(2, 3); SKNNR_PLAN_CX(4, 5); SKNNR_PLAN_CX(6, 7);
    SKNNR_PLAN_CX(2, 4); SKNNR_PLAN_CX(3, 5);
    SKNNR_PLAN_CX(1, 4); SKNNR_PLAN_CX(3, 6);
    SKNNR_PLAN_CX(1, 2); SKNNR_PLAN_CX(3, 4); SKNNR_PLAN_CX(5, 6);
#undef SKNNR_PLAN_CX
    double c[8];
    c[0] = wv[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) c[i] = c[i - 1] + wv[i];  // (the padded slots add 0.0: c[7] == c[k - 1])
    const double total = c[7];
    double r = yv[0];
    bool found = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < k && !found) {
            const double cdf = c[i] / total;
            r = yv[i];  // (stays at slot k - 1 when no slot qualifies)
            found = cdf != 0.0 && cdf >= q;
        }
    }
    return total > 0.0 ? r : __longlong_as_double(0x7ff8000000000000LL);
}

// The next element of the row in (v, i) order behind (lv, li); false: there is none.
__device__ __forceinline__ bool plan_next(const SummaryRow& r, double& lv, int& li) {
    double bv = 0.0;
    int bi = -1;
    for (int j = 0; j < r.k; ++j) {
        const double v = r.label(j);
        if (!plan_after(v, j, lv, li)) continue;
        if (bi < 0 || plan_after(bv, bi, v, j)) {
            bv = v;
            bi = j;
        }
    }
    if (bi < 0) return false;
    lv = bv;
    li = bi;
    return true;
}
__device__ __forceinline__ double plan_wide_quantile(double q, SummaryRow& r) {
    r.any_zero = summary_row_zero(r);
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    double lv = ninf, total = 0.0;
    int li = -1;
    for (int a = 0; a < r.k && plan_next(r, lv, li); ++a) total = a == 0 ? r.weight(li) : total + r.weight(li);
    if (!(total > 0.0)) return __longlong_as_double(0x7ff8000000000000LL);
    lv = ninf;
    li = -1;
    double c = 0.0;
    for (int a = 0; a < r.k && plan_next(r, lv, li); ++a) {
        c = a == 0 ? r.weight(li) : c + r.weight(li);
        const double cdf = c / total;
        if (cdf != 0.0 && cdf >= q) break;
    }
    return lv;
}

#ifdef SKNNR_KERNELS_PLAN
// k <= 8
__global__ void __launch_bounds__(256) plan_kernel(PlanArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nq * a.n_out) return;
    const long q = e / a.n_out;
    const int c = (int)(e - q * a.n_out);
    const int tt = a.cols[c], code = a.codes[c];
    if (code == kStatMean) {
        a.out[e] = a.mean[q * a.t + tt];
        return;
    }
    double yv[8], wv[8];
    summary_small_load(a.y, a.idx + q * a.k, a.dist ? a.dist + q * a.k : nullptr, a.w ? a.w + q * a.k : nullptr, a.k, a.t,
                       a.mode, tt, yv, wv);
    if (code == kStatQuantile) {
        summary_small_weights(a.k, a.mode, wv);
        a.out[e] = plan_small_quantile(a.param[c], a.k, yv, wv);
        return;
    }
    a.out[e] = summary_small_stat(code, a.k, a.t, a.mode, yv, wv);
}

// k up to kSummaryMaxK
__global__ void __launch_bounds__(256) plan_wide_kernel(PlanArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nq * a.n_out) return;
    const long q = e / a.n_out;
    const int c = (int)(e - q * a.n_out);
    const int tt = a.cols[c], code = a.codes[c];
    if (code == kStatMean) {
        a.out[e] = a.mean[q * a.t + tt];
        return;
    }
    SummaryRow r{a.y, a.idx + q * a.k, a.dist ? a.dist + q * a.k : nullptr, a.w ? a.w + q * a.k : nullptr, a.k, a.t, a.mode,
                 tt, false};
    a.out[e] = code == kStatQuantile ? plan_wide_quantile(a.param[c], r) : summary_wide_stat(code, r);
}
#endif  // SKNNR_KERNELS_PLAN

}  // namespace sknnr
