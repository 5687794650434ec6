// summary.hip.h -- per-target neighbour summaries: one statistic per target column, reduced from the (dist, idx) a search
// just wrote (sknnr_summarize*, sknnr_stream_set_statistics).  Kernels are defined in k_summary.hip only.
//
// The `mean` columns stay with the predict kernels of exact.hip.h; the kernels here answer the other columns, given as a
// compact device table: tab[0 .. nc) the target columns, tab[nc .. 2 nc) their sknnr_statistic codes.  One thread per
// (query, listed column).  Definitions (all float64; v_i = y[idx_i, j], w_i the weights predict uses; np_sum = numpy's
// pairwise sum over the k axis, exact.hip.h):
//   mode     sklearn.utils.extmath.weighted_mode as KNeighborsClassifier.predict applies it: per distinct label c the vote
//            np_sum_i(v_i == c ? w_i : 0.0); the largest vote wins, the smaller label on equal votes; all votes zero: NaN
//   min/max  of v_i (weights ignored)
//   nearest  v_0
//   std      sqrt(np_sum_i((w_i * (v_i - m)) * (v_i - m)) / np_sum_i(w_i)), m = the float64 mean predict gives that column
//            (uniform weights and t >= 2: the k values added in order, as np.mean on (nq, k, t) does)
// The build's -ffp-contract=off keeps every product and sum a rounding of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "exact.hip.h"

namespace sknnr {

// sknnr_statistic (include/sknnr_hip.h)
constexpr int kStatMean = 0, kStatMode = 1, kStatMin = 2, kStatMax = 3, kStatNearest = 4, kStatStd = 5;
constexpr int kStatCount = 6;
constexpr int kSummaryMaxK = 192;  // the largest k a search gives (the host unit's kScanMaxKK); np_sum's single split holds
constexpr int kSummarySmallK = 8;  // summary_kernel holds this many neighbours in registers; above it summary_wide_kernel

struct SummaryArgs {
    const double* y;     // (n_ref, t)
    const double* dist;  // (nq, k) or null (uniform)
    const long* idx;     // (nq, k)
    const double* w;     // (nq, k) explicit weights or null
    long nq;
    int k;               // at most kSummaryMaxK
    int t;
    int mode;            // 0 uniform, 1 distance, 2 explicit (as PredictArgs)
    const int* tab;      // (2 nc) device table: columns, then codes; no code is kStatMean
    int nc;
    double* out;         // (nq, t): only the listed columns are written
};

// One candidate label against the running winner: strict > on the vote, the smaller label on equal votes.  The start
// (vote 0, label NaN) leaves NaN where every vote is zero: no label is smaller than NaN.
__device__ __forceinline__ void summary_vote(double vote, double label, double& best_vote, double& best_label) {
    if (vote > best_vote || (vote == best_vote && label < best_label)) {
        best_vote = vote;
        best_label = label;
    }
}

// ---- the statistics' bodies, shared by the kernels below and by plan_kernel / plan_wide_kernel (plan.hip.h) ---------------
// k <= kSummarySmallK: the query's indices, then target column tt's values and the raw weights (1, the given weight, or the
// DISTANCE: summary_small_weights turns it into predict's weight), requested before the first use and held in registers
// (as predict_kernel).  Slots i >= k repeat neighbour 0's value and hold a neutral weight.
__device__ __forceinline__ void summary_small_load(const double* y, const long* ids, const double* dd, const double* ww,
                                                   int k, int t, int mode, int tt, double (&yv)[8], double (&wv)[8]) {
    long id[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) id[i] = i < k ? ids[i] : ids[0];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        yv[i] = y[id[i] * t + tt];
        wv[i] = mode == 0 ? 1.0 : (mode == 2 ? (i < k ? ww[i] : 0.0) : (i < k ? dd[i] : 1.0));
    }
}
// distance weights: 1/d, or the row's 0/1 mask where it holds d == 0 (other modes: nothing changes)
__device__ __forceinline__ void summary_small_weights(int k, int mode, double (&wv)[8]) {
    if (mode == 1) {
        bool any_zero = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) any_zero |= (i < k) && (wv[i] == 0.0);
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = any_zero ? (wv[i] == 0.0 ? 1.0 : 0.0) : 1.0 / wv[i];
    }
}
// one of the five statistics (code != kStatMean) from the registers summary_small_load filled
__device__ __forceinline__ double summary_small_stat(int code, int k, int t, int mode, const double (&yv)[8],
                                                     double (&wv)[8]) {
    if (code == kStatNearest) return yv[0];
    if (code == kStatMin || code == kStatMax) {
        double r = yv[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (i < k) r = code == kStatMin ? (yv[i] < r ? yv[i] : r) : (yv[i] > r ? yv[i] : r);
        return r;
    }
    summary_small_weights(k, mode, wv);
    if (code == kStatMode) {
        double best_vote = 0.0, best_label = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bool first = i < k;  // one vote per first occurrence of a label
#pragma unroll
            for (int j = 0; j < i; ++j) first &= !(yv[j] == yv[i]);
            if (first) {
                double tv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) tv[j] = (j < k && yv[j] == yv[i]) ? wv[j] : 0.0;
                summary_vote(np_sum_small(k, tv), yv[i], best_vote, best_label);
            }
        }
        return best_label;
    }
    // kStatStd
    double m;
    if (mode == 0 && t > 1) {
        double acc = yv[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (i < k) acc = acc + yv[i];
        m = acc / (double)k;
    } else {
        double nv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) nv[i] = yv[i] * wv[i];
        m = np_sum_small(k, nv) / np_sum_small(k, wv);
    }
    double sv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double dv = yv[i] - m;
        sv[i] = (wv[i] * dv) * dv;
    }
    return sqrt(np_sum_small(k, sv) / np_sum_small(k, wv));
}

// k up to kSummaryMaxK: a query's labels of column tt and its weights, re-read from L2 on every use (the query's k
// indices and the target values they point at were fetched by this very thread a moment ago).
struct SummaryRow {
    const double* y;
    const long* ids;
    const double* dd;
    const double* ww;
    int k, t, mode, tt;
    bool any_zero;  // distance weights: the row holds d == 0 (summary_row_zero)
    __device__ __forceinline__ double label(int i) const { return y[ids[i] * t + tt]; }
    __device__ __forceinline__ double weight(int i) const {
        if (mode == 0) return 1.0;
        if (mode == 2) return ww[i];
        if (any_zero) return dd[i] == 0.0 ? 1.0 : 0.0;
        return 1.0 / dd[i];
    }
};
__device__ __forceinline__ bool summary_row_zero(const SummaryRow& r) {
    bool any_zero = false;
    if (r.mode == 1)
        for (int i = 0; i < r.k; ++i) any_zero |= (r.dd[i] == 0.0);
    return any_zero;
}
// one of the five statistics (code != kStatMean); `mode` votes once per first occurrence of a label
__device__ __forceinline__ double summary_wide_stat(int code, SummaryRow& r) {
    const int k = r.k;
    if (code == kStatNearest) return r.label(0);
    if (code == kStatMin || code == kStatMax) {
        double m = r.label(0);
        for (int i = 1; i < k; ++i) {
            const double v = r.label(i);
            m = code == kStatMin ? (v < m ? v : m) : (v > m ? v : m);
        }
        return m;
    }
    r.any_zero = summary_row_zero(r);
    if (code == kStatMode) {
        double best_vote = 0.0, best_label = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = 0; i < k; ++i) {
            const double ci = r.label(i);
            bool first = true;
            for (int j = 0; j < i && first; ++j) first = !(r.label(j) == ci);
            if (!first) continue;
            const double vote = np_sum<double>(k, [&](int j) { return r.label(j) == ci ? r.weight(j) : 0.0; });
            summary_vote(vote, ci, best_vote, best_label);
        }
        return best_label;
    }
    // kStatStd
    const double den = np_sum<double>(k, [&](int i) { return r.weight(i); });
    double m;
    if (r.mode == 0 && r.t > 1) {
        double acc = r.label(0);
        for (int i = 1; i < k; ++i) acc = acc + r.label(i);
        m = acc / (double)k;
    } else {
        m = np_sum<double>(k, [&](int i) { return r.label(i) * r.weight(i); }) / den;
    }
    const double ss = np_sum<double>(k, [&](int i) {
        const double dv = r.label(i) - m;
        return (r.weight(i) * dv) * dv;
    });
    return sqrt(ss / den);
}

#ifdef SKNNR_KERNELS_SUMMARY
// k <= 8: summary_small_load, then summary_small_stat on the registers.
__global__ void __launch_bounds__(256) summary_kernel(SummaryArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nq * a.nc) return;
    const long q = e / a.nc;
    const int c = (int)(e - q * a.nc);
    const int tt = a.tab[c], code = a.tab[a.nc + c];
    double yv[8], wv[8];
    summary_small_load(a.y, a.idx + q * a.k, a.dist ? a.dist + q * a.k : nullptr, a.w ? a.w + q * a.k : nullptr, a.k, a.t,
                       a.mode, tt, yv, wv);
    a.out[q * a.t + tt] = summary_small_stat(code, a.k, a.t, a.mode, yv, wv);
}

// k up to kSummaryMaxK: summary_wide_stat on the row.
__global__ void __launch_bounds__(256) summary_wide_kernel(SummaryArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nq * a.nc) return;
    const long q = e / a.nc;
    const int c = (int)(e - q * a.nc);
    const int tt = a.tab[c], code = a.tab[a.nc + c];
    SummaryRow r{a.y, a.idx + q * a.k, a.dist ? a.dist + q * a.k : nullptr, a.w ? a.w + q * a.k : nullptr, a.k, a.t, a.mode,
                 tt, false};
    a.out[q * a.t + tt] = summary_wide_stat(code, r);
}
#endif  // SKNNR_KERNELS_SUMMARY

}  // namespace sknnr
