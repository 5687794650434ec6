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

#ifdef SKNNR_KERNELS_SUMMARY
// k <= 8: indices, then target values and weights, requested before the first use and held in registers (as predict_kernel).
__global__ void __launch_bounds__(256) summary_kernel(SummaryArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nq * a.nc) return;
    const long q = e / a.nc;
    const int c = (int)(e - q * a.nc);
    const int tt = a.tab[c], code = a.tab[a.nc + c];
    const long* ids = a.idx + q * a.k;
    const double* dd = a.dist ? a.dist + q * a.k : nullptr;
    const double* ww = a.w ? a.w + q * a.k : nullptr;
    long id[8];
    double yv[8], wv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) id[i] = i < a.k ? ids[i] : ids[0];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        yv[i] = a.y[id[i] * a.t + tt];
        wv[i] = a.mode == 0 ? 1.0 : (a.mode == 2 ? (i < a.k ? ww[i] : 0.0) : (i < a.k ? dd[i] : 1.0));
    }
    double* out = a.out + q * a.t + tt;
    if (code == kStatNearest) {
        *out = yv[0];
        return;
    }
    if (code == kStatMin || code == kStatMax) {
        double r = yv[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (i < a.k) r = code == kStatMin ? (yv[i] < r ? yv[i] : r) : (yv[i] > r ? yv[i] : r);
        *out = r;
        return;
    }
    if (a.mode == 1) {
        bool any_zero = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) any_zero |= (i < a.k) && (wv[i] == 0.0);
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = any_zero ? (wv[i] == 0.0 ? 1.0 : 0.0) : 1.0 / wv[i];
    }
    if (code == kStatMode) {
        double best_vote = 0.0, best_label = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bool first = i < a.k;  // one vote per first occurrence of a label
#pragma unroll
            for (int j = 0; j < i; ++j) first &= !(yv[j] == yv[i]);
            if (first) {
                double tv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) tv[j] = (j < a.k && yv[j] == yv[i]) ? wv[j] : 0.0;
                summary_vote(np_sum_small(a.k, tv), yv[i], best_vote, best_label);
            }
        }
        *out = best_label;
        return;
    }
    // kStatStd
    double m;
    if (a.mode == 0 && a.t > 1) {
        double acc = yv[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (i < a.k) acc = acc + yv[i];
        m = acc / (double)a.k;
    } else {
        double nv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) nv[i] = yv[i] * wv[i];
        m = np_sum_small(a.k, nv) / np_sum_small(a.k, wv);
    }
    double sv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double dv = yv[i] - m;
        sv[i] = (wv[i] * dv) * dv;
    }
    *out = sqrt(np_sum_small(a.k, sv) / np_sum_small(a.k, wv));
}

// k up to kSummaryMaxK.  Labels and weights are re-read from L2 (the query's k indices and the target values they point at
// were fetched by this very thread a moment ago); `mode` votes once per first occurrence of a label.
__global__ void __launch_bounds__(256) summary_wide_kernel(SummaryArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nq * a.nc) return;
    const long q = e / a.nc;
    const int c = (int)(e - q * a.nc);
    const int tt = a.tab[c], code = a.tab[a.nc + c];
    const long* ids = a.idx + q * a.k;
    const double* dd = a.dist ? a.dist + q * a.k : nullptr;
    const double* ww = a.w ? a.w + q * a.k : nullptr;
    double* out = a.out + q * a.t + tt;
    auto label = [&](int i) -> double { return a.y[ids[i] * a.t + tt]; };
    if (code == kStatNearest) {
        *out = label(0);
        return;
    }
    if (code == kStatMin || code == kStatMax) {
        double r = label(0);
        for (int i = 1; i < a.k; ++i) {
            const double v = label(i);
            r = code == kStatMin ? (v < r ? v : r) : (v > r ? v : r);
        }
        *out = r;
        return;
    }
    bool any_zero = false;
    if (a.mode == 1)
        for (int i = 0; i < a.k; ++i) any_zero |= (dd[i] == 0.0);
    auto weight = [&](int i) -> double {
        if (a.mode == 0) return 1.0;
        if (a.mode == 2) return ww[i];
        if (any_zero) return dd[i] == 0.0 ? 1.0 : 0.0;
        return 1.0 / dd[i];
    };
    if (code == kStatMode) {
        double best_vote = 0.0, best_label = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = 0; i < a.k; ++i) {
            const double ci = label(i);
            bool first = true;
            for (int j = 0; j < i && first; ++j) first = !(label(j) == ci);
            if (!first) continue;
            const double vote = np_sum<double>(a.k, [&](int j) { return label(j) == ci ? weight(j) : 0.0; });
            summary_vote(vote, ci, best_vote, best_label);
        }
        *out = best_label;
        return;
    }
    // kStatStd
    const double den = np_sum<double>(a.k, [&](int i) { return weight(i); });
    double m;
    if (a.mode == 0 && a.t > 1) {
        double acc = label(0);
        for (int i = 1; i < a.k; ++i) acc = acc + label(i);
        m = acc / (double)a.k;
    } else {
        m = np_sum<double>(a.k, [&](int i) { return label(i) * weight(i); }) / den;
    }
    const double ss = np_sum<double>(a.k, [&](int i) {
        const double dv = label(i) - m;
        return (weight(i) * dv) * dv;
    });
    *out = sqrt(ss / den);
}
#endif  // SKNNR_KERNELS_SUMMARY

}  // namespace sknnr
