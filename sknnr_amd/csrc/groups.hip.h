// groups.hip.h -- leave-group-out neighbours: the float64 scan that knows about groups.
//
// Contract (include/sknnr_hip.h, sknnr_kneighbors_grouped, states it once): `codes` is an int32 label per reference
// row.  For reference row i the candidates are the rows r with codes[r] != codes[i] -- so never i itself.  Each pair
// has the float64 value kneighbors ranks it by under the call's formula (exact.hip.h: expanded, direct, weighted
// Hamming).  The answer of row i is the k candidates smallest by (value, r), ascending in that order, then sqrt (not for
// Hamming), then sknnr's reorder when asked for.  Exact ties at the k-th value go to the lower index: no heap history
// is replayed here, because no reference behaviour exists for a grouped search.
//
// group_scan_kernel is a sibling of exact_scan_kernel (exact.hip.h): the same float64 tiles -- a pass of queries in
// LDS, steps of kScanRefs reference columns of the transposed copy, two columns per thread -- and per pair THE SAME
// OPERATIONS IN THE SAME ORDER, so the values are bit-equal to the oracle's.  It differs in four places:
//   queries   reference rows [s.row_offset, s.row_offset + s.nq), read from the handle's own row copy (s.ref)
//   mask      a thread loads the codes of its two columns once per step, a query's code sits in LDS beside its row; a
//             pair of equal codes is published as +inf (like the padding columns), so the ballot never offers it
//   selection the sorted list for every formula: sorted_insert_ref with strict < against the k-th entry, references
//             offered in ascending index order -- exactly "smallest (value, index)"
//   finish    the list is in (value, index) order already: sqrt, reorder, k entries out.  No self-drop: the mask did it
// Wide rows: d > kScanColChunk (the node-id rows of RFNN / GBNN) use exact_scan_kernel's column chunking -- the queries'
// columns pass through LDS kScanColChunk at a time inside every step, the CHUNKED instantiation.
// Slices: none.  A pass is one workgroup whatever the row count ("Leave-group-out", has the cost).
//
// Buffered leave-out (include/sknnr_hip.h, sknnr_index_set_buffer, states the contract once): the MASK template parameter
// of group_scan_kernel says which predicates exclude a pair -- kMaskGroups: equal codes (the kernel as it was);
// kMaskBuffer: g(i, r) = ((xi - xr)^2 + (yi - yr)^2) + (zi - zr)^2 <= r2 on the rows' positions, every operation a
// separately rounded float64 operation; kMaskBoth: either.  Positions are a (3, n_ref) column-major float64 array like
// refT (a missing column is all +0.0), loaded by a thread for its two columns at publish time only, when the row loads
// of the feature loop are dead; the positions of the pass's queries sit in LDS beside their codes.  (Fetching a step's
// positions one step ahead into LDS slots of the thread's own was tried and was slower: DESIGN.md, "Buffered leave-out".)
#pragma once
#include "exact.hip.h"

namespace sknnr {

struct GroupScanArgs {
    SelectArgs s;        // s.ref: the (n_ref, d) rows the queries are read from; s.xq unused; s.kk == s.k
    const double* refT;  // (d, n_ref) transposed reference rows
    const int* codes;    // (n_ref) group code of every reference row, >= 0 (read when MASK has kMaskGroups)
    const double* pos;   // (3, n_ref) plot positions, column-major (read when MASK has kMaskBuffer)
    double r2;           // radius * radius: a pair with g(i, r) <= r2 is excluded
};

// which predicates exclude a pair (group_scan_kernel's MASK, sknnr_debug_last_buffer's out[0])
constexpr int kMaskGroups = 1;
constexpr int kMaskBuffer = 2;
constexpr int kMaskBoth = kMaskGroups | kMaskBuffer;
constexpr int kPosCols = 3;  // rows of the position array: x, y, z

// Two queries per wave under every formula: the codes and the mask cost registers on top of exact_scan_kernel's, whose
// three queries per wave (expanded formula) sit at 165 VGPRs.  Eight queries per pass also keep the LDS of the widest
// accepted call (d >= kScanColChunk, k = 192) at 115 KiB, inside a CU's 160 KiB.
constexpr int kGroupQpw = 2;
constexpr int kGroupNq = kScanWaves * kGroupQpw;  // queries per workgroup pass

// Workgroup LDS: xs[NQ][dpad] | qn[NQ] | hv[NQ][k] | hi[NQ][kp] | code[NQ] | pos[NQ][3] (buffer masks only) |
// d2[NQ][kScanRefs]
struct GroupScanLayout {
    int dpad, kp;
    size_t xs, qn, hv, hi, code, pos, d2, total;
};
__host__ __device__ constexpr GroupScanLayout group_scan_layout(int d, int k, int mask = kMaskGroups) {
    GroupScanLayout L{};
    L.dpad = ((d < kScanColChunk ? d : kScanColChunk) + 1) & ~1;
    L.kp = k + (k & 1);
    size_t b = 0;
    L.xs = b;   b += 8 * (size_t)kGroupNq * L.dpad;
    L.qn = b;   b += 8 * (size_t)kGroupNq;
    L.hv = b;   b += 8 * (size_t)kGroupNq * k;
    L.hi = b;   b += 4 * (size_t)kGroupNq * L.kp;
    L.code = b; b += 4 * (size_t)kGroupNq;
    b = (b + 15) & ~(size_t)15;
    L.pos = b;  b += (mask & kMaskBuffer) ? 8 * (size_t)kGroupNq * kPosCols : 0;
    L.d2 = b;   b += 8 * (size_t)kGroupNq * kScanRefs;
    L.total = b;
    return L;
}
__host__ __device__ constexpr size_t group_scan_bytes(int d, int k, int mask = kMaskGroups) {
    return group_scan_layout(d, k, mask).total;
}

// The end of a query: its k list entries, ascending by (value, index) -> sqrt -> sknnr's reorder -> outputs.
template <int FORMULA>
__device__ void group_finish_query(const SelectArgs& s, long q, double* hv, int* hi) {
    const int n = s.k;
    const long self_id = s.row_offset + q;
    if (FORMULA != 2)  // (a Hamming distance is not a square)
        for (int e = 0; e < n; ++e) hv[e] = sqrt(hv[e] > 0.0 ? hv[e] : 0.0);
    if (s.deterministic) {
        double dmax = 0.0;
        for (int e = 0; e < n; ++e) dmax = fmax(dmax, hv[e]);
        const double row_scale = fmax(dmax, 1.0);
        // stable insertion sort by (rounded, |idx - row|, idx)  (REF _base.py:166-175)
        for (int e = 1; e < n; ++e) {
            const double dv = hv[e];
            const int iv = hi[e];
            const double k0 = round_key(dv / row_scale, s.pow10, s.pow10_is_divisor);
            long k1 = (long)iv - self_id;
            k1 = k1 < 0 ? -k1 : k1;
            int jj = e - 1;
            while (jj >= 0) {
                const double k0j = round_key(hv[jj] / row_scale, s.pow10, s.pow10_is_divisor);
                long k1j = (long)hi[jj] - self_id;
                k1j = k1j < 0 ? -k1j : k1j;
                const bool greater = (k0j > k0) || (k0j == k0 && (k1j > k1 || (k1j == k1 && hi[jj] > iv)));
                if (!greater) break;
                hv[jj + 1] = hv[jj];
                hi[jj + 1] = hi[jj];
                --jj;
            }
            hv[jj + 1] = dv;
            hi[jj + 1] = iv;
        }
    }
    for (int e = 0; e < n; ++e) {
        if (s.out_dist) s.out_dist[q * s.k + e] = hv[e];
        s.out_idx[q * s.k + e] = hi[e];
    }
}

// One workgroup (4 waves) per pass of kGroupNq queries, passes taken grid-stride.  Per step of kScanRefs references every
// thread loads TWO columns of the transposed copy (coalesced) and their two codes once, evaluates the float64 values to
// all queries of the pass, and publishes them -- or +inf for a pair that MASK excludes -- to LDS; every wave then offers
// them, in index order, to the lists of its own queries.
template <int FORMULA, bool CHUNKED = false, int MASK = kMaskGroups>
__global__ void __launch_bounds__(kScanWaves * 64, SKNNR_SCAN_WPS) group_scan_kernel(GroupScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NT = kScanWaves * 64;
    constexpr int QPW = kGroupQpw;
    constexpr int NQ = kGroupNq;
    const SelectArgs& s = a.s;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int K = s.k;
    const int d = s.d;
    constexpr bool by_group = (MASK & kMaskGroups) != 0, by_buffer = (MASK & kMaskBuffer) != 0;
    const GroupScanLayout L = group_scan_layout(d, K, MASK);
    double* xs = (double*)(smem_raw + L.xs);
    double* qns = (double*)(smem_raw + L.qn);
    double* hv_all = (double*)(smem_raw + L.hv);
    int* hi_all = (int*)(smem_raw + L.hi);
    int* qcode = (int*)(smem_raw + L.code);
    double* qpos = (double*)(smem_raw + L.pos);
    double* d2buf = (double*)(smem_raw + L.d2);

    const long n_items = s.nq;
    for (long f0 = (long)blockIdx.x * NQ; f0 < n_items; f0 += (long)gridDim.x * NQ) {
        const int n_here = (int)((n_items - f0) < NQ ? (n_items - f0) : NQ);
        __syncthreads();  // previous pass's LDS state is dead
        // padding slots repeat the pass's last query; nothing is written for them
        // query rows of the pass, columns [c0, c0 + kScanColChunk): everything when d fits one chunk (loaded once per
        // pass), else chunk by chunk inside the sweep
        constexpr bool chunked = CHUNKED;  // d > kScanColChunk (the launcher picks the instantiation)
        auto load_chunk = [&](int c0) {
            const int cw = (d - c0) < kScanColChunk ? (d - c0) : kScanColChunk;
            for (int e = tid; e < NQ * cw; e += NT) {
                const int qi = e / cw, c = e - qi * cw;
                const long row = s.row_offset + f0 + (qi < n_here ? qi : n_here - 1);
                xs[qi * L.dpad + c] = s.ref[row * d + c0 + c];
            }
        };
        if (!chunked) load_chunk(0);
        for (int i = tid; i < NQ * K; i += NT) {
            const int qi = i / K, e = i - qi * K;
            hv_all[qi * K + e] = DBL_MAX;
            hi_all[qi * L.kp + e] = 0;
        }
        if (by_group && tid < NQ) qcode[tid] = a.codes[s.row_offset + f0 + (tid < n_here ? tid : n_here - 1)];
        if (by_buffer && tid < NQ * kPosCols) {
            const int qi = tid / kPosCols, c = tid - qi * kPosCols;
            qpos[tid] = a.pos[(size_t)c * s.n_ref + s.row_offset + f0 + (qi < n_here ? qi : n_here - 1)];
        }
        __syncthreads();
        if (FORMULA == 0 && tid < NQ) {
            double qn = 0.0;
            if (!chunked) {  // the rows are in LDS
                for (int c = 0; c < d; ++c) qn = fma(xs[tid * L.dpad + c], xs[tid * L.dpad + c], qn);
            } else {
                const double* xr = s.ref + (s.row_offset + f0 + (tid < n_here ? tid : n_here - 1)) * d;
                for (int c = 0; c < d; ++c) qn = fma(xr[c], xr[c], qn);
            }
            qns[tid] = qn;
        }
        double bound[QPW];
#pragma unroll
        for (int i = 0; i < QPW; ++i) bound[i] = DBL_MAX;

        const size_t ld = (size_t)s.n_ref;
        for (int j0 = 0; j0 < s.n_ref; j0 += kScanRefs) {
            const int ja = j0 + tid, jb = j0 + NT + tid;
            const double* cola = a.refT + (ja < s.n_ref ? ja : 0);
            const double* colb = a.refT + (jb < s.n_ref ? jb : 0);
            // the codes of this thread's two columns, once per step (no query has a negative code)
            const int ca = (by_group && ja < s.n_ref) ? a.codes[ja] : -1;
            const int cb = (by_group && jb < s.n_ref) ? a.codes[jb] : -1;
            double acc[NQ][2];
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) acc[qi][0] = acc[qi][1] = 0.0;
            for (int c0 = 0; c0 < (chunked ? d : 1); c0 += kScanColChunk) {
            if (chunked) {
                __syncthreads();  // everyone is done with the previous chunk
                load_chunk(c0);
                __syncthreads();
            }
            const int ce = (!chunked || (d - c0) < kScanColChunk) ? d : c0 + kScanColChunk;
            int c = c0;
            for (; c + 8 <= ce; c += 8) {
                double ra[8], rb[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    ra[w] = cola[(size_t)(c + w) * ld];
                    rb[w] = colb[(size_t)(c + w) * ld];
                }
#pragma unroll
                for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
                    for (int w = 0; w < 8; ++w) {
                        const double x = xs[qi * L.dpad + (c - c0) + w];
                        if (FORMULA == 0) {
                            acc[qi][0] = fma(x, ra[w], acc[qi][0]);
                            acc[qi][1] = fma(x, rb[w], acc[qi][1]);
                        } else if (FORMULA == 2) {
                            // weighted Hamming as scipy's cdist evaluates it on the float64 node ids:
                            // s += (u != v) * w, in tree order  (REF _weighted_trees.py:53-59, :139-140)
                            const double wv = s.hw[c + w];
                            acc[qi][0] = x != ra[w] ? acc[qi][0] + wv : acc[qi][0];
                            acc[qi][1] = x != rb[w] ? acc[qi][1] + wv : acc[qi][1];
                        } else {
                            const double ta = x - ra[w], tb = x - rb[w];
                            acc[qi][0] = acc[qi][0] + ta * ta;
                            acc[qi][1] = acc[qi][1] + tb * tb;
                        }
                    }
                }
            }
            for (; c < ce; ++c) {
                const double rav = cola[(size_t)c * ld], rbv = colb[(size_t)c * ld];
#pragma unroll
                for (int qi = 0; qi < NQ; ++qi) {
                    const double x = xs[qi * L.dpad + (c - c0)];
                    if (FORMULA == 0) {
                        acc[qi][0] = fma(x, rav, acc[qi][0]);
                        acc[qi][1] = fma(x, rbv, acc[qi][1]);
                    } else if (FORMULA == 2) {
                        const double wv = s.hw[c];
                        acc[qi][0] = x != rav ? acc[qi][0] + wv : acc[qi][0];
                        acc[qi][1] = x != rbv ? acc[qi][1] + wv : acc[qi][1];
                    } else {
                        const double ta = x - rav, tb = x - rbv;
                        acc[qi][0] = acc[qi][0] + ta * ta;
                        acc[qi][1] = acc[qi][1] + tb * tb;
                    }
                }
            }
            }  // column chunks
            const double rna = (FORMULA == 0 && ja < s.n_ref) ? s.rn[ja] : 0.0;
            const double rnb = (FORMULA == 0 && jb < s.n_ref) ? s.rn[jb] : 0.0;
            // the positions of this thread's two columns: loaded here, where the feature loop's row loads are dead
            double pa[kPosCols] = {}, pb[kPosCols] = {};
            if (by_buffer) {
#pragma unroll
                for (int c = 0; c < kPosCols; ++c) {
                    pa[c] = a.pos[(size_t)c * ld + (ja < s.n_ref ? ja : 0)];
                    pb[c] = a.pos[(size_t)c * ld + (jb < s.n_ref ? jb : 0)];
                }
            }
            __syncthreads();  // the previous step's offers have finished reading d2buf (and qns is published)
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                double da = acc[qi][0], db = acc[qi][1];
                if (FORMULA == 0) {
                    const double qn = qns[qi];
                    da = qn + (-2.0 * da) + rna;
                    db = qn + (-2.0 * db) + rnb;
                    da = da > 0.0 ? da : 0.0;
                    db = db > 0.0 ? db : 0.0;
                }
                if (FORMULA == 2) {
                    da = da / s.hw_sum;
                    db = db / s.hw_sum;
                }
                // the mask: a row of the query's own group is no candidate (ca / cb = -1 on padding columns), nor is a
                // row within the radius of the query's position (the query itself: g = 0 <= r2)
                if constexpr (MASK == kMaskGroups) {
                    const int qc = qcode[qi];
                    d2buf[qi * kScanRefs + tid] = (ja < s.n_ref && ca != qc) ? da : INFINITY;
                    d2buf[qi * kScanRefs + NT + tid] = (jb < s.n_ref && cb != qc) ? db : INFINITY;
                    continue;
                }
                bool ka = ja < s.n_ref, kb = jb < s.n_ref;
                if (by_group) {
                    const int qc = qcode[qi];
                    ka = ka && ca != qc;
                    kb = kb && cb != qc;
                }
                if (by_buffer) {
                    const double qx = qpos[qi * kPosCols], qy = qpos[qi * kPosCols + 1], qz = qpos[qi * kPosCols + 2];
                    const double ax = qx - pa[0], ay = qy - pa[1], az = qz - pa[2];
                    const double bx = qx - pb[0], by = qy - pb[1], bz = qz - pb[2];
                    const double ga = (ax * ax + ay * ay) + az * az;
                    const double gb = (bx * bx + by * by) + bz * bz;
                    ka = ka && !(ga <= a.r2);
                    kb = kb && !(gb <= a.r2);
                }
                d2buf[qi * kScanRefs + tid] = ka ? da : INFINITY;
                d2buf[qi * kScanRefs + NT + tid] = kb ? db : INFINITY;
            }
            __syncthreads();
#pragma unroll 1
            for (int i = 0; i < QPW; ++i) {
                const int qi = wave * QPW + i;
                if (qi >= n_here) break;
                double* hv = hv_all + qi * K;
                int* hi = hi_all + qi * L.kp;
                const double* buf = d2buf + qi * kScanRefs;
                double bd = bound[i];
#pragma unroll 1
                for (int u = 0; u < kScanRefs / 64; ++u) {
                    const double v64 = buf[64 * u + lane];
                    unsigned long long m = __builtin_amdgcn_ballot_w64(v64 < bd);
                    while (m) {
                        const int bit = __builtin_ctzll(m);
                        m &= m - 1;
                        const double v = __shfl(v64, bit, 64);
                        if (v < bd) {  // the bound may have dropped since the ballot
                            if (lane == 0) sorted_insert_ref(hv, hi, K, v, j0 + 64 * u + bit);
                            __builtin_amdgcn_wave_barrier();
                            bd = hv[K - 1];
                        }
                    }
                }
                bound[i] = bd;
            }
        }

        if (lane == 0) {
            for (int i = 0; i < QPW; ++i) {
                const int qi = wave * QPW + i;
                if (qi >= n_here) break;
                group_finish_query<FORMULA>(s, f0 + qi, hv_all + qi * K, hi_all + qi * L.kp);
            }
        }
    }
}

}  // namespace sknnr
