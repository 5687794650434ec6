// launch.hip.h -- the seam between the host translation unit (sknnr_hip.hip: index build, workspace, host pipeline, C ABI)
// and the kernel translation units (k_exact.hip, k_hamming.hip, k_forest.hip, k_mask.hip, k_planes.hip, k_narrow.hip, k_summary.hip, k_plan.hip, k_weights.hip, k_groups.hip, k_buffer.hip, k_tally.hip, k_zonal.hip, k_domain.hip, k_replay.hip, k_bootstrap.hip, k_coarse1.hip, k_coarse2.hip), which are compiled in
// parallel by _build.py.  Every kernel is launched through one of the functions below; each returns the launch's
// hipGetLastError() (the coarse launchers: an int that also says "no such instance").  Argument structs, geometry
// constants and shared-memory sizes live in the kernel headers; a header's non-template kernels are defined only in the unit
// that owns them (SKNNR_KERNELS_EXACT / SKNNR_KERNELS_HAMMING / SKNNR_KERNELS_FOREST / SKNNR_KERNELS_MASK / SKNNR_KERNELS_PLANES / SKNNR_KERNELS_NARROW / SKNNR_KERNELS_SUMMARY / SKNNR_KERNELS_PLAN / SKNNR_KERNELS_WEIGHTS / SKNNR_KERNELS_TALLY / SKNNR_KERNELS_ZONAL / SKNNR_KERNELS_BUFFER / SKNNR_KERNELS_DOMAIN / SKNNR_KERNELS_REPLAY / SKNNR_KERNELS_BOOTSTRAP), templates where they are instantiated.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bootstrap.hip.h"
#include "bucket.hip.h"
#include "buffer.hip.h"
#include "coarse2.hip.h"
#include "domain.hip.h"
#include "exact.hip.h"
#include "forest.hip.h"
#include "groups.hip.h"
#include "hamming.hip.h"
#include "mask.hip.h"
#include "narrow.hip.h"
#include "plan.hip.h"
#include "planes.hip.h"
#include "replay.hip.h"
#include "rescue.hip.h"
#include "summary.hip.h"
#include "tally.hip.h"
#include "weights.hip.h"
#include "zonal.hip.h"

namespace sknnr {
namespace launch {

// ---- k_exact.hip: everything around the pre-filter --------------------------------------------------------------------
hipError_t row_norms(const double* x, long n, int d, double* out, hipStream_t st);
hipError_t prep_direct(const PrepArgs& a, hipStream_t st);                  // ks <= 4, register-resident, 256 rows per block
hipError_t prep_lds(int rows_per_block, const PrepArgs& a, hipStream_t st);  // 256 / 128 / 64 rows per block staged through LDS
hipError_t check_finite(const double* x, long n_el, int* status, hipStream_t st);
hipError_t cell_assign(const CellArgs& a, hipStream_t st);
hipError_t cell_count(const CellArgs& a, hipStream_t st);
hipError_t cell_scatter(const CellArgs& a, hipStream_t st);
hipError_t finalize(const FinalizeArgs& f, long n, hipStream_t st);  // f.rec != nullptr: finalize_record_kernel
int finalize_lanes(const FinalizeArgs& f);                             // lanes per query of that launch
hipError_t exact_scan(int formula, bool chunked, const ScanArgs& a, long blocks, size_t lds_bytes, hipStream_t st);
hipError_t scan_merge(int formula, const ScanArgs& a, long blocks, size_t lds_bytes, int grid_wg_of_scan, int forced_slices,
                      hipStream_t st);
hipError_t pack_shards(const double* val, const long* idx, long nq, int n_shards, int kk, double* slice_v, int* slice_i,
                       hipStream_t st);
hipError_t predict(const PredictArgs& a, hipStream_t st);
hipError_t crosswalk(const long* table, const long* idx, long n, long* out, hipStream_t st);
hipError_t add_counter(const int* cnt, long long* total, hipStream_t st);
// the rescue re-sweep of the listed rows of one device chunk (rescue.hip.h; ks <= 4) and the call's totals behind it
hipError_t rescue(int ks, const RescueArgs& a, hipStream_t st);
hipError_t rescue_account(const int* listed, const int* state, long long* total, hipStream_t st);

// ---- k_hamming.hip ------------------------------------------------------------------------------------------------------
hipError_t hamming_pack(const double* xq, long nq, long nq_pad, int t, int tp, uint32_t* qimg, int* q_bad, hipStream_t st);
hipError_t hamming_rows(const double* x, long n, int t, int tpr, uint32_t* rows, hipStream_t st);
hipError_t hamming_coarse(const HammingArgs& a, hipStream_t st);
hipError_t hamming_rescore(const HammingRescoreArgs& a, hipStream_t st);
// full float64 distance rows of selected queries (sknnr_hamming_distances)
hipError_t hamming_distance_rows(const HammingRowsArgs& a, hipStream_t st);

// ---- k_forest.hip --------------------------------------------------------------------------------------------------------
// raw query rows -> float64 node ids of every tree of the handle's forests (RFNN / GBNN query-time map)
hipError_t forest_apply(const ForestArgs& a, hipStream_t st);

// ---- k_mask.hip: nodata rows of raster tiles (mask.hip.h) ---------------------------------------------------------------
// row_mask_kernel, then the single-workgroup scan: a.blk becomes the exclusive scan of the block counts, *n_valid the total
hipError_t row_mask(const MaskArgs& a, long* n_valid, hipStream_t st);
// valid rows, as raw bytes, to their dense position (a.row_units is filled in here from row_bytes and the addresses)
hipError_t row_compact(const CompactArgs& a, size_t row_bytes, hipStream_t st);
// bytes per copy row_compact chooses: the largest power of two up to 16 that divides row_bytes and both addresses
int compact_unit(const void* x, const void* out, size_t row_bytes);
hipError_t row_expand(const ExpandArgs& a, hipStream_t st);

// ---- k_planes.hip: band-first tiles <-> packed rows (planes.hip.h) ------------------------------------------------------
// a.c planes of a.n elements of elem_bytes (1, 2, 4 or 8), a.stride elements apart -> packed (n, c) rows; a raw byte move
hipError_t planes_to_rows(const PlanesArgs& a, int elem_bytes, hipStream_t st);
// packed (n, c) rows of 8-byte elements -> a.c planes of a.n elements, a.stride elements apart
hipError_t rows_to_planes(const PlanesArgs& a, hipStream_t st);

// ---- k_narrow.hip: result tiles to the raster's storage type (narrow.hip.h) ----------------------------------------------
// packed (n, c) float64 (kind kNarrowValue) or int64 (kNarrowIndex) -> dst_dtype (a sknnr_dtype), packed or as planes
// (a.stride); `wide` must satisfy narrow_wide_ok.  With a.table (indices only) every element is looked up first, and
// dst_dtype 0 (int64) is a pair too.  hipErrorInvalidValue for an impossible type pair.
hipError_t narrow(const NarrowArgs& a, int kind, int dst_dtype, bool wide, hipStream_t st);
// bytes per destination element of that pair, 0 when there is no such conversion; `table`: the launch has an id table
int narrow_dst_bytes(int kind, int dst_dtype, bool table = false);

// ---- k_summary.hip: per-target neighbour summaries (summary.hip.h) ----------------------------------------------------------
// the columns of a.tab (none of them `mean`) of every query; k <= kSummarySmallK: summary_kernel, else summary_wide_kernel
hipError_t summary(const SummaryArgs& a, hipStream_t st);

// ---- k_plan.hip: output plans (plan.hip.h) ------------------------------------------------------------------------------------
// the a.n_out entries of every query into (nq, n_out); k <= kSummarySmallK: plan_kernel, else plan_wide_kernel.  a.mean
// must hold the predict kernels' (nq, t) output when an entry is kStatMean (the caller's business: no kernel tests for it).
hipError_t plan(const PlanArgs& a, hipStream_t st);

// ---- k_weights.hip: distance-weight laws (weights.hip.h) ------------------------------------------------------------------
// a.w[e] = law(a.dist[e]) for a.n elements; hipErrorInvalidValue for an unknown law
hipError_t weight_law(const WeightLawArgs& a, hipStream_t st);

// ---- k_groups.hip: leave-group-out neighbours (groups.hip.h) -----------------------------------------------------------------
// reference rows [a.s.row_offset, + a.s.nq) against all rows of other groups; `blocks` workgroups take the passes grid-stride;
// chunked: d > kScanColChunk
hipError_t group_scan(int formula, bool chunked, const GroupScanArgs& a, long blocks, size_t lds_bytes, hipStream_t st);

// ---- k_buffer.hip: buffered leave-out (buffer.hip.h; the kMaskBuffer / kMaskBoth instantiations of groups.hip.h) --------------
// group_scan with the buffer predicate: mask is kMaskBuffer or kMaskBoth (hipErrorInvalidValue otherwise, and for a
// missing a.pos / a.codes); lds_bytes is group_scan_bytes(d, k, mask)
hipError_t buffer_scan(int mask, int formula, bool chunked, const GroupScanArgs& a, long blocks, size_t lds_bytes,
                       hipStream_t st);
// a.out[i] = rows excluded for row i under the masks given (a.pos and / or a.codes); zeroes a.out first;
// buffer_count_grid(a.n_ref) is its grid, kCountLdsBytes its LDS
hipError_t buffer_count(const BufferCountArgs& a, hipStream_t st);

// ---- k_tally.hip: neighbour usage (tally.hip.h) -----------------------------------------------------------------------------
// adds the a.n rows into a.cnt / a.maxbits / a.rec (none of them zeroed here); hipErrorInvalidValue for n_ref * k >= 2^32,
// for distances without maxima (or the reverse) and for null accumulators
hipError_t tally(const TallyArgs& a, hipStream_t st);
bool tally_wide_ok(const TallyArgs& a);  // that launch loads 16 bytes per lane
long tally_blocks(long n, int k);        // its workgroups
// every value of max_dist that is not > 0 becomes +0.0 (accumulate = 1 on a caller's array)
hipError_t tally_clean(double* max_dist, long n, hipStream_t st);

// ---- k_zonal.hip: zonal statistics of a prediction tile (zonal.hip.h) ----------------------------------------------------------
// adds the a.n pixels into a.acc / a.hist / a.rec (none of them initialised here), converting with dst_dtype (an integer
// sknnr_dtype); hipErrorInvalidValue for another type, for n_zones * c >= 2^32 and for null accumulators
hipError_t zonal(const ZonalArgs& a, int dst_dtype, hipStream_t st);
long zonal_blocks(long n, int c);  // its workgroups
// count, sum and limbs 0, min INT64_MAX, max INT64_MIN for n_keys (zone, column) pairs
hipError_t zonal_init(long long* acc, long n_keys, hipStream_t st);

// ---- k_domain.hip: distance domain of a tile's neighbour distances (domain.hip.h) ------------------------------------------------
// codes the a.n pixels into a.codes (or none) and adds them into a.acc / a.rec (neither zeroed here); with a.pred the rows
// of beyond pixels become NaN; hipErrorInvalidValue for a rank outside [1, k], m outside [1, 2^31 - 1], null accumulators
// and a mask without a threshold
hipError_t domain(const DomainArgs& a, hipStream_t st);
long domain_blocks(long n);  // its workgroups

// ---- k_replay.hip: stored neighbour tiles into the full-layout tile (replay.hip.h) ----------------------------------------------
// decodes the a.n pixels into a.out_idx / a.out_dist / a.bad and adds them into a.rec (not zeroed here); idx_bytes 4 or 8,
// dist_kind kReplayDistNone / F32 / F64, planes: the stored layout; hipErrorInvalidValue for k outside [1, ks], an
// unknown type, missing arrays, an id table of more than 2^31 - 1 entries and planes closer together than a.n
hipError_t replay(const ReplayArgs& a, int idx_bytes, int dist_kind, bool planes, hipStream_t st);
long replay_blocks(long n);  // its workgroups
// the final state of the pixels a.bad marks, behind the reduction of a tile decoded with ReplayArgs::provisional
hipError_t replay_blank(const ReplayBlankArgs& a, hipStream_t st);

// ---- k_bootstrap.hip: bootstrap standard errors of a tile's neighbour lists (bootstrap.hip.h) -----------------------------------
// the a.n_out entries of every pixel into (nq, n_out) and the two tallies added into a.tally (not zeroed here);
// hipErrorInvalidValue for B outside [1, kBootMaxB], k outside [1, kw], kw above kBootMaxKw, n_out outside [1, kBootMaxOut],
// an unknown mode or law, missing arrays, a table pitch that is no multiple of 64 and a.ppw other than bootstrap_ppw(B, kw)
hipError_t bootstrap(const BootstrapArgs& a, hipStream_t st);
long bootstrap_blocks(long n, int ppw);  // its workgroups: the pixel groups, at most kBootMaxGrid (they stride)

// ---- k_coarse1.hip / k_coarse2.hip: the MFMA pre-filters ----------------------------------------------------------------
struct Coarse1Launch {
    const char* rimg;
    int n_stages;
    const uint4* qimg;
    const double* qnc;
    float skip_scale;
    int n_sentinel;
    float* cand_val;
    int* cand_idx;
    long nq_pad;  // rows of the launch (a multiple of the workgroup's rows)
};
struct Coarse2Launch {
    const char* rhi;
    const char* rlo;
    int n_stages;
    const uint4* qimg;
    const double* qnc;
    float skip_scale;
    int n_sentinel;
    float* cand_val;
    int* cand_idx;
    int pos0;
    const int* qperm;
    const unsigned char* qcell;
    const int* cell_stage;
    long rows;  // positions [pos0, pos0 + rows) of the chunk (a multiple of the workgroup's rows)
    Coarse2Record rec;  // rec.entry != nullptr: merged candidate records instead of the lists (coarse2_record_supported)
};
constexpr int kNoInstance = -1;  // the (ks, list length, waves, rank) combination has no compiled kernel
// return 0 and *err = the launch status, or kNoInstance
int coarse1(int ks, int m_list, const Coarse1Launch& L, hipStream_t st, hipError_t* err);
int coarse2(int ks, int m_list, int waves, int rank_extra, const Coarse2Launch& L, hipStream_t st, hipError_t* err);
hipError_t coarse_matrix(int ks, const char* rimg, const int* perm, const uint4* qimg, int n_ref, long nq, long n_tiles,
                         long nqb, float* out);
// development builds (-DSKNNR_COARSE_COUNTERS / -DSKNNR_COARSE_TIMERS): print and clear the device-side tallies
void coarse1_dev_report();
void coarse2_dev_report();

}  // namespace launch
}  // namespace sknnr
