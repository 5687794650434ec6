/*
 * sknnr_hip.h -- C ABI of the MI355X (gfx950) backend for sknnr's
 * kneighbors()/predict() hot path.
 *
 * Drop-in boundary: the reference has no FFI; everything its
 * estimators need from the engine is behind two calls on a fitted
 * sklearn.neighbors.KNeighborsRegressor,
 *     RawKNNRegressor.kneighbors  -> super().kneighbors(X, n_neighbors, return_distance=True)
 *                                    /root/reference/src/sknnr/_base.py:162-164
 *     (inherited) predict         -> /root/reference/src/sknnr/_base.py:39, :346-348
 * plus the transform that precedes them (_base.py:236-239) and the post-steps that
 * follow them (_base.py:166-180).  Each entry point below names the reference
 * interface it replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns
 * SKNNR_OK (0) or a negative sknnr_status; sknnr_last_error() gives the message of
 * the calling thread's last failure.  All matrices are row-major (C order) float64,
 * indices are int64 -- exactly what the reference hands to / gets from scikit-learn.
 * The caller owns every buffer it passes; the handle owns its device copies.
 * One call at a time per handle: entry points serialise on a per-handle mutex, and a call that is handed a
 * different stream than the previous one first makes that stream wait (hipStreamWaitEvent) for the previous
 * call's last kernel, because both use the handle's workspace.
 */
#ifndef SKNNR_HIP_H
#define SKNNR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; exactly these declarations are exported. */
#pragma GCC visibility push(default)

#define SKNNR_ABI_VERSION 5

typedef enum sknnr_status {
    SKNNR_OK = 0,
    SKNNR_ERR_INVALID = -1,     /* bad argument (message says which) */
    SKNNR_ERR_K_TOO_LARGE = -2, /* n_neighbors > n_samples_fit: SKL/neighbors/_base.py:848-859 */
    SKNNR_ERR_NO_TARGETS = -3,  /* predict without targets */
    SKNNR_ERR_UNSUPPORTED = -4, /* outside the envelope of the HIP kernels (no CPU fallback exists) */
    SKNNR_ERR_HIP = -5,         /* HIP runtime failure (message carries hipGetErrorString) */
    SKNNR_ERR_NO_DEVICE = -6,   /* no usable gfx950 device */
    SKNNR_ERR_NONFINITE = -7    /* query (or reference) rows contain NaN or infinity; the message is scikit-learn's
                                   ("Input X contains NaN." / "Input X contains infinity or a value too large
                                   for dtype('float64')."): SKL/utils/validation.py _assert_all_finite, reached
                                   from SKL/neighbors/_base.py:838-845 and REF transformers' transform() */
} sknnr_status;

/* Where the caller's query/output buffers live. */
typedef enum sknnr_memspace {
    SKNNR_MEM_HOST = 0,  /* ordinary host pointers; the library stages through PCIe */
    SKNNR_MEM_DEVICE = 1 /* device pointers on the handle's GPU (e.g. torch tensor.data_ptr()) */
} sknnr_memspace;

/* Which float64 expression the reference's engine evaluates for a pair
 * (SKL/neighbors/_base.py:620-648 picks the engine at fit time). */
typedef enum sknnr_formula {
    SKNNR_FORMULA_EXPANDED = 0, /* "brute"/ArgKmin: |x|^2 - 2 x.y + |y|^2, clamped at 0
                                   (SKL/metrics/_pairwise_distances_reduction/_argkmin.pyx.tp:492-502) */
    SKNNR_FORMULA_DIRECT = 1,   /* "kd_tree" (D <= 15): sum (x - y)^2
                                   (SKL/metrics/_dist_metrics.pxd.tp:39-57) */
    SKNNR_FORMULA_HAMMING = 2   /* RFNN / GBNN: weighted Hamming distance of tree node ids,
                                   sum_t w_t [a_t != b_t] / sum_t w_t, as scipy's cdist(metric="hamming", w=w)
                                   evaluates it on the float64 ids (sums in tree order), reached from
                                   REF _weighted_trees.py:53-59 (algorithm="brute", metric="hamming") and
                                   :139-140 (metric_params={"w": hamming_weights_}) through
                                   SKL/neighbors/_base.py:896-926 (pairwise_distances_chunked +
                                   _kneighbors_reduce_func).  No square root; rows tied exactly at the k-th
                                   distance are taken lowest index first.  The reference takes what numpy's
                                   argpartition takes; a caller that wants exactly that choice gets the tied
                                   rows' full distance rows from sknnr_hamming_distances and runs argpartition
                                   on them (the Python layer's hamming_tie_policy("numpy"); INTEGRATION.md,
                                   "Hamming ties").  Needs sknnr_index_set_hamming_weights. */
} sknnr_formula;

/* Element type of the query rows handed to kneighbors / predict / a stream (opts->query_dtype).  Rasters come as
 * float32 / int16 / uint8 ...; the reference widens them to float64 on the host before any arithmetic
 * (validate_data(..., dtype=FLOAT_DTYPES) then `X - env_center_` in float64: REF transformers/_cca_transformer.py:78-87,
 * _ccora_transformer.py:67-70; integers become float64 in every transformer).  Here the kernel that reads the rows
 * widens them -- exact for every type below, so the results are those of the float64 call bit for bit -- and the rows
 * cross PCIe at their own width. */
typedef enum sknnr_dtype {
    SKNNR_DTYPE_F64 = 0,
    SKNNR_DTYPE_F32 = 1,
    SKNNR_DTYPE_I16 = 2,
    SKNNR_DTYPE_U16 = 3,
    SKNNR_DTYPE_U8 = 4,
    SKNNR_DTYPE_I32 = 5
} sknnr_dtype;

typedef enum sknnr_weight_mode {
    SKNNR_WEIGHTS_UNIFORM = 0,  /* np.mean over the k neighbours  (SKL/neighbors/_regression.py:254-255) */
    SKNNR_WEIGHTS_DISTANCE = 1, /* 1/d, rows containing d == 0 become a 0/1 mask (SKL/neighbors/_base.py:113-119) */
    SKNNR_WEIGHTS_EXPLICIT = 2, /* caller supplies w (nq, k): result of a Python callable on the distances */
    /* A weight_mode argument is one of the three above in its low byte, optionally OR-ed with flag bits that name the
     * dtype numpy reduces in (the values themselves always travel as float64, holding the float32 ones exactly): */
    SKNNR_WEIGHTS_BASE_MASK = 0xff,
    SKNNR_WEIGHTS_F32_TARGETS = 0x100, /* the targets are float32: the uniform mean runs in binary32 (np.mean keeps the
                                          dtype); with F32_WEIGHTS also y * w, its sum and the quotient.  Distance
                                          weights ignore it (1 / d is float64, so everything promotes) */
    SKNNR_WEIGHTS_F32_WEIGHTS = 0x200  /* EXPLICIT only: w is float32, np.sum(w, axis=1) runs in binary32 */
} sknnr_weight_mode;

/* Distance-weight laws: w = law(d) evaluated ON THE DEVICE between the search and the reduction (opts->weight_law), in
 * place of a Python weights callable on the host.  All float64, every + - * / one IEEE rounding (never fused), so the
 * weights are numpy's bit for bit (sknnr_amd/csrc/weights.hip.h; sknnr_amd/weights.py states them in numpy).  p0 is the
 * law's parameter (sknnr_index_set_weight_law_params), finite and > 0; p1 is unused so far. */
typedef enum sknnr_weight_law {
    SKNNR_LAW_NONE = 0,            /* no law: the call does what it did before the field existed */
    SKNNR_LAW_INVERSE = 1,         /* 1 / (p0 + d)           yaImpute's weighting at p0 = 1 */
    SKNNR_LAW_INVERSE_SQUARED = 2, /* 1 / (p0 + d * d) */
    SKNNR_LAW_TRIANGULAR = 3,      /* max(0, 1 - d / p0)     compact: a row may be all zero, its prediction is NaN */
    SKNNR_LAW_EPANECHNIKOV = 4     /* max(0, 1 - (d / p0)^2) compact, likewise */
} sknnr_weight_law;

typedef struct sknnr_index sknnr_index; /* opaque handle */

/* Per-call options of kneighbors/predict.  Zero-initialise, then set fields. */
typedef struct sknnr_query_opts {
    int32_t n_neighbors;   /* k of this call (reference: n_neighbors argument / ctor value) */
    int32_t exclude_self;  /* 1 = the X=None path: the query rows ARE reference rows
                              [row_offset, row_offset + nq); k+1 are searched and each row's own
                              index is dropped (SKL/neighbors/_base.py:828-833, :936-963) */
    int32_t deterministic; /* 1 = apply sknnr's tie-break reorder (REF _base.py:166-175) */
    int32_t decimals;      /* RawKNNRegressor.DISTANCE_PRECISION_DECIMALS (REF _base.py:102), default 10 */
    int32_t formula;       /* sknnr_formula */
    int32_t apply_affine;  /* 1 = apply the handle's query-time map: queries are untransformed (d_in columns) and
                              go through the affine map (REF _base.py:236-239) -- or, with formula = HAMMING on a
                              handle with a forest (sknnr_index_set_forest), through the forests, which turn them
                              into node ids; 0 = already transformed (d columns) */
    int32_t weight_mode;   /* predict only: sknnr_weight_mode, with its F32_TARGETS flag */
    int32_t check_finite;  /* 1 = the kernels that read the query rows also test them for NaN / infinity
                              (what validate_data(ensure_all_finite=True) does on the host in the reference).
                              Host-memory calls then fail with SKNNR_ERR_NONFINITE; device-memory calls stay
                              asynchronous and the caller polls sknnr_check_finite() */
    int32_t query_dtype;   /* sknnr_dtype of the query rows `q` (0 = float64).  Other types need the MFMA envelope
                              (d <= 128) and a Euclidean formula, or the forest map (formula = HAMMING with
                              apply_affine = 1); they are widened by the kernel that reads them */
    int32_t weight_law;    /* predict / summarize / streams only: sknnr_weight_law, 0 = none (the field was reserved_,
                              kept 0).  Non-zero: weight_mode must be SKNNR_WEIGHTS_EXPLICIT (F32_TARGETS allowed,
                              F32_WEIGHTS not: the laws are float64) and the law must be the one whose parameters the
                              handle holds (sknnr_index_set_weight_law_params), else SKNNR_ERR_INVALID.  The weights
                              are then computed on the device from the call's own distances.  Ignored by kneighbors */
    int64_t row_offset;    /* position of query row 0 inside the logical call: key 2 of the reorder is
                              |idx - row| with row counted over the whole call (REF _base.py:171), so a
                              shard or chunk must carry its global offset */
} sknnr_query_opts;

/* Counters of the handle since creation (or the last reset). */
typedef struct sknnr_stats {
    int64_t queries;           /* query rows answered */
    int64_t coarse_queries;    /* rows that went through the f16x3 MFMA pre-filter */
    int64_t exact_fallbacks;   /* rows whose certificate failed and were re-scanned in float64 */
    int64_t exact_only_queries;/* rows answered by the float64 scan alone (k or d outside the MFMA envelope) */
    double  last_kernel_ms;    /* device time of the most recent call (hipEvent, launch stream) */
    double  last_coarse_ms;    /* ... of which the MFMA pre-filter kernel */
    double  total_kernel_ms;   /* device time of all calls since the last reset (sums the chunks of a step) */
    double  total_coarse_ms;   /* ... of which the MFMA pre-filter kernel */
    int64_t timed_calls;       /* calls summed in the two totals */
    int64_t coarse_rows_timed; /* query rows processed by the pre-filter launches that total_coarse_ms sums: all rows of a
                                  call, except that when the thin last round runs beside the finaliser (side stream)
                                  only the 16-wave bulk launch is timed -- the rows to price its time against */
    double  mfma_executed_ratio; /* matrix work the most recent pre-filter launch ISSUED over the algorithmic
                                  2 nq n_ref d: reference rows padded to whole tiles / stages, the seed window swept
                                  twice, K padded to 16 (second-generation kernel: exact; first generation: its main
                                  products only, the correction products of visited tiles come on top) */
} sknnr_stats;

/* ---- lifetime -------------------------------------------------------------------------- */

/* Number of visible HIP devices (0 if none).  Never fails. */
int32_t sknnr_device_count(void);

/* ABI version of the loaded library (== SKNNR_ABI_VERSION). */
int32_t sknnr_abi_version(void);

/* Message of this thread's last error ("" if none). */
const char* sknnr_last_error(void);

/*
 * Build the device-resident index from the transformed reference rows.
 * Replaces KNeighborsRegressor.fit -> NeighborsBase._fit storing _fit_X and _y
 * (SKL/neighbors/_base.py:474-694; called from REF _base.py:107, :266-267).
 *   ref   : host, (n_ref, d) transformed features (the reference's _fit_X); every value finite, else
 *           SKNNR_ERR_NONFINITE (the reference's fit raises the same ValueError from its input validation)
 *   y     : host, (n_ref, t) targets (the reference's _y) or NULL (kneighbors only)
 *   device: HIP device ordinal
 */
int sknnr_index_create(const double* ref, int64_t n_ref, int32_t d, const double* y, int32_t t,
                       int32_t device, sknnr_index** out);

/* Free the handle and everything it owns.  NULL is allowed. */
void sknnr_index_destroy(sknnr_index* index);

/*
 * Install the query-time feature transform X -> ((X - center) / scale) @ proj.
 * Replaces transformer_.transform(X) (REF _base.py:236-239;
 * transformers/_cca_transformer.py:87, _ccora_transformer.py:70,
 * _mahalanobis_transformer.py:55, SKL/preprocessing/_data.py:1057-1098).
 *   center, scale : host, (d_in) or NULL;  proj : host, (d_in, d) or NULL (then d_in == d).
 */
int sknnr_index_set_affine(sknnr_index* index, int32_t d_in, const double* center,
                           const double* scale, const double* proj);

/*
 * Weights of the weighted-Hamming distance (one per column of the node-id matrix; finite, >= 0, not all 0).
 * Replaces metric_params={"w": self.hamming_weights_} (REF _weighted_trees.py:139-140).  The index then
 * holds node ids (float64 copies of the int64 ids the transformers emit, REF
 * transformers/_tree_node_transformer.py:177-201) and answers opts->formula = SKNNR_FORMULA_HAMMING.
 */
int sknnr_index_set_hamming_weights(sknnr_index* index, const double* w, int32_t n);

/*
 * Install the query-time forest map of RFNN / GBNN: raw feature rows -> the node each tree sends them to.
 * Replaces transformer_.transform(X) of the tree-node transformers (REF transformers/_tree_node_transformer.py:177-201:
 * forest.apply per forest, SKL/tree/_tree.pyx:956-995 _apply_dense) for query rows: a row's features are converted
 * to float32 (as apply does) and walked down every tree (x <= threshold: left child, else right).  Tree t yields
 * column t of the node-id rows the weighted-Hamming search reads, so n_trees must equal the handle's d.
 *   d_in        : features of a raw row
 *   tree_offset : host, (n_trees + 1) int64: tree t owns nodes [tree_offset[t], tree_offset[t + 1]), at least one
 *   threshold   : host, (tree_offset[n_trees]) float64, the trees' tree_.threshold one after another
 *   feature, left, right : host, int32, the same length: tree_.feature, tree_.children_left / children_right
 *                 (child ids local to the tree; -1 on both for a leaf)
 * Checked on the host: every child id is greater than its parent's and below the tree's node count, every internal
 * node's feature lies in [0, d_in) and its threshold is not NaN (else SKNNR_ERR_INVALID).  The map then applies with
 * opts->formula = SKNNR_FORMULA_HAMMING and opts->apply_affine = 1, to float64 rows or any narrower query_dtype.
 * Besides NaN and infinity, a finite value that overflows float32 is refused with SKNNR_ERR_NONFINITE and
 * scikit-learn's message ("Input X contains infinity or a value too large for dtype('float32').").
 */
int sknnr_index_set_forest(sknnr_index* index, int32_t d_in, int32_t n_trees, const int64_t* tree_offset,
                           const double* threshold, const int32_t* feature, const int32_t* left,
                           const int32_t* right);

/*
 * The installed forest map alone: out_ids (nq, n_trees) float64 = the node ids of the rows q (nq, d_in) of
 * query_dtype, in `mem` (device: launched on the default stream; the call returns when the ids are written).
 * Fails with SKNNR_ERR_NONFINITE as the map does inside a search.  Replaces forest.apply for those rows.
 */
int sknnr_forest_apply(sknnr_index* index, const void* q, int64_t nq, int32_t query_dtype, int32_t mem,
                       double* out_ids);

/*
 * The same affine map as a stand-alone call (no handle): out = ((x - center) / scale) @ proj.
 * Replaces X_transformed = self.transformer_.transform(X) at fit time (REF _base.py:251), so
 * that the stored reference rows and later query rows go through one and the same float64
 * fma chain.  x, out: host, (n, d_in) and (n, d); center/scale/proj as in set_affine.
 */
int sknnr_affine_transform(const double* x, int64_t n, int32_t d_in, const double* center,
                           const double* scale, const double* proj, int32_t d, double* out,
                           int32_t device);

/*
 * The distance-weight law of the handle and its two float64 parameters (they do not fit sknnr_query_opts).  Replaces
 * KNeighborsRegressor(weights=<callable>) (SKL/neighbors/_base.py:121-127 calls it on the (nq, k) distances) for the laws
 * of sknnr_weight_law.  A later call whose opts->weight_law is non-zero must name this law and uses these parameters.
 *   law : SKNNR_LAW_INVERSE .. SKNNR_LAW_EPANECHNIKOV, or SKNNR_LAW_NONE to clear;  p0 finite and > 0;  p1 finite
 * SKNNR_ERR_INVALID for an unknown law or a bad parameter, and -- unless law and parameters are the ones already held --
 * while a stream is open on the handle (its tiles read them).
 */
int sknnr_index_set_weight_law_params(sknnr_index* index, int32_t law, double p0, double p1);

/* Read back sizes: any pointer may be NULL. */
int sknnr_index_shape(const sknnr_index* index, int64_t* n_ref, int32_t* d, int32_t* t,
                      int32_t* d_in, int32_t* device);

int sknnr_get_stats(const sknnr_index* index, sknnr_stats* out);
int sknnr_reset_stats(sknnr_index* index);

/*
 * Poll (and clear) the non-finite-input flag raised by calls made with opts->check_finite = 1 on device
 * memory.  Synchronises `stream` (the stream those calls ran on).  Returns SKNNR_OK or
 * SKNNR_ERR_NONFINITE with scikit-learn's message.  Replaces the finiteness half of
 * validate_data(..., ensure_all_finite=True) (REF transformers/_cca_transformer.py:78-86,
 * SKL/neighbors/_base.py:838-845) for rows that never visit the host.
 */
int sknnr_check_finite(sknnr_index* index, void* stream);

/* ---- the hot path ---------------------------------------------------------------------- */

/*
 * k nearest reference rows of each query row.
 * Replaces RawKNNRegressor.kneighbors (REF _base.py:111-182) = sklearn's
 * KNeighborsMixin.kneighbors (SKL/neighbors/_base.py:763-963) + sknnr's reorder.
 *   q        : (nq, d_in or d) rows of opts->query_dtype (float64 unless set) in `mem`, or NULL with
 *              opts->exclude_self = 1 (the query rows are then the handle's own reference rows)
 *   out_dist : (nq, k) float64 in `mem`, ascending / reordered distances; may be NULL
 *   out_idx  : (nq, k) int64 in `mem`, reference row indices
 *   stream   : hipStream_t to launch on when mem == SKNNR_MEM_DEVICE (NULL = default stream);
 *              ignored for host buffers (the call then returns after the copy-back)
 */
int sknnr_kneighbors(sknnr_index* index, const void* q, int64_t nq,
                     const sknnr_query_opts* opts, double* out_dist, int64_t* out_idx,
                     int32_t mem, void* stream);

/*
 * Weighted multi-output mean of the neighbours' targets.
 * Replaces KNeighborsRegressor.predict (SKL/neighbors/_regression.py:224-268) as reached
 * from REF _base.py:39 (X=None, independent prediction) and :346-348.
 *   out_pred : (nq, t) float64 in `mem`
 *   out_dist, out_idx : optional (nq, k) outputs of the underlying kneighbors (NULL to skip)
 * With opts->weight_mode == SKNNR_WEIGHTS_EXPLICIT use sknnr_predict_from_neighbors instead -- unless opts->weight_law
 * names the handle's distance-weight law: the weights are then law(out_dist) computed on the device (one further launch
 * over nq * k elements into a workspace buffer) and the reduction is the explicit one.  The same holds for
 * sknnr_summarize, sknnr_predict_masked (the law sees the valid rows' distances) and a stream opened with predictions.
 */
int sknnr_predict(sknnr_index* index, const void* q, int64_t nq, const sknnr_query_opts* opts,
                  double* out_pred, double* out_dist, int64_t* out_idx, int32_t mem, void* stream);

/*
 * The reduction alone, from neighbours already found (needed when `weights` is a Python
 * callable: the host evaluates it on the distances and passes w).
 *   dist : (nq, k) or NULL for uniform;  idx : (nq, k);  w : (nq, k) for SKNNR_WEIGHTS_EXPLICIT
 *   k    : at most 192, the largest k of a search (SKNNR_ERR_UNSUPPORTED above)
 * Sums are numpy's, bit for bit: np.sum over k is its pairwise sum (8 partial sums; above 128 terms split at
 * n/2 - (n/2) % 8), and so is the uniform mean of one target; the uniform mean of t >= 2 targets adds the k rows in
 * order.  The result is the float64 value, or the float32 value scikit-learn returns widened exactly.
 */
int sknnr_predict_from_neighbors(sknnr_index* index, const double* dist, const int64_t* idx,
                                 const double* w, int64_t nq, int32_t k, int32_t weight_mode,
                                 double* out_pred, int32_t mem, void* stream);

/* ---- per-target neighbour summaries ------------------------------------------------------------- */

/*
 * One statistic per target column, reduced on the device from the k neighbours of a query in the order sknnr_kneighbors
 * returns them (sknnr_amd/csrc/summary.hip.h; tests/_neighbor_stats.py restates the definitions in numpy).  v_i =
 * y[idx_i, j]; w_i: the weights of sknnr_predict (uniform 1.0; distance 1 / d_i, a row holding d == 0 becomes its 0 / 1
 * mask; explicit as given).  All arithmetic is float64; np_sum is numpy's pairwise sum over the k axis.
 *   MEAN    : the value sknnr_predict gives that column, bit for bit (same kernels)
 *   MODE    : scikit-learn's weighted_mode as KNeighborsClassifier.predict applies it: per distinct label c the vote is
 *             np_sum_i(v_i == c ? w_i : 0.0); the largest vote wins, the smaller label on equal votes; the result is the
 *             label.  Labels are compared as float64 values.  A row whose votes are all zero (explicit weights) gives NaN.
 *   MIN/MAX : of v_i; weights are ignored
 *   NEAREST : v_0
 *   STD     : sqrt(np_sum_i((w_i * (v_i - m)) * (v_i - m)) / np_sum_i(w_i)), m = the float64 weighted mean of that column
 *             as sknnr_predict computes it for float64 targets
 */
enum sknnr_statistic {
    SKNNR_STAT_MEAN = 0,
    SKNNR_STAT_MODE = 1,
    SKNNR_STAT_MIN = 2,
    SKNNR_STAT_MAX = 3,
    SKNNR_STAT_NEAREST = 4,
    SKNNR_STAT_STD = 5
};

/*
 * The reduction alone: sknnr_predict_from_neighbors with a statistic per target.  Same argument rules.
 *   stat : (t) int32 sknnr_statistic codes, HOST memory whatever `mem` is; NULL or an unknown code: SKNNR_ERR_INVALID
 *   out  : (nq, t) float64 in `mem`
 * The MEAN columns come from the predict kernels; the other columns from one further launch (none for an all-MEAN table).
 */
int sknnr_summarize_from_neighbors(sknnr_index* index, const double* dist, const int64_t* idx, const double* w,
                                   int64_t nq, int32_t k, int32_t weight_mode, const int32_t* stat, double* out,
                                   int32_t mem, void* stream);

/* Search plus reduction: sknnr_predict with a statistic per target (stat as above), opts->exclude_self included. */
int sknnr_summarize(sknnr_index* index, const void* q, int64_t nq, const sknnr_query_opts* opts, const int32_t* stat,
                    double* out, double* out_dist, int64_t* out_idx, int32_t mem, void* stream);

/*
 * Debug only.  The last reduction the handle launched (predict or summary entry, one-shot or streamed tile).  Host
 * memory, no device work:
 *   out[0] summary kernel of that reduction: 0 none ran, 1 the register path (k <= 8), 2 the wide path
 *   out[1] rows      out[2] columns the summary kernel handled      out[3] k
 *   out[4] 1 = the predict kernels ran (some column is a mean, or no statistics were given)
 *   out[5] t      out[6] weight mode without its flags      out[7] 0
 */
int sknnr_debug_last_summary(const sknnr_index* index, int64_t out[8]);

/* ---- output plans: many statistics per target from one search --------------------------------- */

/*
 * An output plan is n_out entries (cols[e], stat[e], param[e]), 1 <= n_out <= 1024 (a sanity cap on the row width):
 *   cols[e]  : a target column in [0, t); it may repeat and come in any order
 *   stat[e]  : a sknnr_statistic code, or SKNNR_STAT_QUANTILE
 *   param[e] : float64 parameter, read for SKNNR_STAT_QUANTILE only (0 otherwise)
 * Output plane e of a query holds that statistic of that target over the query's k neighbours, in the order
 * sknnr_kneighbors returns them and with the weights sknnr_predict uses -- all reduced in one pass behind one search
 * (sknnr_amd/csrc/plan.hip.h; tests/_output_plans.py restates the definitions in numpy).  An entry with one of the six
 * sknnr_statistic codes equals that column of sknnr_summarize with that statistic bit for bit (MEAN: the predict
 * kernels' value, float32-target flag included).
 *   QUANTILE : param = q, 0 <= q <= 1 and finite.  numpy's weighted inverted_cdf,
 *              np.quantile(v, q, method="inverted_cdf", weights=w) of numpy >= 2.0:
 *                1. order the k pairs (v_i, w_i) by (v_i, i) ascending (a stable sort by value; -0.0 == 0.0)
 *                2. c_0 = w_(0), c_a = c_(a-1) + w_(a): a sequential float64 running sum in sorted order; total = c_(k-1)
 *                3. cdf_a = c_a / total, one division each
 *                4. the result is v_(a*), a* the first a with cdf_a != 0.0 and cdf_a >= q; k - 1 when there is none
 *                5. total not > 0 (a compact law whose weights all vanish, explicit all-zero weights): NaN, as MEAN
 *              The median is (QUANTILE, 0.5).  The code is kept out of enum sknnr_statistic because the per-target
 *              tables of sknnr_summarize* / sknnr_stream_set_statistics do not take it: they have no parameter.
 */
enum sknnr_plan_statistic { SKNNR_STAT_QUANTILE = 6 };

/*
 * The reduction alone: sknnr_summarize_from_neighbors with an output plan.  Same argument rules.
 *   cols / stat / param : HOST arrays of n_out, whatever `mem` is
 *   out                 : (nq, n_out) float64 in `mem`
 * SKNNR_ERR_INVALID before any device work, the message naming the entry: a NULL array, n_out outside [1, 1024], a column
 * outside [0, t), an unknown code, a q outside [0, 1] or not finite.
 * The predict kernels run (into a buffer of the handle) only if some entry is a MEAN; then one launch writes every entry.
 */
int sknnr_summarize_plan_from_neighbors(sknnr_index* index, const double* dist, const int64_t* idx, const double* w,
                                        int64_t nq, int32_t k, int32_t weight_mode, const int32_t* cols,
                                        const int32_t* stat, const double* param, int32_t n_out, double* out, int32_t mem,
                                        void* stream);

/* Search plus reduction: sknnr_summarize with an output plan; opts->exclude_self and opts->weight_law as there. */
int sknnr_summarize_plan(sknnr_index* index, const void* q, int64_t nq, const sknnr_query_opts* opts, const int32_t* cols,
                         const int32_t* stat, const double* param, int32_t n_out, double* out, double* out_dist,
                         int64_t* out_idx, int32_t mem, void* stream);

/*
 * Debug only.  The plan side of the last reduction the handle launched (the call sknnr_debug_last_summary describes).
 * Host memory, no device work:
 *   out[0] 1 = the plan kernel ran for it (0: a reduction without a plan; the rest is 0 then)
 *   out[1] its path: 1 the register path (k <= 8), 2 the wide path
 *   out[2] rows      out[3] n_out      out[4] k
 *   out[5] entries that are means      out[6] 1 = the predict kernels ran for them      out[7] 0
 */
int sknnr_debug_last_plan(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The weight-law side of the last reduction the handle launched (the call sknnr_debug_last_summary
 * describes), so that a test can prove that the device made the weights.  Host memory, no device work:
 *   out[0] sknnr_weight_law of that reduction (0: none; then out[1 .. 3] describe the reduction all the same)
 *   out[1] rows      out[2] k      out[3] 1 = weight_law_kernel ran for it, 0 = it did not
 *   out[4 .. 7] 0
 */
int sknnr_debug_last_weight_law(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The law kernel alone, no handle: out[e] = law(dist[e]) for n elements with parameters p0, p1; dist and
 * out in `mem` (host: staged; device: on `device`, default stream).  Returns when out is written.  SKNNR_ERR_INVALID for
 * an unknown law (SKNNR_LAW_NONE included), n < 0 and NULL pointers; n == 0 is SKNNR_OK.  The parameters are not
 * checked: the kernel evaluates the expressions as they stand.
 */
int sknnr_debug_weight_law(int32_t law, double p0, double p1, const double* dist, int64_t n, double* out, int32_t mem,
                           int32_t device);

/*
 * Full weighted-Hamming distance rows: out[i, j] = distance between query row rows[i] and reference row j, in the
 * reference's float64 arithmetic (sknnr_formula, SKNNR_FORMULA_HAMMING) -- the matrix the reference's brute search
 * materialises chunk by chunk (SKL/neighbors/_base.py:896-926, pairwise_distances_chunked) before
 * _kneighbors_reduce_func (SKL/neighbors/_base.py:733-760) runs np.argpartition over each row.  For the rows whose
 * k-th distance is tied the caller can thus make numpy's own selection (REF tests/test_regressions.py:125-195 pin it).
 *   q    : (nq, d) float64 node ids in `mem`, or NULL: the handle's reference rows (the X=None path)
 *   rows : (n_rows) int64 in `mem`: which rows of q; NULL: rows 0 .. n_rows - 1
 *   out  : (n_rows, n_ref) float64 in `mem`
 */
int sknnr_hamming_distances(sknnr_index* index, const double* q, int64_t nq, const int64_t* rows, int64_t n_rows,
                            double* out, int32_t mem, void* stream);

/* ---- leave-group-out neighbours ---------------------------------------------------------------- */

/*
 * Independent predictions that skip groups.  The reference's independent_prediction_ (REF _base.py:37-40) leaves out
 * each fitted row itself; that is independent only when every row is its own sampling unit.  Re-measured plots,
 * clusters of subplots and spatial blocks need every fitted row answered from the rows of OTHER groups.  The reference
 * has no such call; the contract, stated here once (sknnr_amd/csrc/groups.hip.h; tests/_groups.py restates it in numpy):
 *
 *   codes is an int32 label per reference row, k = opts->n_neighbors.  For reference row i the candidates are the rows
 *   r with codes[r] != codes[i]; row i itself is therefore never a candidate.  Each pair has a value: the float64
 *   number sknnr_kneighbors ranks the pair (row i, row r) by under opts->formula -- EXPANDED: |x|^2 - 2 x.r + |r|^2
 *   clamped at 0; DIRECT: sum (x - r)^2; HAMMING: the weighted Hamming distance.  The answer of row i:
 *     1. the k candidates smallest by (value, r), ascending in that order
 *     2. distances: sqrt(value) for the two Euclidean formulas, the value itself for HAMMING
 *     3. with opts->deterministic, sknnr's reorder (REF _base.py:166-175), row number i, scale over the k kept distances
 *   under all three formulas alike.  There is NO replay of scikit-learn's heap history: exact ties at the k-th value go
 *   to the lower index.  With every row in a group of its own the result equals sknnr_kneighbors with q = NULL bit for
 *   bit on every row whose k-th and (k+1)-th smallest values among the other rows differ.
 *
 * sknnr_index_set_groups: codes HOST, n == n_ref, every code >= 0 (else SKNNR_ERR_INVALID); NULL clears.  Copied to the
 *   device and kept on the handle, like the Hamming weights.
 * sknnr_kneighbors_grouped: rows [opts->row_offset, opts->row_offset + nq) of the reference set, by the contract above.
 *   Reads n_neighbors, deterministic, decimals, formula and row_offset; exclude_self must be 1 (the rows are reference
 *   rows), apply_affine and query_dtype 0.  out_dist / out_idx / mem / stream as for sknnr_kneighbors; out_dist may be
 *   NULL.  One float64 scan (group_scan_kernel), counted in sknnr_stats.queries and exact_only_queries.  Refused before
 *   any launch: no groups set (nor a buffer, below) or a window outside [0, n_ref] (SKNNR_ERR_INVALID); n_neighbors > n_ref - largest group
 *   (SKNNR_ERR_K_TOO_LARGE: some row would have fewer candidates than neighbours); n_neighbors > 192
 *   (SKNNR_ERR_UNSUPPORTED).  Rows of any width are served (beyond 1024 columns in column chunks, like the exact scan).
 */
int sknnr_index_set_groups(sknnr_index* index, const int32_t* codes, int64_t n);
int sknnr_kneighbors_grouped(sknnr_index* index, int64_t nq, const sknnr_query_opts* opts, double* out_dist,
                             int64_t* out_idx, int32_t mem, void* stream);

/*
 * Debug only.  The leave-group-out scan of the last search call (zeroed by every search call).  Host memory, no device work:
 *   out[0] 0 = no grouped scan ran, else formula + 1      out[1] k      out[2] workgroups      out[3] dynamic LDS bytes
 *   out[4] rows      out[5] slices (1 = none)      out[6] rows of the largest group      out[7] number of groups
 */
int sknnr_debug_last_grouped(const sknnr_index* index, int64_t out[8]);

/* ---- buffered leave-out ------------------------------------------------------------------------ */

/*
 * Independent neighbours that skip nearby plots: "predict plot i from the plots farther than R from it".  "Within R" is
 * no equivalence relation, so no group labelling encodes it; it is a second mask of sknnr_kneighbors_grouped.  The
 * contract, stated here once (sknnr_amd/csrc/groups.hip.h and buffer.hip.h; tests/_buffer.py restates it in numpy):
 *
 *   coords is an (n_ref, c) float64 array of plot positions, c = 1, 2 or 3, every value finite; radius is a finite
 *   float64 >= 0; r2 = radius * radius, one float64 multiplication.  For reference rows i and r
 *     g(i, r) = ((x_i - x_r)*(x_i - x_r) + (y_i - y_r)*(y_i - y_r)) + (z_i - z_r)*(z_i - z_r)
 *   every operation a separately rounded float64 operation (no fused multiply-add).  A missing column counts as 0 for
 *   both rows: it adds +0.0, so c < 3 gives the bits of the shorter sum.  Row r is EXCLUDED for row i when
 *   g(i, r) <= r2 and, with group codes set as well, also when codes[r] == codes[i].  g(i, i) = 0 <= r2 always: a row is
 *   never its own candidate, and radius = 0 excludes exactly the co-located rows.  Everything else is the
 *   leave-group-out contract above, unchanged: the candidates' values under opts->formula, the k smallest by
 *   (value, index), sqrt (not for HAMMING), sknnr's reorder when asked for, exact ties at the k-th value to the lower
 *   index, no replay of scikit-learn's heap history.
 *   excluded[i] is the number of rows excluded for row i, itself included: row i has n_ref - excluded[i] candidates.
 *
 * sknnr_index_set_buffer: coords HOST, row-major (n, c); NULL clears the buffer.  SKNNR_ERR_INVALID for n != n_ref, c
 *   outside 1..3, a position that is not finite, a radius that is negative or not finite.  The positions are copied to
 *   the device as (3, n_ref) and kept on the handle with the radius, like the group codes.
 * sknnr_kneighbors_grouped runs when groups, a buffer or both are set (with neither: its error above).  With a buffer it
 *   is refused before the scan is launched when n_neighbors > n_ref - max(excluded) (SKNNR_ERR_K_TOO_LARGE; the message
 *   names max(excluded) and the first row that attains it); with groups alone max(excluded) is the largest group, the
 *   test and its message above.  excluded[] is counted on the device (buffer_count_kernel, a sweep over the positions
 *   and the codes that never reads the feature rows) once per change of either mask and cached on the handle.
 * sknnr_buffer_counts: excluded[] under the masks now set (groups, a buffer or both; SKNNR_ERR_INVALID with neither),
 *   (n_ref) int64 in `mem`; mem / stream as for sknnr_kneighbors.
 */
int sknnr_index_set_buffer(sknnr_index* index, const double* coords, int64_t n, int32_t c, double radius);
int sknnr_buffer_counts(sknnr_index* index, int64_t* out, int32_t mem, void* stream);

/*
 * Debug only.  The masks of the leave-out scan of the last search call (zeroed by every search call).  Host memory, no
 * device work:
 *   out[0] 0 = no grouped scan ran, else the mask mode: 1 groups, 2 buffer, 3 both      out[1] c (0 without a buffer)
 *   out[2] max(excluded)      out[3] min(excluded)      out[4] workgroups of the count launch      out[5] its LDS bytes
 *   out[6] the first row that attains max(excluded)      out[7] 0
 * out[2] .. out[6] describe the counts cached on the handle.  A groups-only search never counts: unless
 * sknnr_buffer_counts did since the masks last changed, out[2] is the largest group and out[3] .. out[6] are 0.
 */
int sknnr_debug_last_buffer(const sknnr_index* index, int64_t out[8]);

/* ---- reference-sharded search ------------------------------------------------------------------ */

/*
 * When the REFERENCE rows are split over several handles (several GPUs), every shard answers every query row and the
 * per-shard answers are merged -- SURVEY.md section 8e, "alternative"; the reference's analogue is scikit-learn's
 * parallel-on-Y strategy: per-thread heaps over chunks of Y, then _parallel_on_Y_synchronize
 * (SKL/metrics/_pairwise_distances_reduction/_argkmin.pyx.tp:200-261), reached from REF _base.py:162-164.
 *
 * sknnr_shard_candidates: the n_neighbors nearest rows of THIS handle's reference rows (a shard) as raw candidates:
 *   out_val (nq, n_neighbors) the formula's values -- squared distances (expanded / direct), the Hamming distance --
 *   ascending by (value, index); out_idx the shard's row indices + index_offset (the shard's first row in the whole
 *   reference set).  No self exclusion (exclude_self must be 0: for the X=None path ask for n_neighbors + 1 and let
 *   the merge drop the row itself), no square root, no reorder.  The shard must hold at least n_neighbors rows.
 *
 * sknnr_merge_shards: the ranks' candidate arrays, gathered -- shard_val / shard_idx (n_shards, nq, kk), kk =
 *   n_neighbors + exclude_self, shard g's block at [g] -- merged into the call's final answer exactly as
 *   sknnr_kneighbors gives it (smallest (value, index) first, X=None drop, square root, sknnr's reorder).  `index` is a
 *   handle over ALL reference rows (every rank holds the small float64 copy; the shards split the sweep): a row whose
 *   merged answer is not unique -- an exact tie across the last slot, which the reference's heap settles by its
 *   history -- is re-scanned in float64 over all rows on this handle, the same replay of the reference's engine that
 *   sknnr_kneighbors uses for tied rows, so that a sharded call returns what the unsharded call returns.
 *   q / opts as for sknnr_kneighbors (q NULL with exclude_self = 1: the rows are reference rows [row_offset, +nq)).
 */
int sknnr_shard_candidates(sknnr_index* index, const double* q, int64_t nq, const sknnr_query_opts* opts,
                           int64_t index_offset, double* out_val, int64_t* out_idx, int32_t mem, void* stream);
int sknnr_merge_shards(sknnr_index* index, const double* q, int64_t nq, const sknnr_query_opts* opts, int32_t n_shards,
                       const double* shard_val, const int64_t* shard_idx, double* out_dist, int64_t* out_idx,
                       int32_t mem, void* stream);

/* ---- streamed query tiles (raster ingestion) ------------------------------------------------ */

/*
 * Wall-to-wall mapping feeds the hot path tile by tile: the reference's documented workflow predicts
 * plot IDs / attributes for every pixel of a raster (REF docs/pages/usage.md:101-128, README.md:66-67),
 * i.e. calls kneighbors(X_tile, return_dataframe_index=True) / predict(X_tile) once per block of pixels.
 * A stream keeps the handle's three-stream PCIe pipeline (copy-in | kernels | copy-out) full ACROSS
 * those calls and carries the global row offset itself, so that N pushes give bit for bit what one call
 * on the concatenated rows gives (key 2 of the reorder, REF _base.py:171, counts rows over the whole
 * logical call).
 *
 *   begin : opts as for sknnr_kneighbors / sknnr_predict (exclude_self must be 0); opts->row_offset is
 *           the global row of the first pushed row.  want_dist / want_pred say which optional outputs
 *           later pushes may ask for.  One open stream per handle; host-memory kneighbors/predict
 *           calls on the handle fail while it is open (device-memory calls are allowed).
 *   push  : q is a HOST (nq, d_in or d) tile of the stream's opts->query_dtype and may be reused as soon as the call returns.  The
 *           tile's results are written to the HOST buffers passed with it -- out_idx (nq, k), out_dist
 *           (nq, k) or NULL, out_pred (nq, t) or NULL -- at the latest when a flush or end returns (earlier in
 *           practice: a tile leaves its pipeline slot when the slot is needed again, four tiles later);
 *           the buffers must stay valid until then.
 *   flush : every pushed tile's results are in place on return.  With opts->check_finite the status
 *           is SKNNR_ERR_NONFINITE if any pushed value was NaN or infinite.
 *   end   : flush, then free the stream (NULL is allowed); *rows_pushed (optional) = total rows.
 * A stream refers to its index: end it before sknnr_index_destroy.
 */
typedef struct sknnr_stream sknnr_stream;
int sknnr_stream_begin(sknnr_index* index, const sknnr_query_opts* opts, int32_t want_dist, int32_t want_pred,
                       sknnr_stream** out);
int sknnr_stream_push(sknnr_stream* stream, const void* q, int64_t nq, double* out_dist, int64_t* out_idx,
                      double* out_pred);
int sknnr_stream_flush(sknnr_stream* stream);
int sknnr_stream_end(sknnr_stream* stream, int64_t* rows_pushed);

/* ---- nodata rows (raster masks) ------------------------------------------------------------ */

/*
 * Real rasters carry nodata: pixels outside the study area, cloud and water masks, per-band sentinels such as -32768 or
 * 255.  The reference has no notion of them; its user drops those pixels first -- valid = (X != nodata).all(1);
 * est.kneighbors(X[valid]) -- and scatters the answers back.  The entry points below do the three steps on the device
 * (sknnr_amd/csrc/mask.hip.h): mask, stable compaction, the ordinary search on the packed rows, expansion.
 *
 *   nodata : HOST, (d_in) float64, one value per RAW input column (the columns the call reads, before any affine map or
 *            forest map).  A row is masked when any column, widened exactly to float64, equals its nodata value; a NaN
 *            entry means "NaN in that column is nodata".
 *   Valid rows are answered exactly as the unmasked call answers X[valid], bit for bit; row positions (key 2 of the
 *   reorder, REF _base.py:171) count valid rows only, over the whole logical call.
 *   Masked rows get fill_index in out_idx and NaN in out_dist / out_pred.  They are not tested for finiteness and cost
 *   no search work (sknnr_stats.queries grows by the valid rows only).
 *
 * sknnr_mask_rows: the mask alone, no handle.  q (nq, d_in) rows of query_dtype and out_valid (nq) uint8, 1 = valid, in
 *   `mem` on `device`; *out_n_valid (host) the number of valid rows.  Returns when both are written.
 * sknnr_kneighbors_masked / sknnr_predict_masked: the arguments of sknnr_kneighbors / sknnr_predict plus nodata,
 *   fill_index and *out_n_valid (host, optional).  q must be given and opts->exclude_self must be 0.  The host reads the
 *   valid count (one 8-byte copy) before it enqueues the search, so device-memory calls synchronise `stream` once; a
 *   fully valid tile is searched in place, a fully masked one only filled.  The sharded entry points take no mask.
 * sknnr_stream_set_nodata: allowed only before the first push (SKNNR_ERR_INVALID afterwards).  Every pushed tile is
 *   then masked behind its host-to-device copy, and the stream carries the running count of VALID rows as the row
 *   offset.  Results reach the host in full layout, fills included.  sknnr_stream_end's rows_pushed stays the pushed
 *   rows; sknnr_stream_valid_rows gives the valid ones submitted so far.
 */
int sknnr_mask_rows(const void* q, int64_t nq, int32_t d_in, int32_t query_dtype, const double* nodata, int32_t device,
                    int32_t mem, void* stream, uint8_t* out_valid, int64_t* out_n_valid);
int sknnr_kneighbors_masked(sknnr_index* index, const void* q, int64_t nq, const sknnr_query_opts* opts,
                            const double* nodata, int64_t fill_index, double* out_dist, int64_t* out_idx, int32_t mem,
                            void* stream, int64_t* out_n_valid);
int sknnr_predict_masked(sknnr_index* index, const void* q, int64_t nq, const sknnr_query_opts* opts,
                         const double* nodata, int64_t fill_index, double* out_pred, double* out_dist, int64_t* out_idx,
                         int32_t mem, void* stream, int64_t* out_n_valid);
int sknnr_stream_set_nodata(sknnr_stream* stream, const double* nodata, int64_t fill_index);

/*
 * sknnr_stream_set_statistics: the stream's predictions become per-target summaries (enum sknnr_statistic): stat is a
 * HOST array of t codes, t the handle's number of targets.  Allowed after sknnr_stream_begin and before the first push;
 * SKNNR_ERR_INVALID on a stream opened without predictions, after a push, or with another t.  The summary is written
 * where the prediction is: masked rows, band-first results and typed outputs treat it alike.  A stream without this call
 * (or with an all-MEAN table) enqueues exactly what it did before.
 */
int sknnr_stream_set_statistics(sknnr_stream* stream, const int32_t* stat, int32_t t);
/*
 * sknnr_stream_set_plan: the stream's predictions become the n_out planes of an output plan (cols / stat / param: HOST
 * arrays, as sknnr_summarize_plan).  Allowed after sknnr_stream_begin and before the first push, on a stream opened with
 * predictions, and before a sknnr_stream_set_output that gives a scale / offset; mutually exclusive with
 * sknnr_stream_set_statistics (whichever comes second is SKNNR_ERR_INVALID).  From then on the prediction lane has n_out
 * columns: sknnr_stream_push* expect out_pred of (nq, n_out), the band-first pushes n_out planes, and
 * sknnr_stream_set_output's pred_scale / pred_offset hold one value per output plane.  Masked rows are NaN (or the fill)
 * across all n_out planes.
 */
int sknnr_stream_set_plan(sknnr_stream* stream, const int32_t* cols, const int32_t* stat, const double* param, int32_t n_out);
int sknnr_stream_valid_rows(const sknnr_stream* stream, int64_t* out_valid_rows);

/* ---- band-first tiles (raster layouts) ------------------------------------------------------ */

/*
 * Raster readers deliver a window as (bands, h, w) and raster writers want (targets, h, w); every search kernel reads
 * packed (n, bands) rows and writes (n, k) / (n, t) rows.  The entry points below do both transpositions on the device
 * (sknnr_amd/csrc/planes.hip.h), so that no strided pass over a tile is left to the host.
 *
 * sknnr_planes_to_rows: no handle.  src holds c planes of n elements of elem_bytes (1, 2, 4 or 8) each, plane j starting
 *   j * src_stride ELEMENTS after src (src_stride >= n); dst receives the packed (n, c) rows.  Both are DEVICE memory on
 *   `device`, at any address that is a multiple of elem_bytes.  A raw byte move: no value is widened or looked at.
 * sknnr_rows_to_planes: the reverse for 8-byte elements (int64 indices, float64 distances and predictions): src packed
 *   (n, c) rows, plane j of dst starting j * dst_stride elements after dst (dst_stride >= n).
 *   Both enqueue on `stream` and return; c in [1, 65536], n below 2^31.  SKNNR_ERR_INVALID, before any device call, for
 *   elem_bytes outside {1, 2, 4, 8}, n < 0, c < 1, a stride below n and NULL pointers; n == 0 is SKNNR_OK.
 * sknnr_stream_push_planes: sknnr_stream_push for a band-first tile.  planes: HOST array of d_in (or d) HOST pointers,
 *   each to nq contiguous elements of the stream's opts->query_dtype (the bands may be separate arrays); the array and the
 *   bands may be reused as soon as the call returns.  Results are band-first too: neighbour j of the tile starts at
 *   out_idx + j * out_stride (out_dist likewise), target j at out_pred + j * out_stride; out_stride >= nq elements.
 *   The tile is staged with one plain copy per band, transposed behind its host-to-device copy (in front of the nodata
 *   mask, where one is set), searched exactly as a row tile is, and its results are transposed before they leave the
 *   device: bit for bit the rows sknnr_stream_push gives for the transposed tile.  Buffer lifetime, flush / end,
 *   check_finite, sknnr_stream_set_nodata and the row offset are as for sknnr_stream_push.  A stream may mix both kinds
 *   of push: each tile's results come in the layout of its own push, and row positions run on across them.
 */
int sknnr_planes_to_rows(const void* src, int64_t n, int32_t c, int32_t elem_bytes, int64_t src_stride, void* dst,
                         int32_t device, void* stream);
int sknnr_rows_to_planes(const void* src, int64_t n, int32_t c, void* dst, int64_t dst_stride, int32_t device,
                         void* stream);
int sknnr_stream_push_planes(sknnr_stream* stream, const void* const* planes, int64_t nq, double* out_dist,
                             int64_t* out_idx, double* out_pred, int64_t out_stride);

/* ---- typed outputs (rasters stored as int16 / uint8 / float32 / int32) -------------------------- */

/*
 * Output rasters are stored narrow, with a scale factor and a nodata value; plot-id rasters are int32.  The entry points
 * below convert a result tile to that type ON THE DEVICE (sknnr_amd/csrc/narrow.hip.h), so that only the narrow bytes
 * cross PCIe and are copied on the host.  The conversions, exactly (tests/_narrow.py restates them in numpy):
 *   values (float64) -> SKNNR_DTYPE_F32: x = v, or x = v * scale[j] + offset[j] for column j, as two float64 roundings
 *     (never a fused multiply-add); NaN gives (float)fill when a fill is set; else the C cast, round to nearest even:
 *     overflow gives +-inf, NaN stays NaN, and without scale / offset -0.0 keeps its sign.
 *   values -> SKNNR_DTYPE_I16 / U16 / U8 / I32: x as above; NaN is tested FIRST and gives fill (0 when no fill is set:
 *     set one wherever NaN can occur); otherwise rint(x), half to even, then the clamp to the type's [min, max] -- so
 *     +-inf clamp -- then the cast.  The clamp does NOT avoid the fill value: a valid pixel may come to equal it.
 *   indices (int64) -> SKNNR_DTYPE_I32: plain narrowing; the caller guarantees that every index (and fill_index) fits.
 *
 * sknnr_narrow: no handle.  src: DEVICE memory, a packed (n, c) tile of float64 (kind SKNNR_NARROW_VALUE) or int64
 *   (SKNNR_NARROW_INDEX).  dst: DEVICE memory of dst_dtype elements, at any element-aligned address: packed (n, c) rows
 *   when dst_stride == 0, else c planes of n elements, plane j starting j * dst_stride ELEMENTS after dst (dst_stride
 *   >= n) -- transposed and converted in one pass.  scale / offset: DEVICE arrays of c float64 each, or both NULL.
 *   has_fill / fill: the value NaN becomes; it must be representable in dst_dtype.  Enqueues on `stream` and returns;
 *   *out_wide (optional) = 1 when the launch converted 4 destination elements per lane -- chosen from the addresses, the
 *   stride and the count -- 0 for one element per lane.  c in [1, 65536], n below 2^31.  SKNNR_ERR_INVALID, before any
 *   device call, for an unknown or impossible (kind, dst_dtype) pair, n < 0, c out of range, a non-zero stride below n,
 *   scale without offset (or either, or a fill, with indices), a fill that dst_dtype cannot hold, and NULL src / dst;
 *   n == 0 is SKNNR_OK.
 * sknnr_stream_set_output: the element types in which a stream's results leave the device.  0 (SKNNR_DTYPE_F64) means
 *   "as ever" for that output (int64 indices, float64 distances and predictions); idx_dtype accepts 0 or I32,
 *   dist_dtype 0 or F32, pred_dtype 0 or F32 / I16 / U16 / U8 / I32.  pred_scale / pred_offset: HOST arrays of t float64
 *   each (n_out each on a stream with an output plan, sknnr_stream_set_plan; both or neither), uploaded once; has_pred_fill / pred_fill: what a NaN prediction (a nodata row) becomes.
 *   Allowed only before the first push.  A stream on which it was never called enqueues exactly what it did before the
 *   entry point existed.
 * sknnr_stream_push_typed / sknnr_stream_push_planes_typed: sknnr_stream_push / sknnr_stream_push_planes with the
 *   outputs as void*: HOST arrays of the types set by sknnr_stream_set_output ((nq, k) / (nq, t), or planes out_stride
 *   ELEMENTS of the output's own type apart).  On a stream without typed outputs they are the plain pushes; the plain
 *   pushes, whose signatures promise int64 / float64, return SKNNR_ERR_INVALID on a stream with typed outputs.  The
 *   conversion runs behind the search, the reduction, the nodata expansion (so fill_index is already in the tile) and in
 *   the transposition's place; device-to-host copies, pinned buffers and the host copy move nq * cols * sizeof(type).
 *
 * Dataframe ids on the device.  A plot-id raster holds the ids of the reference rows, not their positions; the index
 * conversion looks them up on its way out, so that the host never walks the output again:
 *   indices (int64) with an id table -> v < 0 ? fill_id : table[v], tested on the source value BEFORE the load, then
 *     the plain narrowing to SKNNR_DTYPE_I32 (the caller guarantees that every table entry and fill_id fits) or, for
 *     dst_dtype 0, no narrowing: int64 ids, lookup only, in the same single pass (tests/_id_table.py restates it).
 * sknnr_narrow_ids: sknnr_narrow for index tiles with a lookup; no handle, every pointer DEVICE memory.  src: packed
 *   (n, c) int64; table: n_table int64; dst / dst_stride as for sknnr_narrow, dst_dtype 0 (int64) or SKNNR_DTYPE_I32.
 *   has_fill / fill_id: what a negative source value becomes; without has_fill it passes through unchanged.  A
 *   NON-NEGATIVE source value at or above n_table is a caller error that the kernel does not test for: it reads
 *   outside the table.  *out_wide as for sknnr_narrow (an int64 destination takes the wide path when it is 32-byte
 *   aligned).  SKNNR_ERR_INVALID, before any device call, for a NULL table, n_table < 1, another dst_dtype, and the
 *   cases sknnr_narrow refuses (n < 0, c out of range, a non-zero stride below n, NULL src / dst); n == 0 is SKNNR_OK.
 * sknnr_stream_set_id_table: table is a HOST array of n_table int64, uploaded once; n_table must be the handle's number
 *   of reference rows.  Allowed only before the first push (SKNNR_ERR_INVALID afterwards, and for another n_table).
 *   From then on the index output of every tile leaves through the conversion kernel with the table -- int64 or, with
 *   idx_dtype SKNNR_DTYPE_I32, int32; rows or planes; masked or not -- and holds ids.  The fill_index of
 *   sknnr_stream_set_nodata stays what the nodata expansion writes into the tile: pass a negative one (-1), and the
 *   lookup gives those pixels fill_id.  A stream on which it is never called enqueues exactly what it did before the
 *   entry point existed.
 */
#define SKNNR_NARROW_VALUE 0
#define SKNNR_NARROW_INDEX 1
int sknnr_narrow(const void* src, int32_t kind, int64_t n, int32_t c, void* dst, int32_t dst_dtype, int64_t dst_stride,
                 const double* scale, const double* offset, int32_t has_fill, double fill, int32_t device, void* stream,
                 int32_t* out_wide);
int sknnr_stream_set_output(sknnr_stream* stream, int32_t idx_dtype, int32_t dist_dtype, int32_t pred_dtype,
                            const double* pred_scale, const double* pred_offset, int32_t has_pred_fill,
                            double pred_fill);
int sknnr_narrow_ids(const int64_t* src, int64_t n, int32_t c, const int64_t* table, int64_t n_table, int32_t has_fill,
                     int64_t fill_id, void* dst, int32_t dst_dtype, int64_t dst_stride, int32_t device, void* stream,
                     int32_t* out_wide);
int sknnr_stream_set_id_table(sknnr_stream* stream, const int64_t* table, int64_t n_table, int64_t fill_id);
int sknnr_stream_push_typed(sknnr_stream* stream, const void* q, int64_t nq, void* out_dist, void* out_idx,
                            void* out_pred);
int sknnr_stream_push_planes_typed(sknnr_stream* stream, const void* const* planes, int64_t nq, void* out_dist,
                                   void* out_idx, void* out_pred, int64_t out_stride);

/* ---- neighbour usage (which reference rows made the map) ---------------------------------------- */

/*
 * Neighbour usage.  THE CONTRACT, stated here once (sknnr_amd/csrc/tally.hip.h implements it, tests/_usage.py restates it
 * in numpy).  For one or more tallied searches over a handle with n_ref reference rows and k neighbours:
 *   counts[r, j]  int64, (n_ref, k), C order: the number of tallied query rows whose j-th returned neighbour is reference
 *                 row r; j is the position in the returned row, after sknnr's reorder when the call uses it.
 *   max_dist[r]   float64, (n_ref): the largest returned distance at which r was anybody's neighbour, at any rank.  A
 *                 distance that is not > 0 (0.0, -0.0, NaN) counts as +0.0.  A row never used holds 0.0: its counts say so.
 * Rows masked by nodata contribute nothing.  In the from-neighbours form an entry < 0 or >= n_ref is never dereferenced:
 * it is skipped and counted in the debug record (a whole row may go that way: a fill row is all negative).  The tally is
 * over ROW INDICES, never dataframe ids, and is unaffected by the id table, the typed outputs, the band layout, the
 * statistics or the plan of the same stream.  The results do not depend on launch geometry, tile cuts or arrival order:
 * counts are integer adds, and the maximum is taken on the distances' bit patterns as unsigned 64-bit integers -- valid
 * because they are non-negative and never NaN after the rule above -- so two runs are bit-equal.  Sums of prediction
 * weights are deliberately absent: a float atomic sum depends on arrival order.
 * n_ref * k must be below 2^32 (the kernel's keys are 32 bits): SKNNR_ERR_UNSUPPORTED otherwise, before any device work.
 *
 * sknnr_tally_from_neighbors: idx (nq, k) int64 and dist (nq, k) float64 as a search returned them; counts / max_dist as
 *   above; all in `mem` (host arrays are staged; device arrays are used in place, enqueued on `stream`).  dist and
 *   max_dist may both be NULL: counts only.  accumulate = 0 zeroes the outputs first; accumulate = 1 adds to what they
 *   hold, max_dist being read back through the same rule (a value that is not > 0 is +0.0).  nq == 0 is allowed.
 * sknnr_stream_set_tally: allowed only before the first push.  Allocates and zeroes the two accumulators for the
 *   stream's k on the handle.  From then on the stream keeps the search's distances even when no distance or prediction
 *   leaves, and every tile is tallied on the device behind its search: the whole tile, or with sknnr_stream_set_nodata
 *   its valid rows (never the expanded rows: fill_index need not be negative).  What the pushes deliver is unchanged,
 *   bit for bit.  A stream on which it is never called enqueues exactly what it did before the entry point existed.
 * sknnr_stream_get_tally: flushes the pipeline (as sknnr_stream_flush) and copies the accumulators to HOST arrays
 *   (either may be NULL).  May be called more than once; the accumulators keep running.
 * sknnr_debug_last_tally: debug only; synchronises the device.  The last sknnr_tally_from_neighbors call, or -- after
 *   sknnr_stream_set_tally -- the stream so far:
 *   out[0] 1 = a tally kernel ran          out[1] rows given to it          out[2] k
 *   out[3] entries tallied                 out[4] entries skipped (outside [0, n_ref))
 *   out[5] global atomics issued on the accumulators
 *   out[6] entries that found no slot in their workgroup's table and went to the accumulators directly
 *   out[7] slots of a workgroup's table
 */
int sknnr_tally_from_neighbors(sknnr_index* index, const double* dist, const int64_t* idx, int64_t nq, int32_t k,
                               int64_t* counts, double* max_dist, int32_t accumulate, int32_t mem, void* stream);
int sknnr_stream_set_tally(sknnr_stream* stream);
int sknnr_stream_get_tally(sknnr_stream* stream, int64_t* counts, double* max_dist);
int sknnr_debug_last_tally(const sknnr_index* index, int64_t out[8]);

/* ---- zonal statistics (summaries of the map over stands, ownerships, counties ...) ---------------- */

/*
 * Zonal statistics.  THE CONTRACT, stated here once (sknnr_amd/csrc/zonal.hip.h implements it, tests/_zonal.py restates
 * it in numpy).  Inputs per tallied tile: a float64 value tile (n, c) -- the prediction lane as computed: c = t targets, or
 * the n_out planes of an output plan; zones (n) int32; and the prediction lane's conversion: an integer dst_dtype
 * (SKNNR_DTYPE_I16 / U16 / U8 / I32) with per-column scale / offset or neither.
 * For pixel i, column j: q = the typed output's stored value of v[i, j] (x = v * scale[j] + offset[j] as two roundings,
 * rint, clamp, cast: "typed outputs" above, the same device function) WITHOUT the fill.  NaN is tested first, on v: a NaN
 * entry contributes nothing -- a nodata pixel, counted in the record -- whatever fill the stream has, and even though a
 * valid pixel's stored value may come to equal the fill.  (A v that is not NaN whose x is -- inf * 0 -- stores 0.)
 * A zone code < 0 or >= n_zones skips the whole pixel: counted in the record, never dereferenced, and its entries are
 * counted neither as tallied nor as NaN.
 * Accumulators, all int64, C order:
 *   acc[z, j, 0..5]  (n_zones, c, 6): count, sum = sum of q, sq_lo = sum of (q^2 mod 2^32), sq_hi = sum of (q^2 >> 32),
 *                    min, max.  The sum of squares is sq_hi * 2^32 + sq_lo: exact for every accepted type up to 2^31
 *                    pixels per zone (int32 outputs make the two limbs necessary).  min / max start at INT64_MAX /
 *                    INT64_MIN and stay there where count == 0.
 *   hist             for every column j with n_classes[j] > 0 (a class plane, e.g. a `mode` statistic) a block
 *                    (n_zones, n_classes[j]); the blocks are concatenated in column order.  hist_j[z, q] counts the
 *                    pixels with 0 <= q < n_classes[j]; a q outside that range is counted in the record as "other".
 *                    Numeric columns have n_classes[j] == 0 and no block; class planes also get their acc entries.
 * Every accumulator is an integer add, min or max: the results do not depend on launch geometry, tile cuts or arrival
 * order, two runs produce the same bytes, and they equal what a zonal-statistics tool computes from the written raster.
 * Sums of the float predictions are deliberately absent: a float atomic sum depends on arrival order.
 * Refused with SKNNR_ERR_UNSUPPORTED before any device work: n_zones * c >= 2^32, and n_zones * max(n_classes) >= 2^32
 * (the kernel's keys are 32 bits); and n_zones > 2^31 - 1 with c == 1 (zone codes are int32).
 *
 * sknnr_zonal_from_values: one-shot.  values (n, c), zones (n), acc and hist live in `mem` (host arrays are staged; device
 *   arrays are used in place, enqueued on `stream`); scale, offset (c each, or both NULL) and n_classes (c, or NULL: no
 *   class planes) are always HOST arrays.  accumulate = 0 initialises acc / hist first, the min / max sentinels included;
 *   accumulate = 1 adds to what they hold.  hist may be NULL when no column has classes.  n == 0 is allowed.  The handle
 *   gives the record and the staging buffers only: neither its rows nor its targets are read.
 * sknnr_stream_set_zonal: allowed only before the first push, on a stream opened with predictions, and after
 *   sknnr_stream_set_plan when there is a plan (n_classes holds one value per column of the prediction lane, or is NULL).
 *   Allocates and initialises the accumulators on the handle.  From then on every tile's float64 prediction tile -- the
 *   full layout, where masked rows are NaN -- is tallied on the device behind its reduction, whether or not the push asks
 *   for the predictions, for row, plane and typed pushes alike.  What the pushes deliver is unchanged, bit for bit.  A
 *   stream on which it is never called enqueues exactly what it did before the entry point existed.
 * sknnr_stream_next_zones: a HOST int32 array, reusable on return, holding the zone codes of the NEXT push: one plane,
 *   in pixel order, in either layout.  A push on a zonal stream without it, or with another nq than it gave, is
 *   SKNNR_ERR_INVALID, and so is a prediction lane without an integer pred_dtype (sknnr_stream_set_output) at the push.
 *   nq == 0 is accepted and ignored, as a push of no rows is.
 * sknnr_stream_get_zonal: flushes the pipeline (as sknnr_stream_flush) and copies the accumulators to HOST arrays (either
 *   may be NULL; hist only where a column has classes).  May be called more than once; the accumulators keep running.
 * sknnr_debug_last_zonal: debug only; synchronises the device.  The last sknnr_zonal_from_values call, or -- after
 *   sknnr_stream_set_zonal -- the stream so far:
 *   out[0] 1 = a zonal kernel ran          out[1] pixels given to it        out[2] c
 *   out[3] entries tallied                 out[4] NaN entries               out[5] pixels outside [0, n_zones)
 *   out[6] class values outside [0, n_classes[j])
 *   out[7] global atomics issued on the accumulators.  (The kernels' sixth counter, entries that found no slot in their
 *          workgroup's table and went to the accumulators directly, does not fit eight words: such entries show here,
 *          five or six atomics each, beyond what a flush of every slot can issue.)
 * sknnr_debug_zonal_geometry: no device work.  out[0] pixels a workgroup takes at c columns, out[1] slots of its table,
 *   out[2] slots of its class table, out[3] slots an entry probes.
 */
int sknnr_zonal_from_values(sknnr_index* index, const double* values, const int32_t* zones, int64_t n, int32_t c,
                            int32_t dst_dtype, const double* scale, const double* offset, int64_t n_zones,
                            const int32_t* n_classes, int64_t* acc, int64_t* hist, int32_t accumulate, int32_t mem,
                            void* stream);
int sknnr_stream_set_zonal(sknnr_stream* stream, int64_t n_zones, const int32_t* n_classes);
int sknnr_stream_next_zones(sknnr_stream* stream, const int32_t* zones, int64_t nq);
int sknnr_stream_get_zonal(sknnr_stream* stream, int64_t* acc, int64_t* hist);
int sknnr_debug_last_zonal(const sknnr_index* index, int64_t out[8]);
int sknnr_debug_zonal_geometry(int32_t c, int64_t out[4]);

/* ---- distance domain (where the map extrapolates) -------------------------------------------------- */

/*
 * Distance domain.  THE CONTRACT, stated here once (sknnr_amd/csrc/domain.hip.h implements it, tests/_domain.py restates
 * it in numpy).  A pixel is placed within a table of reference-to-reference distances by the distance to its r-th
 * neighbour, in the estimator's own metric.
 *   Table T      m float64 values, 1 <= m <= 2^31 - 1, each finite and >= 0 (-0.0 is 0), non-decreasing.  Anything else
 *                is refused on the host with SKNNR_ERR_INVALID before any device work.
 *   Rank r       1 <= r <= k.  The pixel's score is s = dist[i, r - 1], the float64 distance the search returned, after
 *                sknnr's reorder when the call uses it.
 *   Code         uint8.  c = #{ j : T[j] < s } -- a strict comparison: np.searchsorted(T, s, "left") -- and
 *                code = (100 * c) / m in 64-bit integer arithmetic, so 0 <= code <= 100, and code == 100 exactly when
 *                s > T[m - 1].  A score equal to a table entry is not above it.  s = +inf gives 100; s <= 0 (-0.0
 *                included) gives 0.
 *   Nodata       a NaN s marks a nodata pixel (a row masked by sknnr_stream_set_nodata has NaN distances in the full
 *                layout).  Its code is 255; it enters the nodata count and nothing else.
 *   Threshold    theta, optional, finite and >= 0: a pixel is BEYOND when s > theta (false for NaN).
 *   Accumulators acc, int64[103]: acc[0 .. 100] the histogram of codes over the pixels that are not nodata, acc[101] the
 *                beyond pixels (0 without a threshold), acc[102] the nodata pixels.  Integer adds only: the results do
 *                not depend on launch geometry, tile cuts or arrival order, and two runs produce the same bytes.
 *   mask_beyond  (streams with predictions, and only with a threshold): the float64 prediction row of a beyond pixel
 *                becomes NaN in every column -- t targets, or the n_out planes of an output plan -- before the typed
 *                conversion and before the zonal tally, so the pixel stores the fill and enters no zonal table, exactly
 *                as a nodata pixel does.  Its indices, distances, ids and the usage tally are untouched.
 * Everything the pushes deliver without the lane stays bit for bit when mask_beyond is off, and a stream on which
 * sknnr_stream_set_domain is never called enqueues exactly what it did before the entry point existed.
 *
 * sknnr_domain_from_neighbors: one-shot.  dist (nq, k), codes (nq, or NULL: tallies only) and acc live in `mem` (host
 *   arrays are staged; device arrays are used in place, enqueued on `stream`); table is always a HOST array.  The table,
 *   the rank and the threshold are checked first, before the handle is even looked at.  accumulate = 0 zeroes acc first;
 *   accumulate = 1 adds to what it holds.  nq == 0 is allowed.  The handle gives the record and the staging buffers only.
 * sknnr_stream_set_domain: allowed only before the first push.  Checks the table and the rank against the stream's k,
 *   uploads the table once and zeroes the accumulators on the handle.  mask_beyond needs a stream opened with
 *   predictions, and a threshold.  From then on the stream keeps the search's distances even when none leave, and every
 *   tile's full-layout distances are coded on the device behind its search (and, with the mask, behind its reduction).
 * sknnr_stream_next_domain_out: the HOST destination of the NEXT push's code plane: nq bytes in pixel order, in either
 *   layout, filled under the same lifetime rule as that push's own outputs (complete after a flush).  Optional: a push
 *   without it tallies only.  A push with another nq than it named is SKNNR_ERR_INVALID.  nq == 0 is accepted and ignored.
 * sknnr_stream_get_domain: flushes the pipeline (as sknnr_stream_flush) and copies the accumulators to a HOST array.  May
 *   be called more than once; the accumulators keep running.
 * sknnr_debug_last_domain: debug only; synchronises the device.  The last sknnr_domain_from_neighbors call, or -- after
 *   sknnr_stream_set_domain -- the stream so far:
 *   out[0] 1 = a domain kernel ran         out[1] pixels its workgroups took     out[2] k      out[3] rank     out[4] m
 *   out[5] nodata pixels                   out[6] global atomics issued on the accumulators
 *   out[7] prediction rows blanked by the mask
 * sknnr_debug_domain_geometry: no device work.  out[0] pixels a workgroup takes, out[1] the most entries of its skeleton
 *   of the table, out[2] table entries between two skeleton entries at m, out[3] skeleton entries in use at m.
 */
int sknnr_domain_from_neighbors(sknnr_index* index, const double* dist, int64_t nq, int32_t k, int32_t rank,
                                const double* table, int64_t m, int32_t has_threshold, double threshold, uint8_t* codes,
                                int64_t* acc, int32_t accumulate, int32_t mem, void* stream);
int sknnr_stream_set_domain(sknnr_stream* stream, const double* table, int64_t m, int32_t rank, int32_t has_threshold,
                            double threshold, int32_t mask_beyond);
int sknnr_stream_next_domain_out(sknnr_stream* stream, uint8_t* out, int64_t nq);
int sknnr_stream_get_domain(sknnr_stream* stream, int64_t acc[103]);
int sknnr_debug_last_domain(const sknnr_index* index, int64_t out[8]);
int sknnr_debug_domain_geometry(int64_t m, int64_t out[4]);

/* ---- neighbour replay (attribute maps from stored neighbour rasters) ---------------------------------- */

/*
 * Neighbour replay.  THE CONTRACT, stated here once (sknnr_amd/csrc/replay.hip.h implements it, tests/_replay.py restates
 * it in numpy).  The neighbour raster -- plot ids and distances per pixel -- is made once by a search stream and stored;
 * a replay stream takes such tiles in place of feature rows and delivers everything a search stream delivers, bit for
 * bit what the search that wrote the neighbours delivered, without running any part of the search.
 *   Tile        for n pixels, ks stored neighbour columns: idx (required; int32 or int64; row positions in [0, n_ref) or
 *               ids of the handle's id table) and dist (optional; float32 or float64), as rows (n, ks) or as band-first
 *               planes (ks, n).  A stream uses the leading k <= ks columns as stored: with ties among the neighbours
 *               that is "the first k stored columns", not necessarily what a fresh k-search would return.
 *   Decode      on the device, into the pipeline's own full-layout tile: int64 idx (n, k), float64 dist (n, k) -- what a
 *               search followed by its nodata expansion leaves there.  Widening is exact (int32 -> int64,
 *               float32 -> float64).
 *   Masked      a pixel whose FIRST stored index equals fill_index; the test is made on the stored value, before any
 *               lookup, and no other column takes part.  It gets index -1, NaN distances and NaN in every prediction
 *               plane, enters neither the usage tally nor a zonal table, and gets domain code 255.
 *   Ids         every stored value is looked up in the handle's id table (sknnr_index_set_replay_ids: the int64 ids,
 *               sorted once on the host together with their row positions) by a lower-bound search on the device.
 *   Unknown     an id that is not in the table, or a row position outside [0, n_ref), in any of the k USED columns of a
 *               pixel that is not masked.  The pixel is then treated as masked, and counted.  No gather ever reads
 *               outside y.
 *   Afterwards  the tile goes through the unchanged later stages of the pipeline: the reduction (predictions,
 *               per-target statistics or the output plan), the blanking pass that gives masked and unknown pixels the
 *               state above, the usage tally, the distance domain with its mask, the zonal tally, the typed conversion
 *               with scale / offset / fill, the band transposes and the copies.  (The tally runs behind the blanking
 *               pass and skips the -1 indices; its sums are integer adds and do not depend on where it is enqueued.)
 *   Weights     uniform needs no distances; distance weights and the weight laws are computed from the stored distances
 *               as widened, never from any geometry.
 * Nothing of the search runs -- no preparation, no pre-filter, no finaliser, no scan -- and a replay stream never reads
 * the handle's reference rows.
 *
 * sknnr_index_create_targets: an attribute-only handle: it owns the (n_ref, t) float64 HOST table y and nothing else.  The
 *   from-neighbours entries and replay streams accept it; every entry that searches or configures a search refuses it
 *   with SKNNR_ERR_INVALID and a message that says why.  Freed by sknnr_index_destroy.
 * sknnr_index_set_replay_ids: installs the id table (n = n_ref int64 ids, HOST).  Duplicates are refused with
 *   SKNNR_ERR_INVALID before any device work -- the table is checked first, before the handle is even looked at;
 *   ids = NULL removes the table.  Not while a stream is open.
 * sknnr_replay_begin: opens a replay stream on the handle (one open stream per handle, as sknnr_stream_begin).
 *   k / ks as above; weight_mode / weight_law as in sknnr_query_opts; idx_dtype 0 (int64) or SKNNR_DTYPE_I32; dist_dtype
 *   0 (float64), SKNNR_DTYPE_F32 or SKNNR_REPLAY_NO_DIST; ids = 1: the stored values are ids; want_dist: pushes may ask
 *   for the decoded distances again (needs stored ones); want_pred as in sknnr_stream_begin.  Every refusal comes before
 *   any device work.  The stream works with sknnr_stream_set_statistics / _set_plan / _set_output / _set_id_table (the
 *   decoded indices may leave as ids again) / _set_tally / _get_tally / _set_zonal / _next_zones / _get_zonal /
 *   _set_domain / _next_domain_out / _get_domain / _flush / _end unchanged.  sknnr_stream_set_nodata is refused (the
 *   mask is the fill index), and so are _set_tally and _set_domain on a stream without stored distances, and the
 *   sknnr_stream_push* entries.
 * sknnr_replay_push / sknnr_replay_push_planes: one tile of nq pixels.  idx / dist are HOST arrays of the stream's stored
 *   types -- rows (nq, ks), or planes in_stride >= nq elements apart -- and may be reused as soon as the call returns;
 *   dist is given exactly when the stream has stored distances.  The outputs are those of sknnr_stream_push_typed /
 *   _planes_typed, in the stream's output types, each optional: a push may ask for none and still feed the tally, the
 *   zonal tables and the domain.  nq == 0 is accepted and counts as a push.
 * sknnr_replay_get_counts: flushes, then out[0] pixels, out[1] masked pixels, out[2] unknown pixels of the stream so
 *   far, out[3] the first push (counted from 0, empty ones included) that held unknown values, -1 when none did.
 * sknnr_debug_last_replay: debug only, host memory.  The last replayed tile of the handle:
 *   out[0] its pixels    out[1] masked    out[2] unknown    (of the last tile that has left the pipeline: after a flush, the last)
 *   out[3] the decode instantiation: 6 * (int64 indices) + 2 * (0 no distances, 1 float32, 2 float64) + (planes)
 *   out[4] 1 = ids: the skeleton path looked the values up      out[5] searches the tile's submission ran: 0
 *   out[6] k     out[7] ks
 */
#define SKNNR_REPLAY_NO_DIST (-1)
int sknnr_index_create_targets(const double* y, int64_t n_ref, int32_t t, int32_t device, sknnr_index** out);
int sknnr_index_set_replay_ids(sknnr_index* index, const int64_t* ids, int64_t n);
int sknnr_replay_begin(sknnr_index* index, int32_t k, int32_t ks, int32_t weight_mode, int32_t weight_law, int32_t idx_dtype,
                       int32_t dist_dtype, int64_t fill_index, int32_t ids, int32_t want_dist, int32_t want_pred,
                       sknnr_stream** out);
int sknnr_replay_push(sknnr_stream* stream, const void* idx, const void* dist, int64_t nq, void* out_dist, void* out_idx,
                      void* out_pred);
int sknnr_replay_push_planes(sknnr_stream* stream, const void* idx, const void* dist, int64_t nq, int64_t in_stride,
                             void* out_dist, void* out_idx, void* out_pred, int64_t out_stride);
int sknnr_replay_get_counts(sknnr_stream* stream, int64_t out[4]);
int sknnr_debug_last_replay(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The output side of the last tile the handle's host pipeline submitted, so that a test can prove that the
 * device converted it and that only the narrow bytes were copied.  Host memory, no device work:
 *   out[0] 1 = a conversion kernel ran for the tile, 0 = none did (no typed output and no id table)
 *   out[1] rows of the tile
 *   out[2] / out[3] / out[4] sknnr_dtype of the indices / distances / predictions (0 = int64 / float64)
 *   out[5] bytes the tile's device-to-host copies moved (0 until they are enqueued: behind the next tile, or by a flush)
 *   out[6] outputs whose conversion took the 4-elements-per-lane path: bit 0 indices, bit 1 distances, bit 2 predictions
 *   out[7] 1 = the tile's indices were crosswalked on the device (sknnr_stream_set_id_table), 0 = they left as row indices
 */
int sknnr_debug_last_narrow(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The last tile the handle's host pipeline submitted (host-memory calls and streams), so that a test can
 * prove that the device transposed it, not the host.  Host memory, no device work:
 *   out[0] 1 = its rows arrived as planes and planes_to_rows_kernel packed them on the device, 0 = a row tile
 *   out[1] rows of the tile      out[2] its columns      out[3] bytes per element
 *   out[4] 1 = its results left as planes (rows_to_planes_kernel), 0 = as rows
 *   out[5] output planes written (k per index / distance output, t for predictions; 0 for a row tile)
 *   out[6] columns one workgroup of planes_to_rows_kernel handles at that element size (0 for a row tile)
 *   out[7] 0
 */
int sknnr_debug_last_planes(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The nodata front end of the most recent call on the handle (its last tile), so that a test can prove
 * which path served it.  Host memory, no device work:
 *   out[0] 1 = the mask ran, 0 = it did not (then out[1 .. 7] = 0)
 *   out[1] rows of the last tile                out[2] its valid rows
 *   out[3] 1 = every row valid: searched in place, no compaction or expansion; 2 = every row masked: the fill alone;
 *          0 = compacted, searched, expanded
 *   out[4] workgroups of row_mask_kernel        out[5] bytes of a row
 *   out[6] valid rows of the whole call, or of the stream so far
 *   out[7] 0
 * Every search call zeroes the record first.
 */
int sknnr_debug_last_mask(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The kernels of the nodata front end alone, without a handle, so that a test can compare everything they
 * write -- not only final answers -- with a host restatement, at an alignment of its own choosing.
 *
 * sknnr_debug_mask_compact: mask, scan and compaction exactly as a masked device-memory call runs them, except that the
 *   compaction is launched whatever the valid count is (0 and nq included).
 *   q          (nq, d_in) rows of query_dtype, DEVICE memory on `device`; any address aligned to the element
 *   nodata     (d_in) float64, host
 *   out_packed DEVICE memory for the valid rows (nq rows always suffice); any address.  Only the first n_valid rows'
 *              bytes are written.
 *   out_valid  (nq) uint8, out_blk_off (ceil(nq / 256)) int32: the exclusive scan of the blocks' valid counts,
 *   out_rank   (nq) int32: valid rows in front of each row (written for masked rows too); host, each optional
 *   out_unit   host: bytes per copy of the compaction (1, 2, 4, 8 or 16: the largest power of two up to 16 that divides
 *              the row size and both addresses);  out_n_valid  host: the valid rows
 *   Returns when everything is written.
 * sknnr_debug_expand_rows: the expansion alone on the current device.  valid (nq) uint8, rank (nq) int32, the packed
 *   c_idx (n_valid, k) int64 / c_dist (n_valid, k) / c_pred (n_valid, t) and the full idx (nq, k) / dist (nq, k) /
 *   pred (nq, t) are DEVICE memory.  Each output may be NULL (it is not written); valid NULL: every row is masked and the
 *   packed arrays are not read.  With valid given, a NULL rank or a NULL packed array of a requested output is refused:
 *   SKNNR_ERR_INVALID.  Returns when the outputs are written.
 */
int sknnr_debug_mask_compact(const void* q, int64_t nq, int32_t d_in, int32_t query_dtype, const double* nodata,
                             int32_t device, void* stream, uint8_t* out_valid, int32_t* out_blk_off, int32_t* out_rank,
                             void* out_packed, int32_t* out_unit, int64_t* out_n_valid);
int sknnr_debug_expand_rows(int64_t nq, int32_t k, int32_t t, const uint8_t* valid, const int32_t* rank,
                            const int64_t* c_idx, const double* c_dist, const double* c_pred, int64_t* idx, double* dist,
                            double* pred, int64_t fill_index, void* stream);

/*
 * Dataframe-index crosswalk: out[i] = table[idx[i]].
 * Replaces self.dataframe_index_in_[neigh_ind] (REF _base.py:177-180) for int64 plot IDs.
 *   table : (n_table) int64 in `mem`;  idx, out : (n) int64 in `mem`
 */
int sknnr_crosswalk(const int64_t* table, int64_t n_table, const int64_t* idx, int64_t n,
                    int64_t* out, int32_t device, int32_t mem, void* stream);

/* ---- Bootstrap (standard errors per pixel from one search) -------------------------------------------- */

/*
 * How uncertain is a pixel's value because the plots are a sample?  The bootstrap over plots answers it: replicate b
 * contains reference row r M[b, r] = 0, 1, 2 ... times.  The k nearest rows of a pixel inside replicate b are found by
 * walking the pixel's ordinary neighbour list, nearest first, and taking M[b, r_j] copies of each neighbour until k copies
 * are taken -- so ONE search at a wider kw > k serves all B replicates, and the reduction per pixel runs on the device
 * (sknnr_amd/csrc/bootstrap.hip.h; tests/_bootstrap.py restates every line below in numpy).  The transform of a
 * transformed estimator is NOT refitted per replicate.  No product is fused into an addition anywhere: every product is
 * rounded, then added.
 *
 * Inputs per pixel: its kw neighbours (d_j, r_j), j = 0 .. kw - 1, in the order sknnr_kneighbors returns them; the handle's
 * table M, uint8 (B, n_ref) (sknnr_index_set_bootstrap); the replicate size k <= kw <= 192; a plan of n_out entries
 * (cols[e], stat[e]), stat a sknnr_bootstrap_statistic.
 *
 * Copies.  For replicate b: left = k; for j ascending c_j = min(M[b, r_j], left), left -= c_j; stop at left == 0.  The
 *   replicate is SHORT for this pixel when left > 0 behind column kw - 1.
 * Weights.  Those sknnr_predict uses, evaluated on d_j; only the taken columns (c_j > 0) count.
 *   UNIFORM  : 1
 *   DISTANCE : 1 / d_j.  If a TAKEN column has d_j == 0 the weights become the 0 / 1 mask of d == 0 over the taken columns;
 *              a zero-distance neighbour that is absent from the replicate does not trigger the mask.
 *   a law    : w(d_j) of sknnr_weight_law, bit for bit (weight_mode SKNNR_WEIGHTS_EXPLICIT names it, as in sknnr_predict)
 * Replicate value of target column col: den = sum_j cw_j, num = sum_j cw_j * y[r_j, col], cw_j = (double)c_j * w_j; both
 *   sums sequential, j ascending over the taken columns, from +0.0; p_b = num / den.  A replicate is INVALID when it is
 *   short or when den is not > 0 (a compact law).
 * Point value.  p0 is the same formula with c_j = 1 for j < k and 0 behind.  If its den is not > 0 every plane of the pixel
 *   is NaN and its count is 0.
 * Across replicates, per pixel and entry: a_b = p_b - p0 for a valid replicate, +0.0 for an invalid one; m = the valid
 *   replicates.  64 partial sums: partial l adds a_b (for S2: a_b * a_b) over b = l, l + 64, l + 128 ... ascending, from
 *   +0.0; they are folded by P[l] = P[l] + P[l + s] for l < s, s = 32, 16, 8, 4, 2, 1; the result is P[0].
 * Outputs:
 *   SKNNR_BOOT_BIAS  : S1 / m                          NaN when m == 0
 *   SKNNR_BOOT_MEAN  : p0 + S1 / m                     NaN when m == 0
 *   SKNNR_BOOT_SE    : sqrt(max((S2 - S1 * (S1 / m)) / (m - 1), 0.0))      NaN when m < 2
 *   SKNNR_BOOT_COUNT : (double)m; cols[e] is not read
 * Tallies, integer adds: tally[0] the pixels reduced, tally[1] the sum of m over them.
 * A pixel whose list names a row outside [0, n_ref) (the -1 of a blanked pixel) is all NaN with count 0 and enters
 * neither tally.
 * Multiplicities above 255 may be clamped to 255 by the caller without changing any result, since k <= 192.
 */
enum sknnr_bootstrap_statistic { SKNNR_BOOT_SE = 0, SKNNR_BOOT_MEAN = 1, SKNNR_BOOT_BIAS = 2, SKNNR_BOOT_COUNT = 3 };

/*
 * Installs (or with table == NULL removes) the multiplicity table: HOST memory, uint8 (B, n) row-major, n == n_ref,
 * 1 <= B <= 4096.  The handle keeps a transposed copy on the device.  Refused while a stream is open.  Handles of
 * sknnr_index_create_targets accept it.
 */
int sknnr_index_set_bootstrap(sknnr_index* index, const uint8_t* table, int32_t B, int64_t n);

/*
 * The reduction alone, from (dist, idx) of kw columns.
 *   dist, idx  : (nq, kw) float64 / int64 in `mem`; dist may be NULL for UNIFORM weights
 *   weight_mode, weight_law : as opts->weight_mode / opts->weight_law of sknnr_predict; explicit weights without a law
 *                and the F32 flags are refused
 *   cols, stat : HOST arrays of n_out, whatever `mem` is
 *   out        : (nq, n_out) float64 in `mem`
 *   tally      : (2) int64 in `mem`, set by the call; may be NULL
 * SKNNR_ERR_INVALID before any device work: no table installed, k outside [1, kw], kw above 192 or above n_ref, n_out
 * outside [1, 1024], a column outside [0, t), an unknown code, NULL arrays.
 * SKNNR_MEM_HOST returns when out is written; SKNNR_MEM_DEVICE enqueues on `stream`.
 */
int sknnr_bootstrap_from_neighbors(sknnr_index* index, const double* dist, const int64_t* idx, int64_t nq, int32_t kw,
                                   int32_t k, int32_t weight_mode, int32_t weight_law, const int32_t* cols,
                                   const int32_t* stat, int32_t n_out, double* out, int64_t* tally, int32_t mem,
                                   void* stream);

/*
 * A stream whose reduction stage is the bootstrap: valid on search streams opened at opts->n_neighbors = kw and on replay
 * streams (k of sknnr_replay_begin = kw), both opened with predictions; `k` here is the replicate size.  The prediction
 * lane becomes n_out wide; everything behind the reduction runs unchanged (blanking, typed conversion, band transposes,
 * copies).  Only before the first push and before sknnr_stream_set_output.  Refused together with
 * sknnr_stream_set_statistics, _set_plan, _set_tally, _set_domain and _set_zonal, whichever comes second; the caps of
 * sknnr_bootstrap_from_neighbors apply.  The F32_TARGETS flag of the stream's weight mode is ignored: the bootstrap
 * reduces in float64.  Masked pixels (nodata, replay fill, replay unknown) enter neither tally.
 * sknnr_stream_get_bootstrap flushes the stream and returns the two tallies over all tiles pushed so far (host memory).
 */
int sknnr_stream_set_bootstrap(sknnr_stream* stream, int32_t k, const int32_t* cols, const int32_t* stat, int32_t n_out);
int sknnr_stream_get_bootstrap(sknnr_stream* stream, int64_t tally[2]);

/*
 * Debug only.  The last bootstrap reduction the handle launched.  Host memory, no device work:
 *   out[0] rows      out[1] B      out[2] k      out[3] kw      out[4] n_out
 *   out[5] pixels per wave (1, 2 or 4)      out[6] kernel launches      out[7] 0
 */
int sknnr_debug_last_bootstrap(const sknnr_index* index, int64_t out[8]);

/* ---- diagnostics (used by the parity tests to validate the MFMA operand maps) ----------- */

/*
 * Full matrix of the pre-filter's approximate ranking values for a small problem:
 *   out[i, j] ~= s^2 (|r_j - mu|^2 - 2 (q_i - mu).(r_j - mu))   float32, host (nq, n_ref)
 * computed by the MFMA sequence of the first-generation kernel (all three split products on the matrix pipe;
 * the second-generation kernel's values differ by its smaller rounding budget only and are covered end to end).  Also returns the scale s,
 * the per-query |s (q_i - mu)|^2 (host, nq) and the error budget eps the certificate uses.
 * q is host, already transformed (d columns).  nq * n_ref must be <= 2^24.
 */
int sknnr_debug_coarse_matrix(sknnr_index* index, const double* q, int64_t nq, float* out,
                              double* out_qnorm, double* out_scale, double* out_eps);

/*
 * Which Euclidean pre-filter launches the most recent call on the handle made (its last device chunk), so that a test
 * can prove it reached the kernel instance it names.  Host memory, no device work:
 *   out[0] generation: 0 = no Euclidean pre-filter ran (exact scan only, or Hamming), 1 = coarse_kernel,
 *          2 = coarse2_kernel
 *   out[1] K-steps (16 features each)          out[2] list length M
 *   out[3] rank beyond the list E (0: the list holds kk + 1, with sentinels; always 0 for generation 1)
 *   out[4] waves per workgroup of the bulk launch (0: no bulk launch)
 *   out[5] rows given to the bulk launch       out[6] rows given to the 4-wave thin launch (generation 2)
 *   out[7] cell depth of the bucketed query order (0: plain order)
 * Every search call zeroes the record first.
 */
int sknnr_debug_last_prefilter(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The finaliser launches of the most recent call on the handle (its last device chunk), so that a test can
 * prove which finaliser served it:
 *   out[0] lanes per query (0: no finaliser ran; 8: finalize_record_kernel; 16 / 32 / 64: finalize_kernel on lists)
 *   out[1] 1 = the pre-filter filed merged candidate records and finalize_record_kernel read them, 0 = raw lists
 *   out[2] rows the record's truncation rule (its last entry inside the re-score window) handed to the exact scan over
 *          the whole call (read from the device, synchronously; 0 without records)
 *   out[3] 0 (reserved)
 * Every search call zeroes the record first.
 */
int sknnr_debug_last_finalize(const sknnr_index* index, int64_t out[4]);

/*
 * Debug only.  The integer pre-filter of the weighted-Hamming search (formula HAMMING) that the most recent call on the
 * handle ran, so that a test can prove which path served it:
 *   out[0] 1 = the integer pre-filter ran, 0 = it did not (every row went to the float64 exact scan; then out[1 .. 7] = 0)
 *   out[1] kk, the neighbours searched (k, + 1 for X=None)
 *   out[2] 1 = the candidate lists are seeded and compacted (kk >= 8)
 *   out[3] rows of the seeding pass (0 without compaction)
 *   out[4] band, in 16-bit weight units (trees + 2)
 *   out[5] tree pairs                          out[6] device chunks of the call (2^18 rows each)
 *   out[7] rows the integer path handed to the exact scan over the whole call (read from the device, synchronously)
 * Every search call zeroes the record first.  Under the forest map (sknnr_index_set_forest) a call runs in forest chunks
 * and the record describes the last of them.
 */
int sknnr_debug_last_hamming(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The float64 exact scan of the most recent call on the handle (the scan sequence of its last device chunk:
 * exact_scan_kernel, and for a call that may be sliced scan_merge_kernel and the sequential replay), so that a test can
 * prove which launch served it:
 *   out[0] 0 = no scan ran (then out[1 .. 7] = 0), else formula + 1
 *   out[1] 1 = the column-chunked instantiation ran (d > 1024)
 *   out[2] kk, the neighbours searched (k, + 1 for X=None)
 *   out[3] workgroups of the first scan launch    out[4] its dynamic LDS bytes
 *   out[5] rows offered to the scan: the call's rows, or the rows on the fail list (read from the device, synchronously)
 *   out[6] slices the reference rows of a pass are split into for that count (1 = not sliced): computed on the host from
 *          out[5] with the kernels' own scan_slices, not read back from the device
 *   out[7] rows the slice merge filed for the sequential replay (read from the device, synchronously)
 * After sknnr_merge_shards: out[3], out[4] describe the replay scan, out[6] is n_shards and out[7] the rows replayed.
 * Every search call zeroes the record first.
 */
int sknnr_debug_last_scan(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only: the rescue re-sweep of the last call -- the rows the finalisers listed, swept again under the bound their
 * re-scored candidates give before the float64 scan sees what is left: launched (0: the call was not served, all zero up
 * to out[6]), K-steps, rows offered (= the growth of exact_fallbacks), rows without a threshold (not rescuable), rows with
 * more than 16 references under their bound (overflowed), rows rescued, rows handed on to the exact scan; out[7]: rows
 * rescued by the handle since creation or the last sknnr_reset_stats.  Synchronises the device.
 */
int sknnr_debug_last_rescue(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  The candidate lists the integer Hamming pre-filter wrote for the first n rows of the last device chunk of
 * the most recent call (n at most that chunk's rows; SKNNR_ERR_INVALID when the pre-filter did not run).  Host memory:
 *   cnt (n)       candidates per row, -1 = the row went to the exact scan (list overflow, or ids outside 16 bits)
 *   ids (n, 192)  row i's candidates in ascending order in ids[192 i .. 192 i + cnt[i] - 1]; the other slots are stale
 * Synchronises the device.
 */
int sknnr_debug_hamming_candidates(const sknnr_index* index, int32_t* cnt, int32_t* ids, int64_t n);

/*
 * Debug only.  The candidate lists the first-generation Euclidean pre-filter (coarse_kernel) wrote for the first n rows of
 * the last device chunk of the most recent call, as stored (n at most that chunk's rows with their padding), M = out[2] of
 * sknnr_debug_last_prefilter.
 * Host memory:
 *   val  (n, 2, M) float32  ranking values: the list of the lane half that owns image positions p % 8 < 4, then the other's
 *   pos  (n, 2, M) int32    image positions, -1 = no row (a leading sentinel, value -FLT_MAX, or an unused slot, FLT_MAX)
 *   perm (n_ref)   int32    image position -> reference row of the first-generation image
 * SKNNR_ERR_UNSUPPORTED when the last call ran no Euclidean pre-filter, filed merged candidate records instead of lists, or
 * ran the second-generation kernel (its lists are filed by position of a bucketed call, in positions of its own image);
 * SKNNR_ERR_INVALID on a NULL argument or n beyond the chunk.  Reads only; synchronises the device.
 */
int sknnr_debug_coarse_candidates(const sknnr_index* index, int64_t n, float* val, int32_t* pos, int32_t* perm);

/*
 * Debug only.  The query preparation launch (prep_queries_direct_kernel / prep_queries_kernel) of the most recent call on
 * the handle (its last device chunk), so that a test can prove which kernel prepared its rows.  Host memory, no device work:
 *   out[0] 0 = no preparation kernel ran (then out[1 .. 7] = 0), 1 = prep_queries_direct_kernel, 2 = prep_queries_kernel (LDS)
 *   out[1] rows per block (256; the LDS kernel: 256 / 128 / 64 by the width of the input rows)
 *   out[2] element type of the rows (sknnr_dtype)
 *   out[3] live rows of the chunk              out[4] rows with the padding (a multiple of 6144)
 *   out[5] 1 = the kernel wrote the float64 transformed rows (an affine map, or rows narrower than float64)
 *   out[6] who named the rows' cells: 0 = nobody (the call was not bucketed), 1 = the preparation kernel,
 *          2 = cell_assign_kernel
 *   out[7] bits of the affine map in use: 1 center, 2 scale, 4 proj
 * Every search call zeroes the record first.
 */
int sknnr_debug_last_prep(const sknnr_index* index, int64_t out[8]);

/*
 * Debug only.  What the preparation and bucketing kernels wrote for the last device chunk of the most recent call, copied
 * from the handle's workspace (n at most that chunk's padded rows, out[4] above).  Host memory; each pointer may be NULL:
 *   qimg    (n, 64 ks bytes)  f16 hi / lo image rows: [hi | lo][K-step][K half] pieces of 16 bytes (8 halves)
 *   qnc     (n)               |s (q - mu)|^2, +inf for a row whose image overflows f16, 0 on padding rows
 *   xt      (min(n, live rows), d) the float64 transformed rows
 *   cell    (n)               cell of every row (padding rows: the last cell)
 *   perm    (n)               position -> row of the bucketed order
 *   qnc_pos (n)               qnc by position
 * SKNNR_ERR_INVALID when no preparation kernel ran, or for a buffer the call did not fill (xt without a transform; cell and
 * perm on a call that was not bucketed; qnc_pos unless the bucketed call filed candidate records).  Synchronises the device.
 */
int sknnr_debug_query_prep(const sknnr_index* index, int64_t n, void* qimg, double* qnc, double* xt, uint8_t* cell,
                           int32_t* perm, double* qnc_pos);

/*
 * Debug only.  The host-built constants the preparation and bucketing kernels read; each pointer may be NULL:
 *   mu (16 ks) zero-padded centre of the image      s: its power-of-two scale
 *   cell_depth: levels of the cell tree (0: none; then axes, centre and thr are left alone)
 *   axes (cell_depth, d)    centre (d)    thr (2^cell_depth - 1), node n of level l at 2^l - 1 + n
 * SKNNR_ERR_UNSUPPORTED when the index has no image (d > 128).
 */
int sknnr_debug_image_constants(const sknnr_index* index, double* mu, double* s, int32_t* cell_depth, float* axes,
                                float* centre, float* thr);

/*
 * Debug only.  The plan a search call works out before its first launch (which pre-filter, which lists, which finaliser,
 * which passes after it), for an index of n_ref x d reference rows with a cell tree of cell_depth levels and no affine
 * map, and a call of nq float64 rows searching kk neighbours (n_neighbors, + 1 when exclude_self is set) by `formula`.
 * The function the calls themselves run, on the description sknnr_index_create would leave: no handle, no device, so a
 * test can sweep the dispatch rules without a GPU.  flags: 1 exclude_self, 2 raw (shard candidates), 4 every reference id
 * fits the integer Hamming pre-filter, 8 the rescue re-sweep is enabled.
 *   out[0 .. 4] what sknnr_debug_last_prefilter would report of a one-chunk call: generation (0: no pre-filter), KS, list
 *               length, rank beyond the list, cell depth of a bucketed call
 *   out[5] 1 = the finaliser works from merged candidate records      out[6] 1 = the rescue re-sweep runs
 *   out[7] 1 = the integer Hamming pre-filter runs                    out[8] kk
 *   out[9] query rows per device chunk      out[10] rows of the largest chunk with its padding
 *   out[11] 1 = float64 transformed rows are written      out[12] columns of the caller's rows      out[13] check_finite
 *   out[14] element type of the rows (sknnr_dtype)        out[15] bits: 1 the affine map applies, 2 the rows are reference rows
 */
int sknnr_debug_search_plan(int64_t n_ref, int32_t d, int32_t cell_depth, int32_t kk, int64_t nq, int32_t formula,
                            int32_t flags, int64_t out[16]);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SKNNR_HIP_H */
