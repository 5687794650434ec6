// sknnr_hip.hip -- the C ABI of include/sknnr_hip.h over the gfx950 kernels (host translation unit).
//
// Host side only: index construction (coarse image of the reference rows), workspace,
// the per-chunk launch sequence  prep -> coarse (MFMA) -> finalize -> exact_scan,
// staging for host buffers, error reporting.  No CPU path computes results: if a
// device call fails the function fails.
// The host pipeline's lanes, staging copies, tile cuts and push description: no HIP in there.  (scripts/lane_arithmetic_check.cpp
// compiles this file up to here alone, SKNNR_LANE_ARITHMETIC_ONLY, under the sanitizers.)
#include "host_stage.h"

#ifndef SKNNR_LANE_ARITHMETIC_ONLY
#include "../../include/sknnr_hip.h"

#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

// kernels live in their own translation units (k_*.hip: each defines SKNNR_KERNELS_* for the non-template kernels it owns);
// this one sees their argument structs and geometry constants only
#include "launch.hip.h"

using namespace sknnr;

// ----------------------------------------------------------------------------------------
// errors
// ----------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(SKNNR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                 \
    } while (0)

// ----------------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------------
namespace {

// IEEE binary16 from double, round-to-nearest-even, overflow -> inf.
uint16_t f64_to_f16_bits(double v) {
    const float f = (float)v;  // double rounding is harmless: lo is taken from the actual hi
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t absx = x & 0x7fffffffu;
    if (absx >= 0x7f800000u) return (uint16_t)(sign | (absx > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (absx >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to >= 65520 -> inf
    if (absx < 0x33000001u) return (uint16_t)sign;               // < 2^-25 (or exactly) -> 0
    int exp = (int)(absx >> 23) - 127;
    uint32_t man = (absx & 0x7fffffu) | 0x800000u;  // 24-bit significand
    int shift;                                        // bits to drop
    uint32_t hexp;
    if (exp < -14) {  // subnormal half
        shift = 13 + (-14 - exp);
        hexp = 0;
    } else {
        shift = 13;
        hexp = (uint32_t)(exp + 15);
    }
    uint32_t q = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1u);
    const uint32_t halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (q & 1u))) ++q;
    uint32_t out;
    if (hexp == 0) out = q;  // q may reach 0x400 = smallest normal: encoding is continuous
    else out = ((hexp - 1) << 10) + q;  // q in [0x400, 0x800]; carry bumps the exponent
    return (uint16_t)(sign | out);
}

double f16_bits_to_f64(uint16_t h) {
    const int sign = (h >> 15) & 1;
    const int exp = (h >> 10) & 31;
    const int man = h & 1023;
    double v;
    if (exp == 0) v = std::ldexp((double)man, -24);
    else if (exp == 31) v = man ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
    else v = std::ldexp((double)(man | 1024), exp - 25);
    return sign ? -v : v;
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }  // early returns (HIP_TRY) free what a function allocated
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    // room for `count` elements, filled from host memory
    int upload(const void* src, size_t count) {
        HIP_TRY(ensure(count));
        HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return SKNNR_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// One array argument of a one-shot call that takes either memspace.  Device memory: p is the caller's pointer.  Host
// memory: p is a device buffer of this object's own, filled from the caller's array when the launch reads it (kStageIn,
// kStageInOut) and copied back by download() when the launch writes it (kStageOut, kStageInOut).  A null argument stays
// null.  The buffer is freed by the destructor on every return path.
enum { kStageIn = 1, kStageOut = 2, kStageInOut = kStageIn | kStageOut };
template <typename T>
struct Staged {
    T* p = nullptr;
    DevBuf<T> buf;
    void* host = nullptr;  // where download() copies `count` elements to (null: nowhere)
    size_t count = 0;
    int stage(const void* caller, size_t n, int mem, int dir) {
        p = (T*)caller;
        if (mem != SKNNR_MEM_HOST || !caller) return SKNNR_OK;
        HIP_TRY(buf.ensure(n));
        if ((dir & kStageIn) && n) HIP_TRY(hipMemcpy(buf.p, caller, n * sizeof(T), hipMemcpyHostToDevice));
        if (dir & kStageOut) host = (void*)caller;
        count = n;
        p = buf.p;
        return SKNNR_OK;
    }
    int download() {
        if (host && count) HIP_TRY(hipMemcpy(host, buf.p, count * sizeof(T), hipMemcpyDeviceToHost));
        return SKNNR_OK;
    }
};

// The debug record of a side product (neighbour usage, zonal statistics, distance domain): the device words its kernels
// add to -- two halves of `words` each, half 0 of one-shot calls, half 1 of the open stream, so that neither disturbs the
// other's counters -- and the host's words of the sknnr_debug_last_* entry (ran, rows, then the product's own), with the
// half they belong to: whoever started or ran last.
struct ProductRec {
    const int words;
    DevBuf<unsigned long long> dev;
    int64_t host[5] = {};
    int half = 0;
    explicit ProductRec(int words_) : words(words_) {}
    hipError_t ensure() { return dev.ensure(2 * (size_t)words); }
    unsigned long long* at(int h) const { return dev.p + h * words; }
    // a call or a stream begins: its device words are zeroed on `st`, the host's words are `h5` (the rest zero)
    hipError_t reset(int h, hipStream_t st, std::initializer_list<int64_t> h5) {
        std::fill(host, host + 5, 0);
        std::copy(h5.begin(), h5.end(), host);
        half = h;
        return hipMemsetAsync(at(h), 0, words * sizeof(unsigned long long), st);
    }
    // a tile of the open stream was launched
    void ran(int h, long n) {
        host[0] = 1;
        host[1] += n;
        half = h;
    }
    // out: the host's words, zeros behind them; w: the device words of their half, once the device is idle (zeros while
    // nothing was launched).  Takes the handle's lock.
    int read(std::mutex& mtx, int device, int64_t out[8], unsigned long long w[]) {
        std::lock_guard<std::mutex> lock(mtx);
        std::fill(out, out + 8, 0);
        std::copy(host, host + 5, out);
        std::fill(w, w + words, 0);
        if (!dev.p) return SKNNR_OK;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(w, at(half), words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return SKNNR_OK;
    }
};

// The side products on the handle, one struct each: `call` holds what a one-shot call parks on the handle, `stream` what
// the open stream's setter (sknnr_stream_set_*) installed and the stream's accumulators, `rec` the debug record.
// Neighbour usage (tally.hip.h): the stream's counts (n_ref, k) and maxima (n_ref); the record's host words are ran,
// rows, k.
struct TallyProduct {
    struct { DevBuf<unsigned long long> cnt, max; } stream;
    ProductRec rec{kTallyRecWords};
};
// Zonal statistics (zonal.hip.h): the class table of each kind of call -- n_classes per column (cls) and where each
// column's block begins in hist (off); the conversion parameters of one-shot calls (par: scale then offset); the
// stream's accumulators and class blocks; the record's host words are ran, pixels, c.
struct ZonalProduct {
    struct { DevBuf<int> cls; DevBuf<long> off; DevBuf<double> par; } call;
    struct { DevBuf<int> cls; DevBuf<long> off; DevBuf<long long> acc, hist; } stream;
    ProductRec rec{kZonalRecWords};
};
// Distance domain (domain.hip.h): the sorted table of each kind of call and the stream's accumulators; the record's host
// words are ran, pixels, k, rank, m.
struct DomainProduct {
    struct { DevBuf<double> table; } call;
    struct { DevBuf<double> table; DevBuf<unsigned long long> acc; } stream;
    ProductRec rec{kDomainRecWords};
};
// Bootstrap (bootstrap.hip.h): the plan arrays and the two tally words of a one-shot call (the plan is a workspace buffer
// behind ev_ws) and of the open stream's stage; its record is the handle's last_boot.
struct BootProduct {
    struct Bufs { DevBuf<int> plan; DevBuf<unsigned long long> tally; } call, stream;
};

// Device buffers of the nodata front end (mask.hip.h) for one tile: the handle has a set for device-memory calls, every
// slot of the host pipeline one of its own.
struct MaskBufs {
    DevBuf<unsigned char> valid;  // (n) 1 = valid
    DevBuf<int> blk, rank;        // valid rows per block, then their exclusive scan; valid rows before each row
    DevBuf<long> nvalid;          // the tile's valid rows (device word), copied to *pin_nv
    DevBuf<char> cx;              // the packed rows
    DevBuf<double> cd, cp;        // packed results
    DevBuf<long> ci;
    long* pin_nv = nullptr;       // pinned host word the 8-byte copy lands in
    MaskBufs() = default;
    MaskBufs(const MaskBufs&) = delete;
    MaskBufs& operator=(const MaskBufs&) = delete;
    ~MaskBufs() {
        if (pin_nv) (void)hipHostFree(pin_nv);
    }
};
constexpr int kMaskMaxCols = 1 << 16;  // the mask kernels index a block's elements with an int

constexpr int kMaxKs = 8;              // coarse path: d <= 128
// a switch that is on unless the variable is set to 0
inline bool env_on(const char* name) {
    const char* e = std::getenv(name);
    return !(e && std::atoi(e) == 0);
}
constexpr size_t kLdsLimit = 150 * 1024;  // LDS bytes a workgroup of any kernel here may ask for
// rows per block of prep_queries_kernel for rows of d_in columns, by what fits the LDS (0: too wide, d_in > 299)
inline int prep_lds_rows(int d_in) {
    for (int bt : {256, 128, 64})
        if ((size_t)bt * (d_in | 1) * 8 <= kLdsLimit) return bt;
    return 0;
}
// rows of a device chunk with its padding (the pre-filter's workgroups and the prep kernel's blocks divide kRowQuantum)
inline long pad_rows(long n) { return (n + kRowQuantum - 1) / kRowQuantum * kRowQuantum; }
// Stages of the second-generation image of n_ref rows: tiles of 32 rows, rounded up to whole stages of tiles_per_stage2(ks)
// (0: no such image -- more than four K-steps, or no coarse image at all)
inline int image_stages2(long n_ref, int ks) {
    if (ks < 1 || ks > 4) return 0;
    const int tps2 = tiles_per_stage2(ks);
    return (int)(((n_ref + 31) / 32 + tps2 - 1) / tps2);
}
constexpr long kChunkRows = 1L << 22;  // rows per chunk of host-side staging loops (transform entry point, X=None results)
// Query rows per device chunk of one call (each chunk: prep -> pre-filter -> finalise, padded to kRowQuantum).
// One launch for as many rows as a 4 GiB workspace holds, at most 2^24: every pre-filter launch ends with a
// partly filled last round of workgroups (a workgroup sweeps the whole image: ~1.3 ms at 50k rows), so fewer,
// larger launches waste less (10M x 50k x 32, k=5: 183 -> 188 Mq/s against chunks of 4M rows,
// scripts/chunk_probe.py).  SKNNR_CHUNK_ROWS overrides (A/B runs).
long chunk_rows(int ks, int m_list) {
    static const long forced = [] {
        const char* e = std::getenv("SKNNR_CHUNK_ROWS");
        const long r = e ? std::atol(e) : 0;
        return r >= kRowQuantum ? std::min<long>(r, 1L << 26) : 0L;
    }();
    if (forced) return forced;
    const long per_row = 64L * std::max(ks, 1) + 8 + 16L * std::max(m_list, 2);  // query image + |q'|^2 + two candidate lists
    const long rows = std::min<long>(1L << 24, (4L << 30) / per_row);
    return std::max<long>(kRowQuantum, rows / kRowQuantum * kRowQuantum);
}
constexpr int kScanMaxKK = 192;
static_assert(kSummaryMaxK == kScanMaxKK, "the summary kernels follow np_sum up to the largest k of a search");
// The per-target statistics of one call or stream (summary.hip.h): the columns that are not the mean, as the device table
// the summary kernels read (columns, then codes), and how many columns stay with the predict kernels.
struct SummaryPlan {
    int nc = 0;
    int n_mean = 0;
    const int* tab = nullptr;
};
// (t) sknnr_statistic codes -> the host image of the table; false: an unknown code, reported in *bad
bool summary_table(const int32_t* stat, int t, std::vector<int>& tab, int* bad) {
    std::vector<int> cols, codes;
    for (int j = 0; j < t; ++j) {
        if (stat[j] < 0 || stat[j] >= kStatCount) {
            *bad = j;
            return false;
        }
        if (stat[j] != kStatMean) {
            cols.push_back(j);
            codes.push_back(stat[j]);
        }
    }
    tab = cols;
    tab.insert(tab.end(), codes.begin(), codes.end());
    return true;
}
// An output plan of one call or stream (plan.hip.h): the device arrays plan_kernel reads, and how many entries are means
// (the predict kernels run into the handle's mean_stage for them).  The prediction lane is n_out wide while one is set.
// The bootstrap stage of an open stream (sknnr_stream_set_bootstrap; bootstrap.hip.h): the plan's device arrays as the
// kernel reads them and the replicate size.
struct BootStage {
    int n_out = 0, n_u = 0;
    int k = 0;
    const int* ucols = nullptr;
    const int* uidx = nullptr;
    const int* codes = nullptr;
};

struct OutputPlan {
    int n_out = 0;
    int n_mean = 0;
    const int* cols = nullptr;
    const int* codes = nullptr;
    const double* param = nullptr;
};
// What the reduction behind a search (or behind stored neighbours) computes: the kind and the part that belongs to it.
// Every function between an entry point and launch_predict takes it as an argument; the handle holds none.  A default
// one is the mean of every target; a statistics table that is all mean (stat.nc == 0) enqueues the same launches.
enum { kReduceMean = 0, kReduceStats, kReducePlan, kReduceBoot };
struct Reduction {
    int kind = kReduceMean;
    SummaryPlan stat;
    OutputPlan plan;
    BootStage boot;
    unsigned long long* boot_tally = nullptr;  // the two tally words a bootstrap launch adds to (device)
    // columns of a prediction row over t targets
    int cols(int t) const { return kind == kReduceBoot ? boot.n_out : kind == kReducePlan ? plan.n_out : t; }
};
// The host image of a plan's device arrays: n_out parameters, then (as ints) n_out columns and n_out codes.
std::vector<double> plan_image(const int32_t* cols, const int32_t* stat, const double* param, int n_out) {
    std::vector<double> img((size_t)2 * n_out, 0.0);
    std::copy(param, param + n_out, img.begin());
    int* ints = (int*)(img.data() + n_out);
    std::copy(cols, cols + n_out, ints);
    std::copy(stat, stat + n_out, ints + n_out);
    return img;
}
// Error bound of the split contraction, in units of 2^-24 (|q'| + max|r'|)^2 -- derived in DESIGN.md
// section 2 from the measured arithmetic of v_mfma_f32_32x32x16_f16 (scripts/microbench/
// mfma_f16_numerics.hip, profiles/r02_mfma_f16_numerics.txt: per instruction two groups of eight exact
// products, each group aligned to its largest product and truncated 24 bits below it, each group sum
// added with one round-to-nearest-even):
//     6.01   dropped terms of the split  (lo.lo, and the residuals a - hi - lo, b - hi - lo)
//   + 3.51   truncation inside the groups  (7 x 2^-24 x sum |products|, sum <= 2 |q'||r'| (1 + 2^-10))
//   + 1.00   |r'|^2 rounded to f32 (the C operand)
//   + 6 ks   two roundings per instruction, 3 ks instructions, each <= 2^-24 x |partial value|
//   + 0.25   f16 subnormal floor of the lo parts
// = 10.77 + 6 ks  ->  11 + 6 ks.  Random operands reach 2.6 (d=8) .. 5.1 (d=100) units
// (tests/test_hip_parity.py::test_coarse_error_budget); adversarial ones (same-sign products at the
// image limits, full mantissas) are tested in test_coarse_error_budget_adversarial.
constexpr double eps_units(int ks) { return 11.0 + 6.0 * ks; }
// coarse2_kernel: only the ks main instructions round in the matrix pipe (2 ks roundings); the correction is a
// packed-f16 dot product in f32 whose own rounding is below 0.1 unit, added with one more rounding:
//   6.01 + 3.51 + 1.00 + (2 ks + 1) + 0.25 + 0.1 = 11.87 + 2 ks  ->  12 + 2 ks.
constexpr double eps_units2(int ks) { return 12.0 + 2.0 * ks; }

}  // namespace

// ----------------------------------------------------------------------------------------
// the handle
// ----------------------------------------------------------------------------------------
constexpr int kHostSlots = 4;  // tiles in flight in the host-buffer pipeline
using Word = unsigned long long;  // the 8-byte unit of the pipeline's output buffers

// One background host thread that runs posted jobs in order (the host-buffer pipeline's copy-in and copy-out legs:
// the staging memcpys used to sit in the enqueueing thread, in series with it -- profiles/r02_host_path_probe.txt).
class HostWorker {
public:
    HostWorker() : th_([this] { run(); }) {}
    ~HostWorker() {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    std::future<int> post(std::function<int()> fn) {
        std::packaged_task<int()> task(std::move(fn));
        std::future<int> f = task.get_future();
        {
            std::lock_guard<std::mutex> l(m_);
            q_.emplace_back(std::move(task));
        }
        cv_.notify_one();
        return f;
    }

private:
    void run() {
        for (;;) {
            std::packaged_task<int()> task;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;  // stop requested and nothing left to do
                task = std::move(q_.front());
                q_.pop_front();
            }
            task();
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::packaged_task<int()>> q_;
    bool stop_ = false;
    std::thread th_;  // (last member: the thread starts when everything above exists)
};

// The debug records of the search path: every search call zeroes them first (zero_records), then each stage files its own.
struct SearchRecords {
    // the Euclidean pre-filter launches of the last device chunk of the last call (sknnr_debug_last_prefilter):
    // generation, KS, list length, rank beyond the list, bulk waves, bulk rows, thin rows, cell depth
    int64_t prefilter[8] = {};
    // the finaliser launches of the last device chunk of the last call (sknnr_debug_last_finalize): lanes per query, record
    // path (the rows its truncation rule sent to the exact scan are read from fail_count[3] when asked)
    int64_t finalize[2] = {};
    // the integer Hamming pre-filter of the last call (sknnr_debug_last_hamming): ran, kk, compacts, seed rows, band,
    // tree pairs, device chunks (out[7], the rows handed to the exact scan, is read from fail_count when asked); rows of
    // its last device chunk, whose candidate lists h_cand_cnt / h_cand_id still hold (sknnr_debug_hamming_candidates)
    int64_t hamming[8] = {};
    long hamming_rows = 0;
    // the exact scan of the last call (sknnr_debug_last_scan): formula + 1, chunked, kk, workgroups and LDS bytes of the
    // first scan launch, rows offered (host count; -1: the fail list's device count, read from fail_count[0] when asked),
    // slices (0: whatever scan_slices gives for the count, worked out when asked; else fixed: 1 = the call cannot be
    // sliced, or the shard count of a shard merge), 1 = count2 (fail_count[2]) holds the rows filed for the replay
    int64_t scan[8] = {};
    // the query preparation of the last device chunk of the last call (sknnr_debug_last_prep): kernel (1 direct, 2 LDS), rows
    // per block, x_dtype, live rows, padded rows, xt written, who named the cells (1 the prep kernel, 2 cell_assign_kernel),
    // bits center | scale << 1 | proj << 2; and what of that chunk the workspace holds (sknnr_debug_query_prep): its
    // transformed rows, the cells and the permutation, |q'|^2 by position
    int64_t prep[8] = {};
    const double* prep_xt = nullptr;
    bool prep_bucketed = false, prep_qnc_pos = false;
    // the rescue re-sweep of the last call (sknnr_debug_last_rescue): launched, KS; the counts are read from resc_state
    int64_t rescue[2] = {};
    // the nodata front end of the last tile (sknnr_debug_last_mask)
    int64_t mask[8] = {};
    // the leave-group-out scan of the last call (sknnr_debug_last_grouped): formula + 1, k, workgroups, LDS bytes, rows,
    // slices (1: none), the largest group, the number of groups
    int64_t grouped[8] = {};
    // the masks of that scan (sknnr_debug_last_buffer): mask mode (1 groups, 2 buffer, 3 both), position columns,
    // max(excluded), min(excluded), workgroups and LDS bytes of the count launch, a row that attains the maximum
    int64_t buffer[8] = {};
};

struct sknnr_index {
    int device = 0;
    long n_ref = 0;
    int d = 0, t = 0;
    int ks = 0;       // K-steps of the coarse image (0 = coarse path unavailable: d > 128)
    int n_stages = 0;
    double s = 1.0;   // coarse scale
    double ymax = 0.0;
    double mu_norm = 0.0;    // |mu| (upper bound), for the reference formula's rounding-noise term
    std::vector<double> mu;  // (16*ks) zero padded
    std::mutex mtx;          // one call at a time per handle (the workspace below is shared)

    // query-time affine map
    int d_in = 0;
    bool has_affine = false;
    DevBuf<double> center, scale, proj;  // proj padded to (d_in, 16*ks) when ks > 0 else (d_in, d)
    bool has_center = false, has_scale = false, has_proj = false;

    // query-time forest map of RFNN / GBNN (forest.hip.h): raw rows -> node ids, one column per tree
    bool has_forest = false;
    int f_d_in = 0;
    DevBuf<int4> f_nodes;
    DevBuf<long> f_off;
    DevBuf<int> f_depth;
    DevBuf<double> f_ids;  // workspace: node ids of one chunk of a call's rows

    DevBuf<double> hw;       // weighted-Hamming weights (one per column), set by sknnr_index_set_hamming_weights
    double hw_sum = 0.0;
    bool has_hw = false;
    // leave-group-out neighbours (groups.hip.h): the group code of every reference row, set by sknnr_index_set_groups
    DevBuf<int> g_codes;
    bool has_groups = false;
    long g_largest = 0, g_count = 0;  // rows of the largest group, number of groups
    // buffered leave-out (buffer.hip.h): the (3, n_ref) positions and the radius, set by sknnr_index_set_buffer; and
    // excluded[] under the masks now set, counted once per change of either mask (ensure_excluded)
    DevBuf<double> b_pos;
    bool has_buffer = false;
    int b_cols = 0;
    double b_radius = 0.0, b_r2 = 0.0;
    DevBuf<unsigned long long> b_excl;
    bool b_excl_valid = false;
    long b_max = 0, b_min = 0, b_argmax = 0;  // of excluded[]; the first row that attains the maximum
    long b_count_wg = 0;                      // workgroups of the launch that counted them
    // integer pre-filter of the weighted-Hamming search (hamming.hip.h): 16-bit ids / weights, two trees per dword
    bool h16_ok = false;           // every reference id is an integer in [0, 65535]
    int h_tp = 0, h_ref_pad = 0;   // tree pairs; reference rows padded to the step of the kernel
    DevBuf<uint32_t> h_rimg, h_wq, h_qimg, h_rrow;  // (h_rrow: row-major ids for the re-score)
    DevBuf<int> h_bad, h_cand_cnt, h_cand_id;
    DevBuf<double> ref64, refT, rn64, y64, mu_dev;  // refT: (d, n_ref) transposed copy for the exact scan
    DevBuf<char> rimg;
    DevBuf<char> rhi2, rlo2;  // coarse2_kernel's image: [hi | |r'|^2] records for the LDS stages, lo fragments apart
    int n_stages2 = 0;
    DevBuf<int> perm;  // image position -> reference row (rows are imaged by increasing centred norm)
    // Second-generation image in CELL order (bucket.hip.h): a median-split tree over the leading principal axes
    DevBuf<int> perm2;             // its image position -> reference row
    int cell_depth = 0;            // 0: the second image is in the first one's order, no bucketing
    DevBuf<float> cell_axes, cell_centre, cell_thr;
    DevBuf<int> cell_stage;        // [2^depth] stage at which a workgroup of that cell starts its sweep
    DevBuf<unsigned char> qcell;   // workspace: cell of every query row of the chunk
    DevBuf<int> qperm, cell_hist;  // workspace: position -> row; [2][kCellMax] rows per cell / cursors

    // workspace (one chunk)
    DevBuf<double> xt, qnc, xstage, dist_stage, pred_stage;
    DevBuf<uint4> qimg;
    DevBuf<float> cand_val;
    DevBuf<int> cand_idx, fail_list, fail_count, fail_list2, slice_i;
    // merged candidate records (coarse2.hip.h, Coarse2Record) and |q'|^2 by position, in place of cand_val / cand_idx
    DevBuf<unsigned long long> rec;
    DevBuf<float> rec_bound;
    DevBuf<double> qnc_pos;
    DevBuf<double> slice_v;  // sliced exact scans: the slice heaps (exact.hip.h, scan_slices)
    // Rescue re-sweep (rescue.hip.h): the thresholds beside fail_list, the second list (what the exact scan still sees) and the
    // call's device words; fail_total[1] is the running count of rescued rows.  SKNNR_RESCUE=0 (read when the index is
    // created) keeps every listed row on the exact scan (A/B runs).
    DevBuf<float> fail_thr;
    DevBuf<int> resc_list, resc_state;
    bool rescue_enabled = true;
    DevBuf<int> status;            // bit 0: a query value was NaN, bit 1: infinite (since the last poll)
    DevBuf<long long> fail_total;  // running count of certificate failures (device)
    DevBuf<long> idx_stage;

    // host-buffer pipeline: pinned staging + device staging, kHostSlots slots; three streams
    struct HostSlot {
        double* pin_x = nullptr;  size_t pin_x_n = 0;
        DevBuf<double> dev_x;
        DevBuf<double> dev_xp;  // band-first tiles (planes.hip.h): the uploaded planes, in front of dev_x
        int32_t* pin_z = nullptr;  size_t pin_z_n = 0;  // zonal streams: the tile's zone codes, pinned and on the device
        DevBuf<int32_t> dev_z;
        uint8_t* pin_dom = nullptr;  size_t pin_dom_n = 0;  // domain streams: the tile's code plane, on the device and pinned
        DevBuf<uint8_t> dev_dom;
        // One output (kLaneIdx / kLaneDist / kLanePred), all in 8-byte words: int64 indices, float64 values, packed narrow elements.
        struct Lane {
            Word* pin = nullptr;  size_t pin_n = 0;  // pinned: what the device-to-host copy fills
            DevBuf<Word> dev;     // (n, cols) as the search / the reduction writes it
            DevBuf<Word> planes;  // band-first tiles: (cols, n) behind dev
            DevBuf<Word> nar;     // typed outputs (narrow.hip.h): the stream's output type, packed rows or planes
            long* i64() const { return (long*)dev.p; }
            double* f64() const { return (double*)dev.p; }
        } lane[kLanes];
        hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_d2h = nullptr;
        MaskBufs mask;  // nodata front end of the slot's tile (a pipeline with a mask only)
    } slot[kHostSlots];
    hipStream_t st_h2d = nullptr, st_run = nullptr, st_d2h = nullptr;
    std::unique_ptr<HostWorker> w_in, w_out;  // copy-in (look-ahead) and copy-out legs of the host pipeline

    // Workspace hand-over between calls on different streams: the last launch of a call records
    // ev_ws; the next call's stream waits for it before it touches the workspace.
    hipEvent_t ev_ws = nullptr;
    bool ws_busy = false;
    // The thin last round of the pre-filter (4-wave workgroups, one wave per SIMD) leaves most of every CU free: the
    // finaliser of the rows that are already done runs beside it on a side stream (fork after the bulk launch, join
    // before the exact scan).
    hipStream_t st_side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    SearchRecords last;  // what the last search left for the sknnr_debug_last_* entries
    bool stream_open = false;  // a sknnr_stream owns the host pipeline's slots
    // nodata front end: the buffers of device-memory calls, the nodata values of one-shot calls and of the open stream,
    // (the record of the last tile is SearchRecords::mask)
    MaskBufs mask;
    DevBuf<double> m_nodata, s_nodata;
    // the last tile of the host pipeline (sknnr_debug_last_planes): rows arrived as planes, rows, columns, element bytes,
    // results left as planes, output planes written, columns per workgroup of planes_to_rows_kernel
    int64_t last_planes[8] = {};
    // typed outputs of the open stream: the per-target scale / offset on the device, and the record of the last tile of
    // the host pipeline (sknnr_debug_last_narrow): conversion ran, rows, the three output types, bytes its device-to-host
    // copies moved, outputs that took the wide path (bit 0 indices, 1 distances, 2 predictions), indices crosswalked on
    // the device; and the open stream's id table (sknnr_stream_set_id_table)
    DevBuf<double> s_scale, s_offset;
    DevBuf<long> s_id_table;
    int64_t last_narrow[8] = {};
    // per-target statistics (summary.hip.h): the device tables of a one-shot call (c_stat, a workspace buffer behind
    // ev_ws) and of the open stream (s_stat); the record of the last reduction (sknnr_debug_last_summary).
    DevBuf<int> c_stat, s_stat;
    int64_t last_summary[8] = {};
    // output plans (plan.hip.h): the device arrays of a one-shot call (c_plan, a workspace buffer behind ev_ws) and of the
    // open stream (s_plan); the (rows, t) means the predict kernels write for a plan's `mean` entries (mean_stage, behind
    // ev_ws too); the record of the last reduction (sknnr_debug_last_plan): plan kernel ran, path (1 register, 2 wide),
    // rows, n_out, k, mean entries, predict kernels ran.
    DevBuf<double> c_plan, s_plan, mean_stage;
    int64_t last_plan[8] = {};
    // distance-weight laws (weights.hip.h): the handle's law and its parameters (sknnr_index_set_weight_law_params), the
    // weights launch_predict computes for a call that names the law (a workspace buffer behind ev_ws), and the record of
    // the last reduction (sknnr_debug_last_weight_law): law, rows, k, kernel ran
    int law_code = 0;
    double law_p0 = 0.0, law_p1 = 0.0;
    DevBuf<double> law_w;
    int64_t last_law[8] = {};
    // the side products (TallyProduct ... BootProduct above: call-side buffers, stream-side buffers, the debug record)
    TallyProduct tally;
    ZonalProduct zonal;
    DomainProduct domain;
    BootProduct boot;
    // neighbour replay (replay.hip.h).  targets_only: the handle was made by sknnr_index_create_targets and owns y64 and
    // nothing of a search.  The sorted id table of sknnr_index_set_replay_ids and the row position of each of its entries;
    // the per-tile records of the open replay stream, one per pipeline slot, on the device and pinned; the searches the
    // handle has run (run_device), so that a replayed tile can show that it ran none; the record of the last tile
    // (sknnr_debug_last_replay).
    bool targets_only = false;
    DevBuf<long> r_id_sorted;
    DevBuf<int> r_id_perm;
    long r_id_n = 0;
    DevBuf<unsigned long long> replay_rec;
    unsigned long long* pin_replay = nullptr;
    long search_calls = 0;
    int64_t last_replay[8] = {};
    // bootstrap (bootstrap.hip.h): the transposed multiplicity table of sknnr_index_set_bootstrap, (n_ref, boot_bpad) bytes,
    // and its replicates (0: none installed); the record of the last reduction (sknnr_debug_last_bootstrap); the plans
    // and tally words are in `boot` above
    DevBuf<unsigned char> boot_mt;
    int boot_B = 0, boot_bpad = 0;
    int64_t last_boot[8] = {};

    // Device timing of calls (HIP events on the launch stream), resolved lazily by sknnr_get_stats:
    // a ring of call records so that several calls of one benchmark step are summed, not only the last.
    struct CallTiming {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> coarse;
        size_t coarse_used = 0;
        long coarse_rows = 0;  // rows the timed pre-filter launches of this call processed
        bool pending = false;
    };
    static constexpr int kTimingRing = 64;
    CallTiming timing[kTimingRing];
    int timing_next = 0;
    sknnr_stats stats{};

    ~sknnr_index() {
        w_in.reset();   // (joins: no job may outlive the buffers below)
        w_out.reset();
        (void)hipSetDevice(device);  // (the DevBuf members free themselves behind this body)
        for (auto& sl : slot) {
            if (sl.pin_x) (void)hipHostFree(sl.pin_x);
            if (sl.pin_z) (void)hipHostFree(sl.pin_z);
            if (sl.pin_dom) (void)hipHostFree(sl.pin_dom);
            for (auto& ln : sl.lane)
                if (ln.pin) (void)hipHostFree(ln.pin);
            for (hipEvent_t e : {sl.ev_h2d, sl.ev_done, sl.ev_d2h})
                if (e) (void)hipEventDestroy(e);
        }
        for (hipStream_t h : {st_h2d, st_run, st_d2h})
            if (h) (void)hipStreamDestroy(h);
        if (pin_replay) (void)hipHostFree(pin_replay);
        if (ev_ws) (void)hipEventDestroy(ev_ws);
        if (st_side) (void)hipStreamDestroy(st_side);
        for (hipEvent_t e : {ev_fork, ev_join})
            if (e) (void)hipEventDestroy(e);
        for (auto& ct : timing) {
            for (hipEvent_t e : {ct.e0, ct.e1})
                if (e) (void)hipEventDestroy(e);
            for (auto& pr : ct.coarse) {
                (void)hipEventDestroy(pr.first);
                (void)hipEventDestroy(pr.second);
            }
        }
    }
};

// An attribute-only handle (sknnr_index_create_targets) has no reference rows: whatever searches, or configures a search,
// refuses it before any device work.
static int refuse_targets_only(const char* entry) {
    return fail(SKNNR_ERR_INVALID, "%s: the handle holds a target table only (sknnr_index_create_targets): it has no "
                "reference rows to search; it serves the from-neighbours entries and replay streams", entry);
}

// ----------------------------------------------------------------------------------------
// misc entry points
// ----------------------------------------------------------------------------------------
extern "C" int32_t sknnr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int32_t sknnr_abi_version(void) { return SKNNR_ABI_VERSION; }

extern "C" const char* sknnr_last_error(void) { return g_last_error.c_str(); }

extern "C" int sknnr_index_shape(const sknnr_index* ix, int64_t* n_ref, int32_t* d, int32_t* t,
                                 int32_t* d_in, int32_t* device) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (n_ref) *n_ref = ix->n_ref;
    if (d) *d = ix->d;
    if (t) *t = ix->t;
    if (d_in) *d_in = ix->has_affine ? ix->d_in : (ix->has_forest ? ix->f_d_in : ix->d);
    if (device) *device = ix->device;
    return SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// index construction
// ----------------------------------------------------------------------------------------
// Decide the order of the reference image by replaying the pre-filter's visit rule on a sample:
// 64 pseudo-queries (a sampled row displaced by 0.35 x the difference of two others) sweep up to
// 8192 sampled rows in tiles of 32, once in the caller's order and once by increasing centred norm,
// keeping the 6 best per query; the order with fewer visited (tile, 32-query block) pairs wins, an
// order other than the caller's only by a clear margin.
// Squared Mahalanobis norms of the rows about `mu` (covariance from up to 65536 evenly spaced rows,
// a small ridge, Cholesky, one forward substitution per row): the density order of a correlated cloud.
// Skipped (returns false) when it would cost more than ~4e9 multiply-adds on the host.
static bool mahalanobis_norms(const double* ref, int64_t n_ref, int d, const std::vector<double>& mu,
                              std::vector<double>& out) {
    if ((double)n_ref * d * d > 8e9 || n_ref < 2 * (int64_t)d) return false;
    const int64_t n_cov = std::min<int64_t>(n_ref, 65536), stride = n_ref / n_cov;
    std::vector<double> cov((size_t)d * d, 0.0), v((size_t)d);
    for (int64_t i = 0; i < n_cov; ++i) {
        const double* r = ref + i * stride * d;
        for (int a = 0; a < d; ++a) v[(size_t)a] = r[a] - mu[(size_t)a];
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) cov[(size_t)a * d + b] += v[(size_t)a] * v[(size_t)b];
    }
    double tr = 0.0;
    for (int a = 0; a < d; ++a) {
        for (int b = 0; b <= a; ++b) cov[(size_t)a * d + b] /= (double)n_cov;
        tr += cov[(size_t)a * d + a];
    }
    if (!(tr > 0.0)) return false;
    for (int a = 0; a < d; ++a) cov[(size_t)a * d + a] += 1e-9 * tr / d;
    // in-place Cholesky, lower triangle
    for (int a = 0; a < d; ++a) {
        for (int b = 0; b <= a; ++b) {
            double sum = cov[(size_t)a * d + b];
            for (int k = 0; k < b; ++k) sum -= cov[(size_t)a * d + k] * cov[(size_t)b * d + k];
            if (a == b) {
                if (!(sum > 0.0)) return false;
                cov[(size_t)a * d + a] = std::sqrt(sum);
            } else {
                cov[(size_t)a * d + b] = sum / cov[(size_t)b * d + b];
            }
        }
    }
    out.resize((size_t)n_ref);
    const unsigned n_thr = std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < n_thr; ++t)
        th.emplace_back([&, t] {
            std::vector<double> z((size_t)d);
            for (int64_t i = t; i < n_ref; i += n_thr) {
                const double* r = ref + i * d;
                double m2 = 0.0;
                for (int a = 0; a < d; ++a) {
                    double sum = r[a] - mu[(size_t)a];
                    for (int k = 0; k < a; ++k) sum -= cov[(size_t)a * d + k] * z[(size_t)k];
                    z[(size_t)a] = sum / cov[(size_t)a * d + a];
                    m2 += z[(size_t)a] * z[(size_t)a];
                }
                out[(size_t)i] = m2;
            }
        });
    for (auto& t : th) t.join();
    return true;
}

// Replay of the pre-filter's visit rule on a sample, shared by the choices below: 64 pseudo-queries (a sampled row
// displaced by 0.35 x the difference of two others) sweep up to 8192 sampled rows in tiles of 32, keeping the 6 best
// per query; counted are the (tile, 32-query block) pairs in which some query of the block has a value below its
// threshold as of the start of the tile.
struct OrderSim {
    const double* ref;
    int64_t n_ref;
    int d, S, NQ = 64, J = 6;
    int64_t stride;
    std::vector<int> sample;
    std::vector<double> q;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    OrderSim(const double* ref_, int64_t n_ref_, int d_) : ref(ref_), n_ref(n_ref_), d(d_) {
        S = (int)std::min<int64_t>(n_ref, 8192);
        stride = n_ref / S;
        sample.resize(S);
        for (int i = 0; i < S; ++i) sample[i] = (int)(i * stride);
        q.resize((size_t)NQ * d);
        auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (int64_t)(rng % (uint64_t)n_ref); };
        for (int i = 0; i < NQ; ++i) {
            const int64_t a = next(), b = next(), c = next();
            for (int k = 0; k < d; ++k) q[(size_t)i * d + k] = ref[a * d + k] + 0.35 * (ref[b * d + k] - ref[c * d + k]);
        }
    }
    // `order`: S row ids; `start` (optional): per query, the position of `order` at which its sweep begins (rotation)
    long visits(const std::vector<int>& order, const std::vector<int>* start = nullptr) const {
        std::vector<double> best((size_t)NQ * J, std::numeric_limits<double>::infinity());
        long n_vis = 0;
        for (int t0 = 0; t0 + 32 <= S; t0 += 32) {
            for (int qb = 0; qb < NQ / 32; ++qb) {
                bool any = false;
                for (int qi = qb * 32; qi < qb * 32 + 32; ++qi) {
                    double* bq = &best[(size_t)qi * J];
                    const double thr = bq[J - 1];  // threshold as of the start of the tile, like the kernel's
                    const int base = start ? (*start)[(size_t)qi] : 0;
                    for (int r = t0; r < t0 + 32; ++r) {
                        const double* rr = ref + (int64_t)order[(size_t)((base + r) % S)] * d;
                        double d2 = 0.0;
                        for (int k = 0; k < d; ++k) {
                            const double t = q[(size_t)qi * d + k] - rr[k];
                            d2 += t * t;
                        }
                        if (d2 < thr) {
                            any = true;
                            if (d2 < bq[J - 1]) {
                                int p = J - 1;
                                while (p > 0 && bq[p - 1] > d2) { bq[p] = bq[p - 1]; --p; }
                                bq[p] = d2;
                            }
                        }
                    }
                }
                n_vis += any;
            }
        }
        return n_vis;
    }
};

// returns 0: the caller's order, 1: increasing centred norm, 2: a fixed pseudo-random shuffle (for callers
// whose rows are sorted by something that correlates with the features: the first tiles would then
// cover one corner of the cloud only)
// (... 3: increasing Mahalanobis norm, when `mnorm` is available); *best_visits: the winner's visit count
static int choose_image_order(OrderSim& sim, const std::vector<double>& cnorm, const std::vector<double>* mnorm, long* best_visits) {
    *best_visits = -1;
    if (std::getenv("SKNNR_IMAGE_ORDER")) return std::atoi(std::getenv("SKNNR_IMAGE_ORDER"));
    if (sim.n_ref < 2048) return 0;
    const int S = sim.S;
    std::vector<int> by_norm(sim.sample);
    std::stable_sort(by_norm.begin(), by_norm.end(), [&](int a, int b) { return cnorm[(size_t)a] < cnorm[(size_t)b]; });
    // the sample in a fixed pseudo-random order (a strided walk is already spread over the rows; the
    // shuffle removes what is left of the caller's ordering)
    std::vector<int> shuffled(sim.sample);
    uint64_t rng = sim.rng;
    for (int i = S - 1; i > 0; --i) {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        std::swap(shuffled[i], shuffled[(int)(rng % (uint64_t)(i + 1))]);
    }
    // caller's order on CONSECUTIVE rows (what the image would really hold tile by tile)
    std::vector<int> head(S);
    for (int i = 0; i < S; ++i) head[i] = i;
    const long v_orig = std::max(sim.visits(sim.sample), sim.visits(head)), v_norm = sim.visits(by_norm), v_shuf = sim.visits(shuffled);
    long best = v_orig;
    int choice = 0;
    if (v_shuf * 100 < best * 93) { best = v_shuf; choice = 2; }
    if (v_norm * 100 < best * 93) { best = v_norm; choice = 1; }
    if (mnorm) {
        std::vector<int> by_mah(sim.sample);
        std::stable_sort(by_mah.begin(), by_mah.end(), [&](int a, int b) { return (*mnorm)[(size_t)a] < (*mnorm)[(size_t)b]; });
        const long v_mah = sim.visits(by_mah);
        if (v_mah * 100 < best * (choice == 0 ? 93 : 97)) { best = v_mah; choice = 3; }
    }
    *best_visits = best;
    return choice;
}

// ----------------------------------------------------------------------------------------
// cell order of the second-generation image (bucket.hip.h)
// ----------------------------------------------------------------------------------------
namespace {

// Eigenvectors of a symmetric d x d matrix (cyclic Jacobi), sorted by decreasing eigenvalue: vec[i * d + k] = k-th
// component of the i-th vector.
void symmetric_eigen(std::vector<double> a, int d, std::vector<double>& val, std::vector<double>& vec) {
    std::vector<double> v((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i) v[(size_t)i * d + i] = 1.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) off += a[(size_t)p * d + q] * a[(size_t)p * d + q];
        if (off < 1e-22) break;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = a[(size_t)p * d + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (a[(size_t)q * d + q] - a[(size_t)p * d + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < d; ++k) {  // columns p, q
                    const double akp = a[(size_t)k * d + p], akq = a[(size_t)k * d + q];
                    a[(size_t)k * d + p] = c * akp - sn * akq;
                    a[(size_t)k * d + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < d; ++k) {  // rows p, q
                    const double apk = a[(size_t)p * d + k], aqk = a[(size_t)q * d + k];
                    a[(size_t)p * d + k] = c * apk - sn * aqk;
                    a[(size_t)q * d + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < d; ++k) {  // accumulate the rotation (columns of v are the vectors)
                    const double vkp = v[(size_t)k * d + p], vkq = v[(size_t)k * d + q];
                    v[(size_t)k * d + p] = c * vkp - sn * vkq;
                    v[(size_t)k * d + q] = sn * vkp + c * vkq;
                }
            }
    }
    std::vector<int> order(d);
    for (int i = 0; i < d; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * d + x] > a[(size_t)y * d + y]; });
    val.resize(d);
    vec.assign((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i) {
        val[i] = a[(size_t)order[i] * d + order[i]];
        for (int k = 0; k < d; ++k) vec[(size_t)i * d + k] = v[(size_t)k * d + order[i]];
    }
}

struct CellTree {
    int depth = 0;
    std::vector<float> axes, centre, thr;  // [depth][d], [d], [2^depth - 1]
    std::vector<int> code;                 // cell of every reference row
};

// Median-split tree over the `depth` leading principal axes of the centred reference rows: level l splits every
// node at the median of its rows' coordinate along axis l.  The reference rows are compared with the same float32
// arithmetic as the device uses for the queries (cell_hist_kernel), so a query that IS a reference row lands in
// that row's cell.
CellTree build_cell_tree(const double* ref, int64_t n_ref, int d, const std::vector<double>& mu, int depth) {
    CellTree t;
    t.depth = depth;
    const int64_t n_cov = std::min<int64_t>(n_ref, 65536), stride = n_ref / n_cov;
    std::vector<double> cov((size_t)d * d, 0.0), v((size_t)d);
    for (int64_t i = 0; i < n_cov; ++i) {
        const double* r = ref + i * stride * d;
        for (int a = 0; a < d; ++a) v[(size_t)a] = r[a] - mu[(size_t)a];
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) cov[(size_t)a * d + b] += v[(size_t)a] * v[(size_t)b];
    }
    for (int a = 0; a < d; ++a)
        for (int b = 0; b <= a; ++b) cov[(size_t)b * d + a] = cov[(size_t)a * d + b] = cov[(size_t)a * d + b] / (double)n_cov;
    std::vector<double> val, vec;
    symmetric_eigen(cov, d, val, vec);
    t.axes.resize((size_t)depth * d);
    t.centre.resize((size_t)d);
    for (int l = 0; l < depth; ++l)
        for (int k = 0; k < d; ++k) t.axes[(size_t)l * d + k] = (float)vec[(size_t)l * d + k];
    for (int k = 0; k < d; ++k) t.centre[(size_t)k] = (float)mu[(size_t)k];
    // coordinates of every row along the axes (the device's arithmetic: float32 fma chain over k)
    std::vector<float> z((size_t)n_ref * depth);
    for (int64_t i = 0; i < n_ref; ++i) {
        float acc[kCellMaxDepth] = {};
        for (int k = 0; k < d; ++k) {
            const float x = (float)ref[i * d + k] - t.centre[(size_t)k];
            for (int l = 0; l < depth; ++l) acc[l] = std::fmaf(x, t.axes[(size_t)l * d + k], acc[l]);
        }
        for (int l = 0; l < depth; ++l) z[(size_t)i * depth + l] = acc[l];
    }
    t.thr.assign(((size_t)1 << depth) - 1, 0.f);
    t.code.assign((size_t)n_ref, 0);
    std::vector<std::vector<int>> nodes(1);
    nodes[0].resize((size_t)n_ref);
    for (int64_t i = 0; i < n_ref; ++i) nodes[0][(size_t)i] = (int)i;
    for (int l = 0; l < depth; ++l) {
        std::vector<std::vector<int>> next(nodes.size() * 2);
        for (size_t n = 0; n < nodes.size(); ++n) {
            std::vector<int>& rows = nodes[n];
            float split = 0.f;
            if (!rows.empty()) {
                std::vector<float> zz(rows.size());
                for (size_t j = 0; j < rows.size(); ++j) zz[j] = z[(size_t)rows[j] * depth + l];
                std::nth_element(zz.begin(), zz.begin() + zz.size() / 2, zz.end());
                split = zz[zz.size() / 2];
            }
            t.thr[((size_t)1 << l) - 1 + n] = split;
            for (int r : rows) next[2 * n + (z[(size_t)r * depth + l] >= split ? 1 : 0)].push_back(r);
        }
        nodes.swap(next);
    }
    for (size_t n = 0; n < nodes.size(); ++n)
        for (int r : nodes[n]) t.code[(size_t)r] = (int)n;
    return t;
}

}  // namespace

extern "C" int sknnr_index_create(const double* ref, int64_t n_ref, int32_t d, const double* y,
                                  int32_t t, int32_t device, sknnr_index** out) {
    if (!out) return fail(SKNNR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ref || n_ref < 1 || d < 1) return fail(SKNNR_ERR_INVALID, "ref must be a non-empty (n_ref, d) matrix");
    if (n_ref > 0x7fffff00L) return fail(SKNNR_ERR_UNSUPPORTED, "n_ref = %ld exceeds 2^31 - 256", (long)n_ref);
    if (y && t < 1) return fail(SKNNR_ERR_INVALID, "t must be >= 1 when y is given");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)
        return fail(SKNNR_ERR_NO_DEVICE, "no HIP device is visible");
    if (device < 0 || device >= n_dev) return fail(SKNNR_ERR_INVALID, "device %d out of range [0, %d)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    {
        // every value finite (the reference's fit validates the same way: SKL/utils/validation.py, ensure_all_finite);
        // x - x is 0 for finite x and NaN for NaN and +-inf
        double bad = 0.0;
        const size_t total = (size_t)n_ref * (size_t)d;
        for (size_t i = 0; i < total; ++i) bad += ref[i] - ref[i];
        if (bad != 0.0) {
            for (size_t i = 0; i < total; ++i)
                if (ref[i] != ref[i]) return fail(SKNNR_ERR_NONFINITE, "Input X contains NaN.");
            return fail(SKNNR_ERR_NONFINITE, "Input X contains infinity or a value too large for dtype('float64').");
        }
    }

    sknnr_index* ix = new (std::nothrow) sknnr_index();
    if (!ix) return fail(SKNNR_ERR_INVALID, "out of host memory");
    struct Guard {
        sknnr_index* p;
        ~Guard() { delete p; }
    } guard{ix};
    ix->device = device;
    ix->n_ref = n_ref;
    ix->d = d;
    ix->t = y ? t : 0;

    const size_t nd = (size_t)n_ref * d;
    HIP_TRY(ix->ref64.ensure(nd));
    HIP_TRY(hipMemcpy(ix->ref64.p, ref, nd * sizeof(double), hipMemcpyHostToDevice));
    {
        std::vector<double> tr(nd);
        for (int64_t i = 0; i < n_ref; ++i)
            for (int c = 0; c < d; ++c) tr[(size_t)c * n_ref + i] = ref[(size_t)i * d + c];
        HIP_TRY(ix->refT.ensure(nd));
        HIP_TRY(hipMemcpy(ix->refT.p, tr.data(), nd * sizeof(double), hipMemcpyHostToDevice));
    }
    HIP_TRY(ix->rn64.ensure(n_ref));
    HIP_TRY(launch::row_norms(ix->ref64.p, n_ref, d, ix->rn64.p, nullptr));
    if (y) {
        HIP_TRY(ix->y64.ensure((size_t)n_ref * t));
        HIP_TRY(hipMemcpy(ix->y64.p, y, (size_t)n_ref * t * sizeof(double), hipMemcpyHostToDevice));
    }

    // ---- coarse image: centred, power-of-two scaled, split into f16 hi/lo, fragment order
    const int ks = (d + 15) / 16;
    if (ks <= kMaxKs) {
        ix->ks = ks;
        const int dp = 16 * ks;
        ix->mu.assign(dp, 0.0);
        for (int c = 0; c < d; ++c) {
            long double acc = 0;
            for (int64_t i = 0; i < n_ref; ++i) acc += ref[i * d + c];
            ix->mu[c] = (double)(acc / n_ref);
        }
        double amax = 0.0;
        for (int64_t i = 0; i < n_ref; ++i)
            for (int c = 0; c < d; ++c) amax = std::max(amax, std::fabs(ref[i * d + c] - ix->mu[c]));
        if (!(amax < std::numeric_limits<double>::infinity()))
            return fail(SKNNR_ERR_INVALID, "reference rows contain non-finite values");
        // A = -2 s (r - mu) must stay <= 256 in magnitude: 2 s amax <= 256
        int e = 0;
        if (amax > 0.0) {
            (void)std::frexp(amax, &e);  // amax = f * 2^e, f in [0.5, 1)
            e = 7 - e;                   // s * amax in [64, 128)
        }
        ix->s = std::ldexp(1.0, e);
        const double s = ix->s;

        // Image order: the caller's, or reference rows by increasing centred norm.  In a high-dimensional
        // cloud a row near the centre is, on average, closer to every query than a far one
        // (d2 = |q'|^2 + |r'|^2 - 2 q'.r'): the lists fill with good candidates early and later tiles
        // are visited less often (benchmark law, 32-D: 31.6 % -> 24.6 % of the tile x q-block tests;
        // 10M x 50k x 64: 83 -> 101 Mq/s).  In few dimensions the norms spread widely and the centre
        // rows are poor candidates for most queries (8-D, 100k rows: 193 -> 148 Mq/s), so the choice is
        // made per index by replaying the candidate orders on a sample (choose_image_order).  `perm` maps an
        // image position back to the caller's row index; only the finaliser needs it.
        std::vector<double> cnorm((size_t)n_ref);
        for (int64_t i = 0; i < n_ref; ++i) {
            double yn = 0.0;
            for (int c = 0; c < d; ++c) {
                const double b = s * (ref[i * d + c] - ix->mu[c]);
                yn += b * b;
            }
            cnorm[(size_t)i] = yn;
        }
        std::vector<int> perm((size_t)n_ref);
        for (int64_t i = 0; i < n_ref; ++i) perm[(size_t)i] = (int)i;
        std::vector<double> mnorm;
        const char* forced = std::getenv("SKNNR_IMAGE_ORDER");
        const bool have_mah = (!forced || std::atoi(forced) == 3) && n_ref >= 2048 && mahalanobis_norms(ref, n_ref, d, ix->mu, mnorm);
        OrderSim sim(ref, n_ref, d);
        long order_visits = -1;
        int image_order = choose_image_order(sim, cnorm, have_mah ? &mnorm : nullptr, &order_visits);
        if (image_order == 3 && !have_mah) image_order = 1;
        if (image_order == 1) {
            std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return cnorm[(size_t)a] < cnorm[(size_t)b]; });
        } else if (image_order == 3) {
            std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return mnorm[(size_t)a] < mnorm[(size_t)b]; });
        } else if (image_order == 2) {
            uint64_t rs = 0xD1B54A32D192ED03ull;
            for (int64_t i = n_ref - 1; i > 0; --i) {
                rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17;
                std::swap(perm[(size_t)i], perm[(size_t)(rs % (uint64_t)(i + 1))]);
            }
        }

        // One 32-reference tile of an image: hi / lo fragments in MFMA A-fragment order and the |r'|^2 block in
        // accumulator order, for the rows order[32 tile .. 32 tile + 31]
        auto fill_tile = [&](const std::vector<int>& order, long tile, uint16_t* frag_hi, uint16_t* frag_lo, float* ci) {
            for (int step = 0; step < ks; ++step)
                for (int lane = 0; lane < 64; ++lane) {
                    const long pos = tile * 32 + (lane & 31);
                    const long row = pos < n_ref ? order[(size_t)pos] : -1;
                    for (int j = 0; j < 8; ++j) {
                        const int k = step * 16 + 8 * (lane >> 5) + j;
                        double a = 0.0;
                        if (row >= 0 && k < d) a = -2.0 * s * (ref[row * d + k] - ix->mu[k]);
                        const uint16_t hi = f64_to_f16_bits(a);
                        frag_hi[((size_t)step * 64 + lane) * 8 + j] = hi;
                        frag_lo[((size_t)step * 64 + lane) * 8 + j] = f64_to_f16_bits(a - f16_bits_to_f64(hi));
                    }
                }
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r) {
                    const long pos = tile * 32 + acc_row(r, h);
                    ci[h * 16 + r] = pos < n_ref ? (float)cnorm[(size_t)order[(size_t)pos]] : std::numeric_limits<float>::infinity();
                }
        };
        double ymax2 = 0.0;
        for (int64_t i = 0; i < n_ref; ++i) ymax2 = std::max(ymax2, cnorm[(size_t)i]);
        ix->ymax = std::sqrt(ymax2);

        const int tps = tiles_per_stage(ks);
        const long n_tiles = ((n_ref + 31) / 32 + tps - 1) / tps * tps;
        ix->n_stages = (int)(n_tiles / tps);
        const size_t tb = tile_bytes(ks);
        std::vector<char> img(n_tiles * tb);
        for (long tile = 0; tile < n_tiles; ++tile) {
            char* rec = img.data() + tile * tb;
            fill_tile(perm, tile, reinterpret_cast<uint16_t*>(rec), reinterpret_cast<uint16_t*>(rec + (size_t)ks * 1024),
                      reinterpret_cast<float*>(rec + tile_frag_bytes(ks)));
        }
        if (ks <= 4) {
            // second-generation kernel: hi fragments + |r'|^2 per tile (staged through LDS), lo fragments in an
            // array of their own (read from L2 by the flush only)
            const int tps2 = tiles_per_stage2(ks);
            ix->n_stages2 = image_stages2(n_ref, ks);
            const long n_tiles2 = (long)ix->n_stages2 * tps2;
            // ... in CELL order when the kernel will serve this index (bucket.hip.h): rows sorted by the cell of a
            // median-split tree over the leading principal axes (inside a cell: by centred norm), so that a workgroup
            // whose query rows were bucketed by the same tree starts its sweep among their neighbours
            std::vector<int> perm2(perm);
            int depth = 0;
            {
                const char* e = std::getenv("SKNNR_CELLS");
                int want = e ? std::atoi(e) : kCellMaxDepth;
                want = std::min(want, std::min(kCellMaxDepth, (int)d));
                while (want > 0 && (n_ref >> want) < 512) --want;  // cells of at least 512 rows (one 16-tile stage)
                if (n_tiles2 >= 2 * kSeedTiles && want >= 2) depth = want;
            }
            const bool cells_forced = std::getenv("SKNNR_CELLS") != nullptr;
            CellTree tree;
            auto mix = [](uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; };
            if (depth > 0) {
                tree = build_cell_tree(ref, n_ref, d, ix->mu, depth);
                if (!cells_forced && order_visits > 0) {
                    // Does the cell order pay for THIS reference set?  The same replay as for the other orders, every
                    // pseudo-query starting its sweep around its own cell.  Isotropic clouds (whitened Mahalanobis
                    // spaces, uniform hypercubes) have no leading axes to split along: they keep the order chosen above
                    // (measured, 10M x 50k x 64 Mahalanobis: 68 ms by norm, 91 ms by cells).
                    std::vector<int> by_cell(sim.sample);
                    std::stable_sort(by_cell.begin(), by_cell.end(), [&](int a, int b) {
                        if (tree.code[(size_t)a] != tree.code[(size_t)b]) return tree.code[(size_t)a] < tree.code[(size_t)b];
                        return mix((uint32_t)a) < mix((uint32_t)b);
                    });
                    const int n_cells = 1 << depth;
                    std::vector<int> first_s((size_t)n_cells + 1, sim.S);
                    for (int pos = sim.S - 1; pos >= 0; --pos) first_s[(size_t)tree.code[(size_t)by_cell[(size_t)pos]]] = pos;
                    for (int c = n_cells - 1; c >= 0; --c)
                        if (first_s[(size_t)c] == sim.S) first_s[(size_t)c] = first_s[(size_t)c + 1];
                    const int window = std::max<int>(32, (int)((int64_t)seed_tiles_for(n_tiles2, tps2) * 32 * sim.S / n_ref));
                    std::vector<int> start((size_t)sim.NQ);
                    for (int qi = 0; qi < sim.NQ; ++qi) {
                        int node = 0;
                        for (int l = 0; l < depth; ++l) {
                            float z = 0.f;
                            for (int k = 0; k < d; ++k)
                                z = std::fmaf((float)sim.q[(size_t)qi * d + k] - tree.centre[(size_t)k], tree.axes[(size_t)l * d + k], z);
                            node = 2 * node + (z >= tree.thr[((size_t)1 << l) - 1 + node] ? 1 : 0);
                        }
                        const int mid = (first_s[(size_t)node] + first_s[(size_t)node + 1]) / 2;
                        start[(size_t)qi] = ((mid - window / 2) % sim.S + sim.S) % sim.S;
                    }
                    const long v_cell = sim.visits(by_cell, &start);
                    if (v_cell * 100 >= order_visits * 85) depth = 0;
                    if (std::getenv("SKNNR_ORDER_TRACE"))
                        std::fprintf(stderr, "[order] best plain order %d: %ld visits; cell order (depth %d): %ld visits -> %s\n", image_order,
                                     order_visits, tree.depth, v_cell, depth ? "cells" : "plain");
                }
            }
            if (depth > 0) {
                for (int64_t i = 0; i < n_ref; ++i) perm2[(size_t)i] = (int)i;
                // (inside a cell: a fixed pseudo-random order -- sorted by norm, a query's nearest rows would share a few
                //  tiles and overflow the per-lane hit queues there)
                const bool by_norm = std::getenv("SKNNR_CELL_NORM_ORDER") != nullptr;
                std::stable_sort(perm2.begin(), perm2.end(), [&](int a, int b) {
                    if (tree.code[(size_t)a] != tree.code[(size_t)b]) return tree.code[(size_t)a] < tree.code[(size_t)b];
                    if (by_norm) return cnorm[(size_t)a] < cnorm[(size_t)b];
                    return mix((uint32_t)a) < mix((uint32_t)b);
                });
                const int n_cells = 1 << depth;
                std::vector<long> first((size_t)n_cells + 1, n_ref);
                for (int64_t pos = n_ref - 1; pos >= 0; --pos) first[(size_t)tree.code[(size_t)perm2[(size_t)pos]]] = pos;
                for (int c = n_cells - 1; c >= 0; --c)
                    if (first[(size_t)c] == n_ref) first[(size_t)c] = first[(size_t)c + 1];  // empty cell: its successor's place
                std::vector<int> stage((size_t)n_cells);
                for (int c = 0; c < n_cells; ++c) {
                    // the seed window (kSeedTiles tiles) is centred on the cell
                    const long mid_tile = (first[(size_t)c] + first[(size_t)c + 1]) / 2 / 32;
                    const long half = seed_tiles_for(n_tiles2, tps2) / 2;
                    long st = (mid_tile - half) / tps2;
                    if (mid_tile - half < 0) st = ix->n_stages2 + (mid_tile - half - tps2 + 1) / tps2;
                    stage[(size_t)c] = (int)(((st % ix->n_stages2) + ix->n_stages2) % ix->n_stages2);
                }
                HIP_TRY(ix->cell_axes.ensure(tree.axes.size()));
                HIP_TRY(hipMemcpy(ix->cell_axes.p, tree.axes.data(), tree.axes.size() * sizeof(float), hipMemcpyHostToDevice));
                HIP_TRY(ix->cell_centre.ensure(tree.centre.size()));
                HIP_TRY(hipMemcpy(ix->cell_centre.p, tree.centre.data(), tree.centre.size() * sizeof(float), hipMemcpyHostToDevice));
                HIP_TRY(ix->cell_thr.ensure(tree.thr.size()));
                HIP_TRY(hipMemcpy(ix->cell_thr.p, tree.thr.data(), tree.thr.size() * sizeof(float), hipMemcpyHostToDevice));
                HIP_TRY(ix->cell_stage.ensure(stage.size()));
                HIP_TRY(hipMemcpy(ix->cell_stage.p, stage.data(), stage.size() * sizeof(int), hipMemcpyHostToDevice));
                HIP_TRY(ix->cell_hist.ensure(2 * kCellMax));
                ix->cell_depth = depth;
            }
            const size_t tb2 = tile2_bytes(ks), lob = (size_t)ks * 1024;
            std::vector<char> hi2(n_tiles2 * tb2, 0), lo2(n_tiles2 * lob, 0);
            for (long tile = 0; tile < n_tiles2; ++tile)
                fill_tile(perm2, tile, reinterpret_cast<uint16_t*>(hi2.data() + tile * tb2),
                          reinterpret_cast<uint16_t*>(lo2.data() + tile * lob), reinterpret_cast<float*>(hi2.data() + tile * tb2 + lob));
            HIP_TRY(ix->rhi2.ensure(hi2.size()));
            HIP_TRY(hipMemcpy(ix->rhi2.p, hi2.data(), hi2.size(), hipMemcpyHostToDevice));
            HIP_TRY(ix->rlo2.ensure(lo2.size()));
            HIP_TRY(hipMemcpy(ix->rlo2.p, lo2.data(), lo2.size(), hipMemcpyHostToDevice));
            HIP_TRY(ix->perm2.ensure((size_t)n_ref));
            HIP_TRY(hipMemcpy(ix->perm2.p, perm2.data(), (size_t)n_ref * sizeof(int), hipMemcpyHostToDevice));
        }
        {
            double m2 = 0.0;
            for (int c = 0; c < d; ++c) m2 += ix->mu[c] * ix->mu[c];
            ix->mu_norm = std::sqrt(m2) * (1.0 + 1e-12);
        }
        HIP_TRY(ix->rimg.ensure(img.size()));
        HIP_TRY(hipMemcpy(ix->rimg.p, img.data(), img.size(), hipMemcpyHostToDevice));
        HIP_TRY(ix->perm.ensure((size_t)n_ref));
        HIP_TRY(hipMemcpy(ix->perm.p, perm.data(), (size_t)n_ref * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(ix->mu_dev.ensure(dp));
        HIP_TRY(hipMemcpy(ix->mu_dev.p, ix->mu.data(), dp * sizeof(double), hipMemcpyHostToDevice));
    }

    HIP_TRY(ix->fail_count.ensure(4));
    HIP_TRY(ix->resc_state.ensure(kRescueWords));
    ix->rescue_enabled = env_on("SKNNR_RESCUE");
    HIP_TRY(ix->fail_total.ensure(2));
    HIP_TRY(hipMemset(ix->fail_total.p, 0, 16));
    HIP_TRY(ix->status.ensure(4));
    HIP_TRY(hipMemset(ix->status.p, 0, 16));
    HIP_TRY(hipEventCreateWithFlags(&ix->ev_ws, hipEventDisableTiming));
    HIP_TRY(hipDeviceSynchronize());
    guard.p = nullptr;
    *out = ix;
    return SKNNR_OK;
}

extern "C" void sknnr_index_destroy(sknnr_index* ix) { delete ix; }

extern "C" int sknnr_index_set_affine(sknnr_index* ix, int32_t d_in, const double* center,
                                      const double* scale, const double* proj) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_index_set_affine");
    if (d_in < 1) return fail(SKNNR_ERR_INVALID, "d_in must be >= 1");
    if (!proj && d_in != ix->d)
        return fail(SKNNR_ERR_INVALID, "without a projection d_in (%d) must equal d (%d)", d_in, ix->d);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // a call still running may be reading the previous map
    ix->d_in = d_in;
    ix->has_center = center != nullptr;
    ix->has_scale = scale != nullptr;
    ix->has_proj = proj != nullptr;
    if (center) {
        HIP_TRY(ix->center.ensure(d_in));
        HIP_TRY(hipMemcpy(ix->center.p, center, d_in * sizeof(double), hipMemcpyHostToDevice));
    }
    if (scale) {
        HIP_TRY(ix->scale.ensure(d_in));
        HIP_TRY(hipMemcpy(ix->scale.p, scale, d_in * sizeof(double), hipMemcpyHostToDevice));
    }
    if (proj) {
        const int dp = ix->ks > 0 ? 16 * ix->ks : ((ix->d + 15) / 16) * 16;
        std::vector<double> padded((size_t)d_in * dp, 0.0);
        for (int c = 0; c < d_in; ++c)
            for (int j = 0; j < ix->d; ++j) padded[(size_t)c * dp + j] = proj[(size_t)c * ix->d + j];
        HIP_TRY(ix->proj.ensure(padded.size()));
        HIP_TRY(hipMemcpy(ix->proj.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    ix->has_affine = true;
    return SKNNR_OK;
}

extern "C" int sknnr_index_set_hamming_weights(sknnr_index* ix, const double* w, int32_t n) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_index_set_hamming_weights");
    if (!w || n != ix->d) return fail(SKNNR_ERR_INVALID, "w must hold one weight per column (%d), got %d", ix->d, n);
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!(w[i] >= 0.0) || !(w[i] < std::numeric_limits<double>::infinity()))
            return fail(SKNNR_ERR_INVALID, "Hamming weights must be finite and non-negative");
        total += w[i];  // index order, as scipy's cdist accumulates it
    }
    if (!(total > 0.0)) return fail(SKNNR_ERR_INVALID, "Hamming weights must not sum to zero");
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(ix->hw.ensure(n));
    HIP_TRY(hipMemcpy(ix->hw.p, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    ix->hw_sum = total;
    ix->has_hw = true;
    // the integer image for the pre-filter (hamming.hip.h): reference ids as 16-bit integers, weights scaled to 16 bits
    ix->h16_ok = false;
    if (!std::getenv("SKNNR_HAMMING_INT") || std::atoi(std::getenv("SKNNR_HAMMING_INT")) != 0) {
        const int tp = (n + 1) / 2;
        const int ref_pad = (int)((ix->n_ref + kHamWaves * 64 - 1) / (kHamWaves * 64) * (kHamWaves * 64));
        double wmax = 0.0;
        for (int i = 0; i < n; ++i) wmax = std::max(wmax, w[i]);
        std::vector<uint32_t> wq((size_t)tp, 0u);
        for (int i = 0; i < n; ++i) {
            // (w / wmax first: it is in [0, 1] for any weights, where 65535 / wmax overflows to inf once
            //  wmax < 65535 / DBL_MAX and every weight, zeros included (0 inf = NaN), came out as 65535)
            const uint32_t q16 = (uint32_t)std::min(65535.0, std::floor(w[i] / wmax * 65535.0 + 0.5));
            wq[(size_t)i / 2] |= q16 << (16 * (i & 1));
        }
        HIP_TRY(ix->h_wq.ensure((size_t)tp));
        HIP_TRY(hipMemcpy(ix->h_wq.p, wq.data(), (size_t)tp * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(ix->h_rimg.ensure((size_t)tp * ref_pad));
        DevBuf<int> bad;
        HIP_TRY(bad.ensure((size_t)ref_pad));
        HIP_TRY(launch::hamming_pack(ix->ref64.p, ix->n_ref, ref_pad, n, tp, ix->h_rimg.p, bad.p, nullptr));
        std::vector<int> hb((size_t)ref_pad);
        HIP_TRY(hipMemcpy(hb.data(), bad.p, (size_t)ref_pad * sizeof(int), hipMemcpyDeviceToHost));
        bool any_bad = false;
        for (int v : hb) any_bad = any_bad || v != 0;
        const int tpr = ham_row_dwords(n);
        bool rows_ok = n <= 4096 && hamming_rescore_lds(n) <= kLdsLimit;
        if (rows_ok && ix->h_rrow.ensure((size_t)ix->n_ref * tpr) != hipSuccess) {
            // (the row-major image takes a KiB per row and 512 trees: when it does not fit, the float64 scan serves the index)
            (void)hipGetLastError();
            rows_ok = false;
        }
        if (rows_ok) {
            HIP_TRY(launch::hamming_rows(ix->ref64.p, ix->n_ref, n, tpr, ix->h_rrow.p, nullptr));
            HIP_TRY(hipDeviceSynchronize());
        }
        ix->h_tp = tp;
        ix->h_ref_pad = ref_pad;
        // (more than 3,584 trees: the float64 scan -- the re-score's dynamic LDS, 16 ceil(T / 2) + 16,384 ceil(T / 512)
        //  bytes, passes 150 KiB at T = 3,585; the 4,096 above is the re-score's register image, never the binding limit)
        ix->h16_ok = !any_bad && rows_ok;
    }
    return SKNNR_OK;
}

extern "C" int sknnr_index_set_forest(sknnr_index* ix, int32_t d_in, int32_t n_trees, const int64_t* tree_offset,
                                      const double* threshold, const int32_t* feature, const int32_t* left,
                                      const int32_t* right) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_index_set_forest");
    if (d_in < 1) return fail(SKNNR_ERR_INVALID, "d_in must be >= 1");
    if (n_trees != ix->d) return fail(SKNNR_ERR_INVALID, "the forests have %d trees, the node-id rows %d columns", n_trees, ix->d);
    if (!tree_offset || !threshold || !feature || !left || !right) return fail(SKNNR_ERR_INVALID, "NULL forest array");
    if (tree_offset[0] != 0) return fail(SKNNR_ERR_INVALID, "tree_offset[0] must be 0");
    for (int t = 0; t < n_trees; ++t)
        if (tree_offset[t + 1] <= tree_offset[t] || tree_offset[t + 1] - tree_offset[t] > 0x7fffffffL)
            return fail(SKNNR_ERR_INVALID, "tree %d has %ld nodes", t, (long)(tree_offset[t + 1] - tree_offset[t]));
    // Termination and bounds of the device walk: children after their parent and inside the tree, features inside the
    // row.  Depths follow in one pass (a child's depth is final once every node before it is done).
    const long n_nodes = (long)tree_offset[n_trees];
    std::vector<int4> nodes((size_t)n_nodes);
    std::vector<int> depth((size_t)n_trees, 0), node_depth;
    for (int t = 0; t < n_trees; ++t) {
        const long base = (long)tree_offset[t];
        const int n_t = (int)(tree_offset[t + 1] - base);
        node_depth.assign((size_t)n_t, 0);
        for (int i = 0; i < n_t; ++i) {
            const long g = base + i;
            const int l = left[g], r = right[g];
            if (l == -1 && r == -1) {
                nodes[(size_t)g] = int4{0, 0, -1, -1};
                depth[(size_t)t] = std::max(depth[(size_t)t], node_depth[(size_t)i]);
                continue;
            }
            if (l <= i || r <= i || l >= n_t || r >= n_t)
                return fail(SKNNR_ERR_INVALID, "tree %d, node %d: children (%d, %d) must lie in (%d, %d)", t, i, l, r, i, n_t);
            if (feature[g] < 0 || feature[g] >= d_in)
                return fail(SKNNR_ERR_INVALID, "tree %d, node %d: feature %d outside [0, %d)", t, i, feature[g], d_in);
            const double thr = threshold[g];
            if (thr != thr) return fail(SKNNR_ERR_INVALID, "tree %d, node %d: threshold is NaN", t, i);
            // the largest float32 <= thr (forest.hip.h: the float32 compare is then the reference's float64 one)
            float f = (float)thr;
            if ((double)f > thr) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
            int fb;
            std::memcpy(&fb, &f, 4);
            nodes[(size_t)g] = int4{fb, feature[g], l, r};
            node_depth[(size_t)l] = std::max(node_depth[(size_t)l], node_depth[(size_t)i] + 1);
            node_depth[(size_t)r] = std::max(node_depth[(size_t)r], node_depth[(size_t)i] + 1);
        }
    }
    std::vector<long> off(tree_offset, tree_offset + n_trees);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // a call still running may be reading the previous forests
    ix->has_forest = false;
    HIP_TRY(ix->f_nodes.ensure((size_t)n_nodes));
    HIP_TRY(ix->f_off.ensure((size_t)n_trees));
    HIP_TRY(ix->f_depth.ensure((size_t)n_trees));
    HIP_TRY(hipMemcpy(ix->f_nodes.p, nodes.data(), (size_t)n_nodes * sizeof(int4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ix->f_off.p, off.data(), (size_t)n_trees * sizeof(long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ix->f_depth.p, depth.data(), (size_t)n_trees * sizeof(int), hipMemcpyHostToDevice));
    ix->f_d_in = d_in;
    ix->has_forest = true;
    return SKNNR_OK;
}

extern "C" int sknnr_affine_transform(const double* x, int64_t n, int32_t d_in, const double* center,
                                      const double* scale, const double* proj, int32_t d, double* out,
                                      int32_t device) {
    if (!x || !out || n < 0 || d_in < 1 || d < 1) return fail(SKNNR_ERR_INVALID, "bad argument");
    if (!proj && d_in != d) return fail(SKNNR_ERR_INVALID, "without a projection d_in (%d) must equal d (%d)", d_in, d);
    if (n == 0) return SKNNR_OK;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return fail(SKNNR_ERR_NO_DEVICE, "no HIP device is visible");
    if (device < 0 || device >= n_dev) return fail(SKNNR_ERR_INVALID, "device %d out of range [0, %d)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    const int ks = (d + 15) / 16, dp = 16 * ks;
    if (!prep_lds_rows(d_in))
        return fail(SKNNR_ERR_UNSUPPORTED, "d_in = %d is too wide for the transform kernel (max 299)", d_in);
    DevBuf<double> dx, dc, dsc, dpj, dout;
    int rc = SKNNR_OK;
    auto cleanup = [&]() { dx.release(); dc.release(); dsc.release(); dpj.release(); dout.release(); };
#define AT_TRY(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            cleanup();                                                                                \
            return fail(SKNNR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                \
        }                                                                                             \
    } while (0)
    std::vector<double> padded;
    if (proj) {
        padded.assign((size_t)d_in * dp, 0.0);
        for (int c = 0; c < d_in; ++c)
            for (int j = 0; j < d; ++j) padded[(size_t)c * dp + j] = proj[(size_t)c * d + j];
        AT_TRY(dpj.ensure(padded.size()));
        AT_TRY(hipMemcpy(dpj.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (center) {
        AT_TRY(dc.ensure(d_in));
        AT_TRY(hipMemcpy(dc.p, center, d_in * sizeof(double), hipMemcpyHostToDevice));
    }
    if (scale) {
        AT_TRY(dsc.ensure(d_in));
        AT_TRY(hipMemcpy(dsc.p, scale, d_in * sizeof(double), hipMemcpyHostToDevice));
    }
    const long rows = std::min<long>(n, kChunkRows);
    AT_TRY(dx.ensure((size_t)rows * d_in));
    AT_TRY(dout.ensure((size_t)rows * d));
    for (long c0 = 0; c0 < n; c0 += rows) {
        const long m = std::min<long>(rows, n - c0);
        AT_TRY(hipMemcpy(dx.p, x + c0 * d_in, (size_t)m * d_in * sizeof(double), hipMemcpyHostToDevice));
        PrepArgs a{};
        a.x = dx.p;
        a.nq = m;
        a.nq_pad = (m + 255) / 256 * 256;
        a.d_in = d_in;
        a.d = d;
        a.ks = ks;
        a.center = center ? dc.p : nullptr;
        a.scale = scale ? dsc.p : nullptr;
        a.proj = proj ? dpj.p : nullptr;
        a.xt = dout.p;
        AT_TRY(launch::prep_lds(prep_lds_rows(d_in), a, nullptr));
        AT_TRY(hipMemcpy(out + c0 * d, dout.p, (size_t)m * d * sizeof(double), hipMemcpyDeviceToHost));
    }
#undef AT_TRY
    cleanup();
    return rc;
}

// ----------------------------------------------------------------------------------------
// stats
// ----------------------------------------------------------------------------------------
// Fold one finished call record into the stats (waits for the call if it is still running).
static void resolve_call(sknnr_index* ix, sknnr_index::CallTiming& ct) {
    if (!ct.pending) return;
    ct.pending = false;
    if (hipEventSynchronize(ct.e1) != hipSuccess) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ct.e0, ct.e1) != hipSuccess) return;
    double cms = 0.0;
    for (size_t i = 0; i < ct.coarse_used; ++i) {
        float m = 0.f;
        if (hipEventElapsedTime(&m, ct.coarse[i].first, ct.coarse[i].second) == hipSuccess) cms += m;
    }
    ix->stats.last_kernel_ms = ms;
    ix->stats.last_coarse_ms = cms;
    ix->stats.total_kernel_ms += ms;
    ix->stats.total_coarse_ms += cms;
    ix->stats.timed_calls += 1;
    ix->stats.coarse_rows_timed += ct.coarse_rows;
}
static void resolve_timing(sknnr_index* ix) {
    // oldest first, so that last_* end up describing the newest call
    for (int i = 0; i < sknnr_index::kTimingRing; ++i)
        resolve_call(ix, ix->timing[(ix->timing_next + i) % sknnr_index::kTimingRing]);
}

extern "C" int sknnr_get_stats(const sknnr_index* cix, sknnr_stats* out) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    (void)hipSetDevice(ix->device);
    resolve_timing(ix);
    long long total = 0;
    if (hipMemcpy(&total, ix->fail_total.p, sizeof total, hipMemcpyDeviceToHost) == hipSuccess)
        ix->stats.exact_fallbacks = total;
    *out = ix->stats;
    launch::coarse1_dev_report();  // (development builds only: -DSKNNR_COARSE_COUNTERS / -DSKNNR_COARSE_TIMERS)
    launch::coarse2_dev_report();
    return SKNNR_OK;
}

extern "C" int sknnr_reset_stats(sknnr_index* ix) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(ix->fail_total.p, 0, 16));
    for (auto& ct : ix->timing) ct.pending = false;
    ix->stats = sknnr_stats{};
    return SKNNR_OK;
}

static int nonfinite_error(int bits) {
    if (bits & 1) return fail(SKNNR_ERR_NONFINITE, "Input X contains NaN.");
    if (bits & 2) return fail(SKNNR_ERR_NONFINITE, "Input X contains infinity or a value too large for dtype('float64').");
    // (bit 2, the forest map only: a value that is infinite as float32 -- forest.apply's own check)
    return fail(SKNNR_ERR_NONFINITE, "Input X contains infinity or a value too large for dtype('float32').");
}

// Read and clear the handle's non-finite flag; the caller has synchronised the stream that set it.
static int poll_status(sknnr_index* ix) {
    int bits = 0;
    HIP_TRY(hipMemcpy(&bits, ix->status.p, sizeof bits, hipMemcpyDeviceToHost));
    if (!bits) return SKNNR_OK;
    HIP_TRY(hipMemset(ix->status.p, 0, 16));
    return nonfinite_error(bits);
}

extern "C" int sknnr_check_finite(sknnr_index* ix, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return poll_status(ix);
}

// ----------------------------------------------------------------------------------------
// launch helpers
// ----------------------------------------------------------------------------------------
namespace {

// What the dispatch rules read of an index: plain numbers (sknnr_debug_search_plan fills one without a handle).
struct IndexDesc { long n_ref; int d, ks, d_in, n_stages2, cell_depth; bool rescue_enabled, h16_ok; };
IndexDesc describe(const sknnr_index* ix) {
    return IndexDesc{ix->n_ref, ix->d, ix->ks, ix->d_in, ix->n_stages2, ix->cell_depth, ix->rescue_enabled, ix->h16_ok};
}

// Everything a search call decides before its first launch (plan_search, below): run_device works it out once and every
// stage reads it.
struct SearchPlan {
    int kk;                  // neighbours searched: n_neighbors, + 1 for the row itself when exclude_self is set
    bool affine, self_rows;  // the rows go through the affine map; no rows given: reference rows from row_offset on
    // rows narrower than float64 (opts->query_dtype): the prep kernel widens them and writes the float64 rows everything
    // after it reads (finaliser, exact scan), as it does for rows that go through the affine map
    int x_dtype;
    bool to_xt;
    int d_x;                 // columns of the caller's rows
    bool check_finite;
    bool coarse, v2;         // the Euclidean pre-filter runs; ... the second-generation kernel (use_coarse2)
    int m_list, rank_extra;  // list length per lane (coarse_list_len); thresholds of rank m_list + rank_extra
    bool record;             // the finaliser works from merged candidate records (use_record)
    bool rescue, bucketed;   // listed rows are swept again before the exact scan (rescue.hip.h); rows bucketed by cell
    bool ham_int;            // the integer pre-filter of the weighted-Hamming search runs (hamming.hip.h)
    long chunk, cap_pad;     // query rows per device chunk (chunk_rows); the largest chunk's rows with their padding
};

// The pre-filters skip a tile whose smallest possible value lies this far (times |q'|) above the threshold; the rescue
// sweep uses the same scale
float skip_scale(const sknnr_index* ix) { return (float)(std::ldexp(1.0, -9) * ix->ymax * 1.02); }

// p.bucketed: also name every row's cell (query bucketing); *cells_done tells whether this kernel did (the
// register-resident one does; otherwise the caller runs cell_assign_kernel on the transformed rows)
int launch_prep(sknnr_index* ix, const SearchPlan& p, const void* x, long nq, long nq_pad, double* xt, hipStream_t st,
                bool* cells_done = nullptr) {
    const bool affine = p.affine;
    PrepArgs a{};
    a.x_dtype = p.x_dtype;
    if (cells_done) *cells_done = false;
    a.status = p.check_finite ? ix->status.p : nullptr;
    a.x = x;
    a.nq = nq;
    a.nq_pad = nq_pad;
    a.d_in = affine ? ix->d_in : ix->d;
    a.d = ix->d;
    a.ks = ix->ks;
    a.center = (affine && ix->has_center) ? ix->center.p : nullptr;
    a.scale = (affine && ix->has_scale) ? ix->scale.p : nullptr;
    a.proj = (affine && ix->has_proj) ? ix->proj.p : nullptr;
    a.mu = ix->mu_dev.p;
    a.s = ix->s;
    a.xt = xt;
    a.qimg = ix->qimg.p;
    a.qnc = ix->qnc.p;
    int64_t* r = ix->last.prep;
    std::fill(r, r + 8, 0);
    ix->last.prep_xt = nullptr;
    ix->last.prep_bucketed = ix->last.prep_qnc_pos = false;
    r[2] = p.x_dtype, r[3] = nq, r[4] = nq_pad, r[5] = xt ? 1 : 0;
    r[7] = (a.center ? 1 : 0) | (a.scale ? 2 : 0) | (a.proj ? 4 : 0);
    if (ix->ks <= 4 && !std::getenv("SKNNR_PREP_LDS")) {
        // narrow feature spaces: register-resident kernel (no LDS, high occupancy)
        if (p.bucketed && ix->cell_depth > 0) {
            a.tree = CellTreeDev{ix->cell_axes.p, ix->cell_centre.p, ix->cell_thr.p, ix->cell_depth};
            a.cell = ix->qcell.p;
            if (cells_done) *cells_done = true;
            r[6] = 1;
        }
        HIP_TRY(launch::prep_direct(a, st));
        r[0] = 1, r[1] = 256;
    } else if (const int bt = prep_lds_rows(a.d_in)) {
        HIP_TRY(launch::prep_lds(bt, a, st));
        r[0] = 2, r[1] = bt;
    } else {
        std::fill(r, r + 8, 0);
        return fail(SKNNR_ERR_UNSUPPORTED, "d_in = %d is too wide for the query preparation kernel (max 299)", a.d_in);
    }
    ix->last.prep_xt = xt;
    return SKNNR_OK;
}

// first-generation pre-filter (k_coarse1.hip)
int launch_coarse(sknnr_index* ix, const SearchPlan& p, long nq_pad, hipStream_t st) {
    const int m_list = p.m_list;
    launch::Coarse1Launch L{ix->rimg.p, ix->n_stages, ix->qimg.p, ix->qnc.p, skip_scale(ix),
                            m_list - (p.kk + 1), ix->cand_val.p, ix->cand_idx.p, nq_pad};
    hipError_t e = hipSuccess;
    if (launch::coarse1(ix->ks, m_list, L, st, &e) == launch::kNoInstance)
        return fail(SKNNR_ERR_UNSUPPORTED, "no coarse kernel for ks = %d, list length %d", ix->ks, m_list);
    HIP_TRY(e);
    int64_t* r = ix->last.prefilter;
    r[0] = 1, r[1] = ix->ks, r[2] = m_list, r[3] = 0, r[4] = coarse_waves(ix->ks, m_list), r[5] = nq_pad;
    return SKNNR_OK;
}

constexpr int kCoarse2TailWaves = 4;  // workgroup size (waves) of the thin-round variant
constexpr int kCusPerDevice = 256;

// The finaliser works from merged candidate records (coarse2.hip.h, Coarse2Record; finalize_record_kernel) where the
// second-generation kernel has an instance that files them (coarse2_record_supported: lists of 2 and 6 with sentinels, up to
// two K-steps -- up to 5 neighbours searched on up to 32 features).
// SKNNR_FINALIZE_RECORD=0 keeps the lists and finalize_kernel<8> (A/B runs).
bool use_record(int ks, int m_list, int kk, bool v2, int raw) {
    static const bool enabled = env_on("SKNNR_FINALIZE_RECORD");
    return enabled && v2 && !raw && coarse2_record_supported(ks, m_list, coarse2_rank_extra(m_list, kk));
}

int launch_coarse2_waves(sknnr_index* ix, const SearchPlan& p, int waves, long row0, long rows, hipStream_t st) {
    // more neighbours than a list holds: thresholds of rank M + E, no sentinels (coarse2_rank_extra)
    const int m_list = p.m_list, kk = p.kk, extra = p.rank_extra;
    if (extra != 0 && !((m_list == 16 && kk <= kCoarse2MaxKK16) || (m_list == 12 && kk <= kCoarse2MaxKK12) || (m_list == 8 && kk <= kCoarse2MaxKK8) || (m_list == 6 && kk <= kCoarse2MaxKK6)))
        return fail(SKNNR_ERR_UNSUPPORTED, "lists of %d cannot serve %d neighbours", m_list, kk);
    // positions [row0, row0 + rows) of the chunk (bucketed calls: position -> row through qperm, else the row itself)
    const bool bucketed = p.bucketed;
    launch::Coarse2Launch L{ix->rhi2.p, ix->rlo2.p, ix->n_stages2, ix->qimg.p, ix->qnc.p, skip_scale(ix),
                            extra != 0 ? 0 : m_list - (kk + 1), ix->cand_val.p, ix->cand_idx.p, (int)row0,
                            bucketed ? ix->qperm.p : nullptr, bucketed ? ix->qcell.p : nullptr,
                            bucketed ? ix->cell_stage.p : nullptr, rows,
                            Coarse2Record{p.record ? ix->rec.p : nullptr, ix->rec_bound.p, ix->perm2.p, (int)ix->n_ref}};
    hipError_t e = hipSuccess;
    if (launch::coarse2(ix->ks, m_list, waves, extra, L, st, &e) == launch::kNoInstance)
        return fail(SKNNR_ERR_UNSUPPORTED, "no second-generation coarse kernel for ks = %d, list length %d, %d waves, rank + %d", ix->ks,
                    m_list, waves, extra);
    HIP_TRY(e);
    int64_t* r = ix->last.prefilter;
    r[0] = 2, r[1] = ix->ks, r[2] = m_list, r[3] = extra;
    if (waves == kCoarse2TailWaves) {
        r[6] += rows;
    } else {
        r[4] = waves;
        r[5] += rows;
    }
    return SKNNR_OK;
}

// A workgroup of 16 waves sweeps the whole image for its 1024 rows (~1.2 ms at 50k reference rows), so the
// last round of a launch leaves most CUs idle when it holds few workgroups (10M rows: 9768 workgroups =
// 38 rounds + 40), and a small call never fills the device.  Rows of such a thin round (at most a quarter of
// the CUs' worth) go to 4-wave workgroups instead: four times as many CUs, one wave per SIMD.
// `rows`: the live rows of the chunk -- its padding rows (up to kRowQuantum - 1 of them, behind the live ones also in a
// bucketed call) get no workgroups of their own: a 262,144-row call is 256 workgroups, not 258 with a thin round of two.
// With a thin round and a side stream, the bulk launch is followed by `ev_bulk_end` (the timed region ends there: the
// thin round shares the device from then on) and by the fork event; *fork tells the caller, who finalises the bulk rows
// beside the thin round: the rows whose pre-filter was complete at ev_fork (0: no fork), whether ev_bulk_end was recorded.
struct BulkFork { long rows_done = 0; bool recorded = false; };
int launch_coarse2(sknnr_index* ix, const SearchPlan& p, long rows, hipEvent_t ev_bulk_end, BulkFork* fork, hipStream_t st) {
    const int m_list = p.m_list;
    if (!coarse2_supported(ix->ks, m_list))
        return fail(SKNNR_ERR_UNSUPPORTED, "no second-generation coarse kernel for ks = %d, list length %d", ix->ks, m_list);
    const int BULK_WAVES = coarse2_waves(ix->ks, m_list);
    const long QPB = BULK_WAVES * kCoarse2Nqb * 32;
    const long QPB_TAIL = kCoarse2TailWaves * kCoarse2Nqb * 32;
    static const bool split = env_on("SKNNR_COARSE_TAIL");
    const long n_wg = (rows + QPB - 1) / QPB;
    long tail_wg = n_wg % kCusPerDevice;
    if (!split || tail_wg > kCusPerDevice / (BULK_WAVES / kCoarse2TailWaves)) tail_wg = 0;
    const long bulk_rows = (n_wg - tail_wg) * QPB;
    *fork = BulkFork{};
    if (bulk_rows > 0) {
        int rc = launch_coarse2_waves(ix, p, BULK_WAVES, 0, bulk_rows, st);
        if (rc) return rc;
        if (tail_wg > 0 && ix->ev_fork) {  // the caller finalises these rows beside the thin round
            HIP_TRY(hipEventRecord(ev_bulk_end, st));
            fork->recorded = true;
            HIP_TRY(hipEventRecord(ix->ev_fork, st));
            fork->rows_done = bulk_rows;
        }
    }
    if (tail_wg > 0) {
        const long tail_rows = std::min(tail_wg * QPB, (rows - bulk_rows + QPB_TAIL - 1) / QPB_TAIL * QPB_TAIL);
        return launch_coarse2_waves(ix, p, kCoarse2TailWaves, bulk_rows, tail_rows, st);
    }
    return SKNNR_OK;
}

// The second-generation kernel serves the shapes of coarse2_supported() (SKNNR_COARSE_V2=0 selects the first one).
bool use_coarse2(const IndexDesc& ix, int m_list) {
    static const bool enabled = env_on("SKNNR_COARSE_V2");
    // (small reference sets keep the first kernel: the second one needs its seeding pass -- without a starting
    // threshold the first tiles give every lane more hits per unit than its queue holds)
    // (and the flush addresses the image with 32-bit offsets)
    const long tiles2 = (long)ix.n_stages2 * tiles_per_stage2(ix.ks);
    // (... and its flush tags a queued entry's image position, below 2^26, with the query column)
    return enabled && tiles2 >= 2 * kSeedTiles && tiles2 * tile2_bytes(ix.ks) < (1L << 32) && tiles2 * 32 < (1L << 26) &&
           coarse2_supported(ix.ks, m_list);
}

// List length per lane for kk neighbours searched: at least one spare slot keeps the certificate
// cheap.  kk > 31 is outside the MFMA envelope (exact scan for the whole call).
constexpr int kCoarseMaxKK = 31;
int coarse_list_len(int kk) { return kk <= 1 ? 2 : (kk <= 5 ? 6 : (kk <= 7 ? 8 : (kk <= 15 ? 16 : 32))); }
// ... for this handle: where the second-generation kernel serves them, 6 .. 7 neighbours keep lists of 6, 8 .. 15 lists of
// 8, 16 .. 23 lists of 12 and 24 .. 31 lists of 16 (up to 64 features), with thresholds of a rank beyond one list over the two lists of a query kept as one pool
// (coarse2.hip.h, pair_union_rank, coarse2_rank_extra) -- shorter lists are cheaper to keep, lists of 8 run with 16 waves
// per CU and no spills where lists of 16 need 12 waves, and lists of 32 exist on the first-generation kernel only.
int coarse_list_len(const IndexDesc& ix, int kk) {
    static const int enabled = [] {
        const char* e = std::getenv("SKNNR_V2_BIG_K");  // 0: off, 1: lists of 16 only, 2: and lists of 8, 3: and 6 .. 7 on lists of 6, default: all
        return e ? std::atoi(e) : 4;
    }();
    // (6 .. 7 neighbours: lists of 8 hold them where that kernel exists -- measured equal, 169 vs 169 Mq/s at 10M x 50k x 32,
    //  k = 7 -- and lists of 6 serve four K-steps, where lists of 8 would spill: 84 -> 95 Mq/s at 64 features)
    if (enabled >= 3 && kk > 5 && kk <= kCoarse2MaxKK6 && !use_coarse2(ix, 8) && use_coarse2(ix, 6)) return 6;
    if (enabled >= 2 && kk > 7 && kk <= kCoarse2MaxKK8 && use_coarse2(ix, 8)) return 8;
    if (enabled >= 4 && kk > 15 && kk <= kCoarse2MaxKK12 && use_coarse2(ix, 12)) return 12;
    if (enabled >= 1 && kk > 15 && kk <= kCoarse2MaxKK16 && use_coarse2(ix, 16)) return 16;
    return coarse_list_len(kk);
}

// The plan of a call of nq rows (rows_given: the caller's, else reference rows) with these opts; raw: shard candidates.
// A pure function of its arguments and of the process-static switches.
SearchPlan plan_search(const IndexDesc& ix, const sknnr_query_opts* o, long nq, bool rows_given, int raw) {
    static const bool scan_everything = std::getenv("SKNNR_EXACT_ONLY") != nullptr;  // development: time the float64 scan alone
    SearchPlan p{};
    p.kk = o->n_neighbors + (o->exclude_self ? 1 : 0);
    p.affine = o->apply_affine != 0 && rows_given;
    p.self_rows = !rows_given;
    p.x_dtype = p.self_rows ? kDtypeF64 : o->query_dtype;
    p.to_xt = p.affine || p.x_dtype != kDtypeF64;
    p.d_x = p.affine ? ix.d_in : ix.d;
    p.check_finite = o->check_finite != 0 && rows_given;
    p.coarse = ix.ks > 0 && p.kk <= kCoarseMaxKK && o->formula != SKNNR_FORMULA_HAMMING && !scan_everything;
    p.m_list = coarse_list_len(ix, p.kk);
    p.v2 = p.coarse && use_coarse2(ix, p.m_list);
    p.rank_extra = coarse2_rank_extra(p.m_list, p.kk);
    p.record = p.coarse && use_record(ix.ks, p.m_list, p.kk, p.v2, raw);
    // Rows the finalisers list are first swept again under their rescue thresholds (rescue.hip.h), behind the
    // second-generation pre-filter (its hi image and query image are what the sweep reads) and up to kRescueMaxKK neighbours
    // searched (the finish has 16 lanes per row); the exact scan then sees the second list only.
    p.rescue = p.v2 && ix.rescue_enabled && !raw && p.kk <= kRescueMaxKK;
    p.bucketed = p.v2 && ix.cell_depth > 0;
    // Weighted Hamming on 16-bit ids: integer pre-filter, float64 re-score of the candidates (hamming.hip.h)
    p.ham_int = !p.coarse && o->formula == SKNNR_FORMULA_HAMMING && ix.h16_ok && p.kk <= kHamMaxKK;
    p.chunk = chunk_rows(ix.ks, p.m_list);
    p.cap_pad = pad_rows(std::min(p.chunk, nq));
    return p;
}

constexpr int kScanGridWg = 256 * 4;  // workgroups of a scan launch (also what scan_slices splits among the passes)
// shared bytes of scan_merge_kernel for kk neighbours searched
size_t scan_merge_bytes(int kk) {
    const int kkp = (kk + 2) & ~1, stk = (2 * kk + 4 + 1) & ~1;
    return 4 * ((size_t)12 * kkp + (size_t)4 * stk);
}

int launch_scan_formula(sknnr_index* ix, const ScanArgs& a0, long max_items, bool chunked, size_t sh, hipStream_t st) {
    const SelectArgs& s = a0.s;
    const int nq_pass = scan_nq(s.formula);
    ScanArgs a = a0;
    // Few queries: their passes would leave most of the device idle while each sweeps every reference row
    // (0.5 ms at 50k rows whatever the count) -- the kernel then splits the rows of a pass over several
    // workgroups and scan_merge_kernel combines the slice heaps.  The count is on the device when the queries
    // come from the fail list, so the decision is taken there; the host only provides the buffers.
    const bool may_slice = s.kk <= kScanSliceMaxKK && scan_slices(1, nq_pass, s.n_ref, s.kk, kScanGridWg) > 1;
    if (may_slice) {
        // at most kScanGridWg / 2 passes are sliced: (passes * nq_pass) slots x S slices <= kScanGridWg * nq_pass heaps
        const size_t heaps = (size_t)kScanGridWg * nq_pass * s.kk;
        HIP_TRY(ix->slice_v.ensure(heaps));
        HIP_TRY(ix->slice_i.ensure(heaps));
        HIP_TRY(ix->fail_list2.ensure((size_t)kScanGridWg * nq_pass));
        HIP_TRY(hipMemsetAsync(ix->fail_count.p + 2, 0, sizeof(int), st));
        a.slice_v = ix->slice_v.p;
        a.slice_i = ix->slice_i.p;
        a.list2 = ix->fail_list2.p;
        a.count2 = ix->fail_count.p + 2;
    }
    const long passes = (max_items + nq_pass - 1) / nq_pass;
    // (sliced mode needs the whole grid even for one pass; otherwise one workgroup per pass is enough)
    const long blocks = may_slice ? kScanGridWg : std::max<long>(1, std::min<long>(passes, kScanGridWg));
    const int64_t rec[8] = {s.formula + 1, chunked ? 1 : 0, s.kk, blocks, (int64_t)sh, a0.list ? -1 : max_items, may_slice ? 0 : 1,
                            may_slice ? 1 : 0};
    std::copy(std::begin(rec), std::end(rec), ix->last.scan);
    HIP_TRY(launch::exact_scan(s.formula, chunked, a, blocks, sh, st));
    if (!may_slice) return SKNNR_OK;
    // one wave per sliced query (none if the scan was not sliced: the kernel returns at once)
    const long sliced_max = std::min<long>(max_items, (long)kScanGridWg * nq_pass / 2);
    HIP_TRY(launch::scan_merge(s.formula, a, (sliced_max + 3) / 4, scan_merge_bytes(s.kk), (int)blocks, 0, st));
    // queries whose merged heaps are not unique (exact ties): the sequential scan, never sliced
    ScanArgs b = a0;
    b.list = ix->fail_list2.p;
    b.count = ix->fail_count.p + 2;
    b.slice_v = nullptr;
    b.slice_i = nullptr;
    const long blocks2 = std::max<long>(1, std::min<long>((sliced_max + nq_pass - 1) / nq_pass, kScanGridWg));
    HIP_TRY(launch::exact_scan(s.formula, chunked, b, blocks2, sh, st));
    return SKNNR_OK;
}

int launch_scan(sknnr_index* ix, const SelectArgs& s, const int* list, const int* count, long max_items,
                hipStream_t st) {
    const size_t sh = scan_block_bytes(s.d, s.kk, s.formula);
    if (sh > kLdsLimit)
        return fail(SKNNR_ERR_UNSUPPORTED, "n_neighbors = %d with d = %d does not fit the exact scan kernel", s.k, s.d);
    ScanArgs a{s, ix->refT.p, list, count, nullptr, nullptr, nullptr, nullptr};
    const bool chunked = s.d > kScanColChunk;  // wide rows (tree node ids) are swept in column chunks
    return launch_scan_formula(ix, a, max_items, chunked, sh, st);
}

// Does a call with these opts map its rows through the handle's forests (apply_affine on a Hamming call)?
bool uses_forest(const sknnr_index* ix, const sknnr_query_opts* o) {
    return o->apply_affine && o->formula == SKNNR_FORMULA_HAMMING && ix->has_forest;
}
// Columns of the caller's query rows: d_in of the query-time map in use (affine or forest), else d.
int query_cols(const sknnr_index* ix, const sknnr_query_opts* o) {
    if (!o->apply_affine) return ix->d;
    return uses_forest(ix, o) ? ix->f_d_in : ix->d_in;
}

int validate_call(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o, int64_t* out_idx) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("a search call");
    if (!o) return fail(SKNNR_ERR_INVALID, "opts is NULL");
    if (o->query_dtype < 0 || o->query_dtype >= kDtypeCount) return fail(SKNNR_ERR_INVALID, "unknown query_dtype %d", o->query_dtype);
    const bool forest_map = uses_forest(ix, o);  // (the forest kernel reads every sknnr_dtype)
    if (o->query_dtype != SKNNR_DTYPE_F64 && q && !forest_map) {
        // narrow rows are widened by the query preparation kernel, which exists inside the MFMA envelope only
        if (ix->ks == 0) return fail(SKNNR_ERR_UNSUPPORTED, "query_dtype %d needs d <= 128 (d = %d): pass float64 rows", o->query_dtype, ix->d);
        if (o->formula == SKNNR_FORMULA_HAMMING) return fail(SKNNR_ERR_UNSUPPORTED, "node ids are float64: query_dtype must be 0 with formula = HAMMING");
    }
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (!out_idx && nq > 0) return fail(SKNNR_ERR_INVALID, "out_idx is NULL");
    if (o->n_neighbors <= 0) return fail(SKNNR_ERR_INVALID, "Expected n_neighbors > 0. Got %d", o->n_neighbors);
    if (!q && !o->exclude_self) return fail(SKNNR_ERR_INVALID, "q is NULL but exclude_self is not set");
    const long n_fit = ix->n_ref;
    if (o->exclude_self) {
        if (o->n_neighbors + 1 > n_fit)
            return fail(SKNNR_ERR_K_TOO_LARGE,
                        "Expected n_neighbors < n_samples_fit, but n_neighbors = %d, n_samples_fit = %ld, n_samples = %ld",
                        o->n_neighbors, n_fit, (long)nq);
        if (!q && (o->row_offset < 0 || o->row_offset + nq > n_fit))
            return fail(SKNNR_ERR_INVALID, "self query rows [%ld, %ld) outside the %ld reference rows",
                        (long)o->row_offset, (long)(o->row_offset + nq), n_fit);
    } else if (o->n_neighbors > n_fit) {
        return fail(SKNNR_ERR_K_TOO_LARGE,
                    "Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %ld, n_samples = %ld",
                    o->n_neighbors, n_fit, (long)nq);
    }
    if (o->apply_affine && !ix->has_affine && !forest_map)
        return fail(SKNNR_ERR_INVALID, "apply_affine is set but no affine map was installed");
    if (o->formula != SKNNR_FORMULA_EXPANDED && o->formula != SKNNR_FORMULA_DIRECT && o->formula != SKNNR_FORMULA_HAMMING)
        return fail(SKNNR_ERR_INVALID, "unknown formula %d", o->formula);
    if (o->formula == SKNNR_FORMULA_HAMMING) {
        if (!ix->has_hw) return fail(SKNNR_ERR_INVALID, "formula = HAMMING needs sknnr_index_set_hamming_weights first");
        if (o->apply_affine && !forest_map) return fail(SKNNR_ERR_INVALID, "node ids are not mapped by an affine transform");
    }
    if (o->n_neighbors + (o->exclude_self ? 1 : 0) > kScanMaxKK)
        return fail(SKNNR_ERR_UNSUPPORTED, "n_neighbors = %d exceeds the HIP backend's limit of %d%s", o->n_neighbors,
                    kScanMaxKK - (o->exclude_self ? 1 : 0),
                    o->exclude_self ? " with X=None (the query rows' own rows are searched too)" : "");
    if (std::abs(o->decimals) > 300) return fail(SKNNR_ERR_INVALID, "decimals out of range");
    return SKNNR_OK;
}

int run_forest(sknnr_index* ix, const void* xdev, long nq, const sknnr_query_opts* o, double* d_dist, long* d_idx,
               hipStream_t st);
// every search call zeroes the debug records first
void zero_records(sknnr_index* ix) { ix->last = SearchRecords{}; }

// ---- the stages of run_device, in the order it runs them -----------------------------------------------------------------
// Workspace of a call: the transformed rows of the WHOLE call (the exact scan at the end reads any row of it), the
// per-chunk buffers at the largest chunk's padded rows, the lists; the device counters of the call start at zero.
int ensure_workspace(sknnr_index* ix, const SearchPlan& p, long nq, hipStream_t st) {
    if (p.to_xt) HIP_TRY(ix->xt.ensure((size_t)nq * ix->d));
    const long cap_pad = p.cap_pad;  // the per-chunk buffers hold the largest chunk with its padding
    if (p.coarse || p.to_xt) {
        HIP_TRY(ix->qimg.ensure((size_t)(cap_pad / 32) * 2 * ix->ks * 64));
        HIP_TRY(ix->qnc.ensure(cap_pad));
    }
    if (p.coarse && ix->cell_depth > 0) {
        HIP_TRY(ix->qcell.ensure((size_t)cap_pad));
        HIP_TRY(ix->qperm.ensure((size_t)cap_pad));
    }
    if (p.record) {
        HIP_TRY(ix->rec.ensure((size_t)cap_pad * kRecordLen));
        HIP_TRY(ix->rec_bound.ensure((size_t)cap_pad));
        if (ix->cell_depth > 0) HIP_TRY(ix->qnc_pos.ensure((size_t)cap_pad));
    } else if (p.coarse) {
        HIP_TRY(ix->cand_val.ensure((size_t)cap_pad * 2 * p.m_list));
        HIP_TRY(ix->cand_idx.ensure((size_t)cap_pad * 2 * p.m_list));
    }
    if (p.coarse) {
        HIP_TRY(ix->fail_list.ensure(nq));
        HIP_TRY(hipMemsetAsync(ix->fail_count.p, 0, 16, st));
    }
    if (p.rescue) {
        HIP_TRY(ix->fail_thr.ensure(nq));
        HIP_TRY(ix->resc_list.ensure(nq));
        HIP_TRY(hipMemsetAsync(ix->resc_state.p, 0, kRescueWords * sizeof(int), st));
        ix->last.rescue[0] = 1;
        ix->last.rescue[1] = ix->ks;
    }
    return SKNNR_OK;
}

// What the finaliser, the re-score and the exact scan select by, for the nq rows at xq (a whole call; a chunk narrows it
// to its window).  raw / id_offset: shard candidates.
SelectArgs make_select_args(const sknnr_index* ix, const sknnr_query_opts* o, int kk, const double* xq, long nq, double* d_dist,
                            long* d_idx, int raw = 0, long id_offset = 0) {
    SelectArgs call{};
    call.xq = xq;
    call.ref = ix->ref64.p;
    call.rn = ix->rn64.p;
    call.nq = nq;
    call.d = ix->d;
    call.n_ref = (int)ix->n_ref;
    call.k = o->n_neighbors;
    call.kk = kk;
    call.exclude_self = o->exclude_self ? 1 : 0;
    call.deterministic = o->deterministic && !raw ? 1 : 0;
    call.formula = o->formula;
    call.pow10_is_divisor = o->decimals < 0;
    call.pow10 = std::pow(10.0, std::abs(o->decimals));
    call.row_offset = o->row_offset;
    call.hw = ix->hw.p;
    call.hw_sum = ix->hw_sum;
    call.raw = raw;
    call.id_offset = id_offset;
    call.out_dist = d_dist;
    call.out_idx = d_idx;
    return call;
}
// ... narrowed to rows [r0, r0 + n) of those rows: their query rows, outputs and row numbers
SelectArgs select_window(const SelectArgs& s, long r0, long n) {
    SelectArgs w = s;
    w.xq = s.xq + r0 * s.d;
    w.nq = n;
    w.row_offset = s.row_offset + r0;
    w.out_dist = s.out_dist ? s.out_dist + r0 * s.k : nullptr;
    w.out_idx = s.out_idx + r0 * s.k;
    return w;
}

// query preparation of rows [c0, c0 + n) of the call
int prep_chunk(sknnr_index* ix, const SearchPlan& p, const SelectArgs& call, const void* xdev, long c0, long n, hipStream_t st,
               bool* cells_done = nullptr) {
    const void* xin = p.self_rows ? (const void*)(call.xq + c0 * ix->d)
                                  : (const void*)((const char*)xdev + (size_t)c0 * p.d_x * dtype_bytes(p.x_dtype));
    return launch_prep(ix, p, xin, n, pad_rows(n), p.to_xt ? ix->xt.p + c0 * ix->d : nullptr, st, cells_done);
}

// cell of every row of the chunk at xq, rows bucketed by cell: position -> row (bucket.hip.h)
int bucket_chunk(sknnr_index* ix, const SearchPlan& p, const double* xq, long n, bool cells_done, hipStream_t st) {
    CellArgs ca{};
    ca.xq = xq;
    ca.nq = n;
    ca.n_pad = pad_rows(n);
    ca.d = ix->d;
    ca.depth = ix->cell_depth;
    ca.axes = ix->cell_axes.p;
    ca.centre = ix->cell_centre.p;
    ca.thr = ix->cell_thr.p;
    ca.cell = ix->qcell.p;
    ca.hist = ix->cell_hist.p;
    ca.perm = ix->qperm.p;
    ca.qnc = ix->qnc.p;
    ca.qnc_pos = p.record ? ix->qnc_pos.p : nullptr;
    HIP_TRY(hipMemsetAsync(ix->cell_hist.p, 0, 2 * kCellMax * sizeof(int), st));
    if (!cells_done) HIP_TRY(launch::cell_assign(ca, st));
    HIP_TRY(launch::cell_count(ca, st));
    HIP_TRY(launch::cell_scatter(ca, st));
    if (!cells_done) ix->last.prep[6] = 2;
    ix->last.prep_bucketed = true;
    ix->last.prep_qnc_pos = p.record;
    return SKNNR_OK;
}

// the finaliser's arguments for rows [c0, c0 + n) of the call, whose candidates the workspace holds
FinalizeArgs finalize_args(const sknnr_index* ix, const SearchPlan& p, const SelectArgs& call, long c0, long n) {
    FinalizeArgs f{};
    f.s = select_window(call, c0, n);
    f.cand_val = ix->cand_val.p;
    f.cand_idx = ix->cand_idx.p;
    f.perm = p.v2 ? ix->perm2.p : ix->perm.p;
    f.qnc = ix->qnc.p;
    f.qperm = p.bucketed ? ix->qperm.p : nullptr;
    if (p.record) {
        f.rec = ix->rec.p;
        f.rec_bound = ix->rec_bound.p;
        f.qnc_pos = p.bucketed ? ix->qnc_pos.p : ix->qnc.p;
        f.trunc_count = ix->fail_count.p + 3;
    }
    f.m_list = p.m_list;
    f.rank_extra = p.rank_extra;
    f.inv_s2 = 1.0 / (ix->s * ix->s);
    f.s2 = ix->s * ix->s;
    f.inv_s = 1.0 / ix->s;
    f.eps_c = (p.v2 ? eps_units2(ix->ks) : eps_units(ix->ks)) * std::ldexp(1.0, -24);
    f.ymax = ix->ymax;
    f.noise_a = (ix->d + 4) * std::ldexp(1.0, -53);
    f.mu2 = call.formula == SKNNR_FORMULA_EXPANDED ? 2.0 * ix->mu_norm : 0.0;
    f.fail_list = ix->fail_list.p;
    f.fail_count = ix->fail_count.p;
    f.fail_thr = p.rescue ? ix->fail_thr.p : nullptr;
    f.fail_base = (int)c0;
    return f;
}

// Finalise rows [r0, r0 + rows) of the chunk f describes (the kernel indexes everything by the row inside its window);
// bucketed calls: POSITIONS [r0, r0 + rows) of the chunk, the kernel maps them to rows of the chunk
hipError_t finalize_rows(const FinalizeArgs& f, const SearchPlan& p, long r0, long rows, hipStream_t st) {
    FinalizeArgs g = f;
    if (p.bucketed) {
        g.pos0 = r0;
        g.s.nq = rows;
        return launch::finalize(g, rows, st);
    }
    g.s = select_window(f.s, r0, rows);
    if (p.record) {
        g.rec = f.rec + (size_t)r0 * kRecordLen;
        g.rec_bound = f.rec_bound + r0;
        g.qnc_pos = f.qnc_pos + r0;
    } else {
        g.cand_val = f.cand_val + (size_t)r0 * 2 * f.m_list;
        g.cand_idx = f.cand_idx + (size_t)r0 * 2 * f.m_list;
    }
    g.qnc = f.qnc + r0;
    g.fail_base = f.fail_base + (int)r0;
    return launch::finalize(g, rows, st);
}

// the rescue sweep of the rows the finaliser of chunk f (rows from c0 of the call) has listed
RescueArgs rescue_args(const sknnr_index* ix, const FinalizeArgs& f, const SelectArgs& call, long c0) {
    RescueArgs ra{};
    ra.f = f;
    ra.f.s = call;  // finalize_core works on call-relative rows here, as the list names them
    ra.f.fail_list = ix->resc_list.p;
    ra.f.fail_count = ix->resc_state.p + kRescueHanded;
    ra.f.fail_thr = nullptr;
    ra.f.fail_base = 0;
    ra.f.rec = nullptr;
    ra.f.qperm = nullptr;
    ra.rhi = ix->rhi2.p;
    ra.n_tiles = ix->n_stages2 * tiles_per_stage2(ix->ks);
    ra.perm = ix->perm2.p;
    ra.qimg = ix->qimg.p;
    ra.qnc = ix->qnc.p;
    ra.row0 = (int)c0;
    ra.skip_scale = skip_scale(ix);
    ra.list = ix->fail_list.p;
    ra.thr = ix->fail_thr.p;
    ra.count = ix->fail_count.p;
    ra.state = ix->resc_state.p;
    return ra;
}

// One chunk of the Euclidean path, rows [c0, c0 + n) of the call: prep, bucketing, the timed pre-filter, the finaliser
// (beside the pre-filter's thin round where there is one), the rescue sweep.
int coarse_chunk(sknnr_index* ix, const SearchPlan& p, const SelectArgs& call, const void* xdev, long c0, long n,
                 sknnr_index::CallTiming& ct, hipStream_t st) {
    bool cells_done = false;
    int rc = prep_chunk(ix, p, call, xdev, c0, n, st, &cells_done);
    if (rc) return rc;
    if (ct.coarse_used == ct.coarse.size()) {
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        ct.coarse.emplace_back(e0, e1);
    }
    auto& ev = ct.coarse[ct.coarse_used++];
    if (p.bucketed && (rc = bucket_chunk(ix, p, call.xq + c0 * ix->d, n, cells_done, st))) return rc;
    HIP_TRY(hipEventRecord(ev.first, st));
    if (p.v2 && !ix->st_side && !std::getenv("SKNNR_NO_SIDE_STREAM")) {
        HIP_TRY(hipStreamCreateWithFlags(&ix->st_side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ix->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ix->ev_join, hipEventDisableTiming));
    }
    std::fill(std::begin(ix->last.prefilter), std::end(ix->last.prefilter), 0);  // (this chunk's launches only)
    ix->last.prefilter[7] = p.bucketed ? ix->cell_depth : 0;
    {
        // matrix work issued / algorithmic (rows of the launch cancel): K-steps x tiles swept over d x n_ref
        const long tiles2 = (long)ix->n_stages2 * tiles_per_stage2(ix->ks);
        const long tiles = p.v2 ? tiles2 + seed_tiles_for(tiles2, tiles_per_stage2(ix->ks)) : (long)ix->n_stages * tiles_per_stage(ix->ks);
        ix->stats.mfma_executed_ratio = (double)tiles * 32.0 * (16.0 * ix->ks) / ((double)ix->n_ref * ix->d);
    }
    BulkFork fork;
    rc = p.v2 ? launch_coarse2(ix, p, n, ev.second, &fork, st) : launch_coarse(ix, p, pad_rows(n), st);
    if (rc) return rc;
    if (!fork.recorded) HIP_TRY(hipEventRecord(ev.second, st));  // (no fork: the whole pre-filter is timed)
    const long done = std::min<long>(fork.rows_done, n);
    ct.coarse_rows += done > 0 ? done : n;

    const FinalizeArgs f = finalize_args(ix, p, call, c0, n);
    ix->last.finalize[0] = launch::finalize_lanes(f);
    ix->last.finalize[1] = p.record ? 1 : 0;
    if (done > 0) {
        // fork: the rows of the bulk launch are finalised on the side stream while the thin round runs here
        HIP_TRY(hipStreamWaitEvent(ix->st_side, ix->ev_fork, 0));
        HIP_TRY(finalize_rows(f, p, 0, done, ix->st_side));
        HIP_TRY(hipEventRecord(ix->ev_join, ix->st_side));
        if (n > done) HIP_TRY(finalize_rows(f, p, done, n - done, st));
        HIP_TRY(hipStreamWaitEvent(st, ix->ev_join, 0));  // join before anything else touches the workspace
    } else {
        HIP_TRY(finalize_rows(f, p, 0, n, st));
    }
    // the rows listed for this chunk, while its query image is in the workspace: one fixed-size launch that reads the
    // count on the device
    if (p.rescue) HIP_TRY(launch::rescue(ix->ks, rescue_args(ix, f, call, c0), st));
    return SKNNR_OK;
}

// Weighted Hamming on 16-bit ids: integer pre-filter, float64 re-score of the candidates (hamming.hip.h); the queries
// it cannot serve (too many candidates, ids outside 16 bits) join the fail list of the exact scan
int hamming_pass(sknnr_index* ix, const SearchPlan& p, const SelectArgs& call, long nq, hipStream_t st) {
    const long chunk_q = 1L << 18;  // 768 candidate bytes per query: 200 MB per chunk
    const long cap_q = std::min(chunk_q, nq);
    const long cap_pad = (cap_q + 255) / 256 * 256;
    HIP_TRY(ix->h_qimg.ensure((size_t)ix->h_tp * cap_pad));
    HIP_TRY(ix->h_bad.ensure((size_t)cap_pad));
    HIP_TRY(ix->h_cand_cnt.ensure((size_t)cap_q));
    HIP_TRY(ix->h_cand_id.ensure((size_t)cap_q * kHamCand));
    HIP_TRY(ix->fail_list.ensure(nq));
    HIP_TRY(hipMemsetAsync(ix->fail_count.p, 0, 16, st));
    const int64_t rec[7] = {1, p.kk, ham_compacts(p.kk) ? 1 : 0, ham_seed_rows((int)ix->n_ref, p.kk), (int64_t)ix->d + 2,
                            ix->h_tp, (nq + chunk_q - 1) / chunk_q};
    std::copy(std::begin(rec), std::end(rec), ix->last.hamming);
    for (long c0 = 0; c0 < nq; c0 += chunk_q) {
        const long n = std::min(chunk_q, nq - c0);
        ix->last.hamming_rows = n;
        const long n_pad = (n + 255) / 256 * 256;
        HIP_TRY(launch::hamming_pack(call.xq + c0 * ix->d, n, n_pad, ix->d, ix->h_tp, ix->h_qimg.p, ix->h_bad.p, st));
        HammingArgs ha{};
        ha.rimg = ix->h_rimg.p;
        ha.wq = ix->h_wq.p;
        ha.qimg = ix->h_qimg.p;
        ha.q_bad = ix->h_bad.p;
        ha.n_ref = (int)ix->n_ref;
        ha.n_ref_pad = ix->h_ref_pad;
        ha.tp = ix->h_tp;
        ha.nq = n;
        ha.nq_pad = n_pad;
        ha.kk = p.kk;
        ha.band = (unsigned)ix->d + 2u;
        ha.cand_cnt = ix->h_cand_cnt.p;
        ha.cand_id = ix->h_cand_id.p;
        HIP_TRY(launch::hamming_coarse(ha, st));
        HammingRescoreArgs hr{};
        hr.s = select_window(call, c0, n);
        hr.cand_cnt = ix->h_cand_cnt.p;
        hr.cand_id = ix->h_cand_id.p;
        hr.fail_list = ix->fail_list.p;
        hr.fail_count = ix->fail_count.p;
        hr.fail_base = (int)c0;
        hr.rrow = ix->h_rrow.p;
        hr.tpr = ham_row_dwords(ix->d);
        HIP_TRY(launch::hamming_rescore(hr, st));
    }
    return SKNNR_OK;
}

// One exact scan per call: the rows the finaliser could not certify (call-relative ids), or every row when the call is
// outside the MFMA envelope.  Then the running totals, and the events that close the call.
int scan_tail(sknnr_index* ix, const SearchPlan& p, const SelectArgs& call, long nq, sknnr_index::CallTiming& ct, hipStream_t st) {
    int rc = p.rescue ? launch_scan(ix, call, ix->resc_list.p, ix->resc_state.p + kRescueHanded, nq, st)
             : (p.coarse || p.ham_int) ? launch_scan(ix, call, ix->fail_list.p, ix->fail_count.p, nq, st)
                                       : launch_scan(ix, call, nullptr, nullptr, nq, st);
    if (rc) return rc;
    if (p.coarse) {
        // keep a running total on the device; sknnr_get_stats reads it (no sync here)
        if (p.rescue) HIP_TRY(launch::rescue_account(ix->fail_count.p, ix->resc_state.p, ix->fail_total.p, st));
        else HIP_TRY(launch::add_counter(ix->fail_count.p, ix->fail_total.p, st));
        ix->stats.coarse_queries += nq;
    } else {
        // (weighted Hamming: the rows the integer pre-filter could not serve -- list overflow, ids beyond 16 bits -- count as
        //  fallbacks too)
        if (p.ham_int) HIP_TRY(launch::add_counter(ix->fail_count.p, ix->fail_total.p, st));
        ix->stats.exact_only_queries += nq;
    }
    HIP_TRY(hipEventRecord(ct.e1, st));
    ct.pending = true;
    HIP_TRY(hipEventRecord(ix->ev_ws, st));
    ix->ws_busy = true;
    ix->stats.queries += nq;
    return SKNNR_OK;
}

// Device-resident core: nq rows at xdev (raw if affine else transformed), outputs on device.
// raw / id_offset: shard candidates (sknnr_shard_candidates): squared values ascending by (value, index), indices +
// id_offset, no post-steps
int run_device(sknnr_index* ix, const void* xdev, long nq, const sknnr_query_opts* o, double* d_dist,
               long* d_idx, hipStream_t st, int raw = 0, long id_offset = 0) {
    zero_records(ix);
    ++ix->search_calls;
    if (xdev && uses_forest(ix, o)) return run_forest(ix, xdev, nq, o, d_dist, d_idx, st);
    const SearchPlan p = plan_search(describe(ix), o, nq, xdev != nullptr, raw);
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 query rows in one call");
    if (p.affine && ix->ks == 0)
        return fail(SKNNR_ERR_UNSUPPORTED, "d = %d > 128 with an affine map is outside the HIP envelope", ix->d);
    // the previous call may have run on another stream: its last kernel must be done with the workspace
    if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));
    int rc = ensure_workspace(ix, p, nq, st);
    if (rc) return rc;
    const double* xq_call = p.to_xt ? ix->xt.p : (p.self_rows ? ix->ref64.p + o->row_offset * ix->d : (const double*)xdev);
    const SelectArgs call = make_select_args(ix, o, p.kk, xq_call, nq, d_dist, d_idx, raw, id_offset);
    // timing record of this call (a ring: an old record still pending is folded into the totals first)
    sknnr_index::CallTiming& ct = ix->timing[ix->timing_next];
    ix->timing_next = (ix->timing_next + 1) % sknnr_index::kTimingRing;
    resolve_call(ix, ct);
    if (!ct.e0) {
        HIP_TRY(hipEventCreate(&ct.e0));
        HIP_TRY(hipEventCreate(&ct.e1));
    }
    ct.coarse_used = 0;
    ct.coarse_rows = 0;
    HIP_TRY(hipEventRecord(ct.e0, st));
    if (p.check_finite && !(p.coarse || p.to_xt)) {
        // no prep kernel reads the rows on this path: scan them here
        const long n_el = nq * (long)p.d_x;
        HIP_TRY(launch::check_finite((const double*)xdev, n_el, ix->status.p, st));
    }
    for (long c0 = 0; c0 < nq; c0 += p.chunk) {
        const long n = std::min(p.chunk, nq - c0);
        rc = p.coarse ? coarse_chunk(ix, p, call, xdev, c0, n, ct, st) : (p.to_xt ? prep_chunk(ix, p, call, xdev, c0, n, st) : SKNNR_OK);
        if (rc) return rc;
    }
    if (p.ham_int && (rc = hamming_pass(ix, p, call, nq, st))) return rc;
    return scan_tail(ix, p, call, nq, ct, st);
}

// Rows of one forest-map chunk: the node ids of at most 2^18 rows (the integer Hamming pre-filter's chunk) and 4 GiB.  A
// call thus never holds more ids than the (nq, n_trees) matrix a call on node ids is handed.
long forest_chunk_rows(int n_trees) {
    const long by_bytes = (4L << 30) / (8L * std::max(n_trees, 1));
    return std::max<long>(kFtRows, std::min<long>(1L << 18, by_bytes) / kFtRows * kFtRows);
}

ForestArgs forest_args(const sknnr_index* ix, const void* x, long n, int x_dtype, double* out, int* status) {
    ForestArgs a{};
    a.x = x;
    a.x_dtype = x_dtype;
    a.nq = n;
    a.d_in = ix->f_d_in;
    a.nodes = ix->f_nodes.p;
    a.tree_off = ix->f_off.p;
    a.tree_depth = ix->f_depth.p;
    a.n_trees = ix->d;
    a.out = out;
    a.status = status;
    return a;
}

// Raw rows through the forest map, chunk by chunk: the forest kernel writes the chunk's node ids into the workspace, then
// the chunk is an ordinary call on node ids (Hamming pre-filter, re-score, exact scan, post-steps) at its global rows.
int run_forest(sknnr_index* ix, const void* xdev, long nq, const sknnr_query_opts* o, double* d_dist, long* d_idx,
               hipStream_t st) {
    if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));  // f_ids belongs to the workspace
    const long chunk = forest_chunk_rows(ix->d);
    HIP_TRY(ix->f_ids.ensure((size_t)std::min(chunk, nq) * ix->d));
    const size_t row_bytes = (size_t)ix->f_d_in * dtype_bytes(o->query_dtype);
    const int k = o->n_neighbors;
    for (long c0 = 0; c0 < nq; c0 += chunk) {
        const long n = std::min(chunk, nq - c0);
        const ForestArgs fa = forest_args(ix, (const char*)xdev + (size_t)c0 * row_bytes, n, o->query_dtype, ix->f_ids.p,
                                          o->check_finite ? ix->status.p : nullptr);
        HIP_TRY(launch::forest_apply(fa, st));
        sknnr_query_opts oc = *o;
        oc.apply_affine = 0;
        oc.query_dtype = SKNNR_DTYPE_F64;
        oc.check_finite = 0;  // (node ids are finite; the forest kernel has checked the rows)
        oc.row_offset = o->row_offset + c0;
        int rc = run_device(ix, ix->f_ids.p, n, &oc, d_dist ? d_dist + c0 * k : nullptr, d_idx + c0 * k, st);
        if (rc) return rc;
    }
    return SKNNR_OK;
}

}  // namespace

// ----------------------------------------------------------------------------------------
// host-buffer pipeline
// ----------------------------------------------------------------------------------------
// skip (a bootstrap only; else null): (nq) rows that enter no tally
static int launch_predict(sknnr_index* ix, const Reduction& red, const double* dist, const long* idx, const double* w, long nq,
                          int k, int mode, int law, double* out, hipStream_t st, const unsigned char* skip = nullptr);
// n rows of a tile of the open stream into the handle's accumulators (sknnr_stream_set_tally), on `st` behind their search
static int tally_tile(sknnr_index* ix, const double* dist, const long* idx, long n, int k, hipStream_t st);
// what one zonal launch converts and tallies with: the zones, the tile's width, the prediction lane's conversion (scale /
// offset on the device, or null) and whether some column has classes
struct ZonalSpec {
    int n_zones, c, dtype;
    const double *scale, *offset;
    bool classes;
};
// n pixels of a tile of the open stream -- its full-layout (n, c) float64 predictions and its zone codes -- into the
// handle's accumulators (sknnr_stream_set_zonal), on `st` behind the reduction
static int zonal_tile(sknnr_index* ix, const ZonalSpec& z, const double* pred, const int32_t* zones, long n, hipStream_t st);
// what one launch of a domain stream codes with: the column of the score, the table's length, the threshold
struct DomainSpec {
    int rank0;
    long m;
    int has_threshold;
    double threshold;
};
// n pixels of a tile of the open stream -- its full-layout (n, k) float64 distances -- into the handle's accumulators
// (sknnr_stream_set_domain) and into `codes` (device, or null), on `st` behind the search; pred (or null): the (n, pred_cols)
// prediction tile whose beyond rows become NaN, behind the reduction
static int domain_tile(sknnr_index* ix, const DomainSpec& d, const double* dist, long n, int k, uint8_t* codes, double* pred,
                       int pred_cols, hipStream_t st);

namespace {

// ---- nodata front end (mask.hip.h) --------------------------------------------------------------------------------------
int mask_ensure(MaskBufs& m, long n, size_t row_bytes, int k, int t, bool want_dist, bool want_pred) {
    HIP_TRY(m.valid.ensure((size_t)n));
    HIP_TRY(m.blk.ensure((size_t)mask_blocks(n)));
    HIP_TRY(m.rank.ensure((size_t)n));
    HIP_TRY(m.nvalid.ensure(1));
    if (!m.pin_nv) HIP_TRY(hipHostMalloc((void**)&m.pin_nv, sizeof(long), hipHostMallocDefault));
    // (sized for the tile, not for its valid rows: the slot is sized before the count is known)
    HIP_TRY(m.cx.ensure((size_t)n * row_bytes));
    HIP_TRY(m.ci.ensure((size_t)n * k));
    if (want_dist || want_pred) HIP_TRY(m.cd.ensure((size_t)n * k));
    if (want_pred) HIP_TRY(m.cp.ensure((size_t)n * t));
    return SKNNR_OK;
}

// Mask and scan of one tile on `st`, and the 8-byte copy of its valid count behind them: *m.pin_nv holds the count once
// the caller has waited for `st` (or for an event recorded behind this).
int mask_front(MaskBufs& m, const void* x, long n, int d_in, int x_dtype, const double* nodata_dev, hipStream_t st) {
    MaskArgs a{};
    a.x = x;
    a.x_dtype = x_dtype;
    a.nq = n;
    a.d_in = d_in;
    a.nodata = nodata_dev;
    a.valid = m.valid.p;
    a.blk = m.blk.p;
    HIP_TRY(launch::row_mask(a, m.nvalid.p, st));
    HIP_TRY(hipMemcpyAsync(m.pin_nv, m.nvalid.p, sizeof(long), hipMemcpyDeviceToHost, st));
    return SKNNR_OK;
}

int mask_compact(MaskBufs& m, const void* x, long n, size_t row_bytes, hipStream_t st) {
    CompactArgs a{};
    a.x = x;
    a.out = m.cx.p;
    a.nq = n;
    a.valid = m.valid.p;
    a.blk_off = m.blk.p;
    a.rank = m.rank.p;
    HIP_TRY(launch::row_compact(a, row_bytes, st));
    return SKNNR_OK;
}

// The search body of every call and tile, on `st`: the n rows at x searched into dd / di, their neighbours tallied if asked,
// and reduced into d_pred if non-null.  What sits between a search and its reduction goes here, once.
// (replay_tile keeps its own order -- decode, reduce, blank, tally: there the tally must see the tile's final state.)
int search_tile(sknnr_index* ix, const Reduction& red, const void* x, long n, const sknnr_query_opts* o, double* dd, long* di,
                double* d_pred, bool tally, hipStream_t st) {
    const int k = o->n_neighbors;
    int rc = run_device(ix, x, n, o, dd, di, st);
    if (rc) return rc;
    if (tally && (rc = tally_tile(ix, dd, di, n, k, st))) return rc;
    if (d_pred) return launch_predict(ix, red, dd, di, nullptr, n, k, o->weight_mode, o->weight_law, d_pred, st);
    return SKNNR_OK;
}

// The search of a masked tile whose valid count nv the host knows, on `st`: in place when every row is valid, nothing but
// the fill when none is, else on the packed rows (mask_compact has run, on `st` or in front of an event `st` waits for) and
// expanded.  o->row_offset counts the valid rows in front of the tile.  d_pred: also predict; d_dist / d_idx may be null.
// tally (a stream's tile; d_dist is given): the valid rows' neighbours are tallied where the search wrote them -- the whole
// tile in place, or the packed rows -- never the expanded ones: a caller's fill_index need not be negative.
int mask_finish(sknnr_index* ix, const Reduction& red, MaskBufs& m, const void* x, long n, long nv, const sknnr_query_opts* o,
                long fill_index, double* d_dist, long* d_idx, double* d_pred, long valid_so_far, hipStream_t st,
                bool tally = false) {
    const int k = o->n_neighbors, t = red.cols(ix->t);  // (the prediction rows' width: the plan's entries, or the targets)
    const size_t row_bytes = (size_t)query_cols(ix, o) * dtype_bytes(o->query_dtype);
    int rc;
    if (nv == n) {
        double* dd = d_dist ? d_dist : (d_pred ? m.cd.p : nullptr);
        long* di = d_idx ? d_idx : m.ci.p;
        if ((rc = search_tile(ix, red, x, n, o, dd, di, d_pred, tally, st))) return rc;
    } else {
        ExpandArgs e{};
        if (nv > 0) {
            double* cd = (d_dist || d_pred) ? m.cd.p : nullptr;
            if ((rc = search_tile(ix, red, m.cx.p, nv, o, cd, m.ci.p, d_pred ? m.cp.p : nullptr, tally, st))) return rc;
            e.valid = m.valid.p;
            e.rank = m.rank.p;
            e.c_idx = m.ci.p;
            e.c_dist = cd;
            e.c_pred = m.cp.p;
        } else {
            zero_records(ix);  // (no search ran)
        }
        e.nq = n;
        e.k = k;
        e.t = t;
        e.idx = d_idx;
        e.dist = d_dist;
        e.pred = d_pred;
        e.fill_index = fill_index;
        HIP_TRY(launch::row_expand(e, st));
        HIP_TRY(hipEventRecord(ix->ev_ws, st));  // (the packed results belong to the workspace of a device-memory call)
        ix->ws_busy = true;
    }
    const int64_t rec[8] = {1, n, nv, nv == n ? 1 : (nv == 0 ? 2 : 0), mask_blocks(n), (int64_t)row_bytes, valid_so_far + nv, 0};
    std::copy(rec, rec + 8, ix->last.mask);
    return SKNNR_OK;
}

// A masked device-memory call: mask, one 8-byte read of the valid count (synchronises `st`), then the search.
int run_device_masked(sknnr_index* ix, const Reduction& red, const void* q, long nq, const sknnr_query_opts* o,
                      const double* nodata, long fill_index, double* d_dist, long* d_idx, double* d_pred, hipStream_t st,
                      int64_t* out_n_valid) {
    const int d_x = query_cols(ix, o);
    const size_t row_bytes = (size_t)d_x * dtype_bytes(o->query_dtype);
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 query rows in one call");
    if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));  // the mask buffers belong to the workspace
    MaskBufs& m = ix->mask;
    int rc = mask_ensure(m, nq, row_bytes, o->n_neighbors, red.cols(ix->t), d_dist != nullptr, d_pred != nullptr);
    if (rc) return rc;
    HIP_TRY(ix->m_nodata.ensure((size_t)d_x));
    HIP_TRY(hipMemcpyAsync(ix->m_nodata.p, nodata, (size_t)d_x * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = mask_front(m, q, nq, d_x, o->query_dtype, ix->m_nodata.p, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    const long nv = *m.pin_nv;
    if (nv > 0 && nv < nq && (rc = mask_compact(m, q, nq, row_bytes, st))) return rc;
    if (out_n_valid) *out_n_valid = nv;
    return mask_finish(ix, red, m, q, nq, nv, o, fill_index, d_dist, d_idx, d_pred, 0, st);
}

}  // namespace

namespace {

constexpr long kHostChunkRows = 1L << 20;  // rows per pipeline slot (SKNNR_HOST_CHUNK_ROWS overrides)

long host_chunk_rows() {
    static const long v = [] {
        const char* e = std::getenv("SKNNR_HOST_CHUNK_ROWS");
        const long r = e ? std::atol(e) : 0;
        return r >= 1024 ? r : kHostChunkRows;
    }();
    return v;
}

template <typename T>
int ensure_pinned(T*& p, size_t& have, size_t want) {
    if (p && have >= want) return SKNNR_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    HIP_TRY(hipHostMalloc((void**)&p, std::max<size_t>(want, 1) * sizeof(T), hipHostMallocDefault));
    have = want;
    return SKNNR_OK;
}

// ---- neighbour replay: what a pipeline's tiles hold instead of feature rows (replay.hip.h) -----------------------------------
struct ReplaySpec {
    bool on = false;
    int ks = 0;                      // stored columns (the pipeline's k leading ones are used)
    int idx_bytes = 8;               // 4: int32, 8: int64
    int dist_kind = kReplayDistNone;
    bool ids = false;                // the stored values are ids of the handle's table (sknnr_index_set_replay_ids)
    long fill_index = -1;
    // what host_stage.h lays a staged tile out by
    ReplayLayout layout() const { return {ks, idx_bytes, dist_kind == kReplayDistNone ? 0 : (dist_kind == kReplayDistF32 ? 4 : 8)}; }
};

// Pageable host arrays in, pageable host arrays out, through kHostSlots pinned/device slots:
//   host thread : copy tile c into its slot's pinned buffer | copy results of tile c - kHostSlots out
//   st_h2d      : pinned -> device                          (PCIe)
//   st_run      : prep / pre-filter / finalise / scan [+ predict]
//   st_d2h      : device -> pinned                          (PCIe)
// so that PCIe in, kernels and PCIe out of neighbouring tiles overlap.  The state lives in a HostPipe so
// that the streamed entry points (sknnr_stream_*) keep the pipeline full ACROSS calls: a pushed tile's
// results leave the slot when the slot is needed again (kHostSlots tiles later) or at flush.
struct HostPipe {
    sknnr_index* ix = nullptr;
    sknnr_query_opts o{};        // o.row_offset advances with every submitted tile
    int k = 0, t = 0, d_x = 0;
    // One output (kLaneIdx / kLaneDist / kLanePred) as this pipeline delivers it; pipe_open and sknnr_stream_set_output fill these in.
    struct Lane {
        bool want = false;        // the pipeline delivers it (a push may still leave a wanted lane out)
        bool search_out = false;  // the search writes its device buffer: sized whether the lane is wanted or not
        int cols = 0;             // k, k, t
        int kind = kNarrowValue;  // the conversion's source kind (narrow.hip.h)
        int dtype = 0;            // sknnr_dtype of a typed output (sknnr_stream_set_output), 0 = as computed (int64 / float64)
        size_t esz = 8;           // bytes of one element
        // predictions only: the per-target scale / offset of their conversion (device, or null), and their NaN fill
        const double *scale = nullptr, *offset = nullptr;
        int has_fill = 0;
        double fill = 0.0;
        // indices only: the id table of their conversion (device, or null: row indices leave) and what a negative becomes
        const long* table = nullptr;
        long fill_id = 0;
        // the lane leaves through the conversion kernel, from its narrow buffer: typed, or the index lane with a table
        bool converts() const { return dtype != 0 || table != nullptr; }
    } lane[kLanes];
    bool mask_dist = false;  // the masked path is handed the distance buffer: distances leave, or the reduction or the tally reads them
    // The side products every tile feeds, into the `stream` buffers of the handle's member of the same name:
    // tally (sknnr_stream_set_tally): the tile's neighbours are tallied;
    // zonal (sknnr_stream_set_zonal): the prediction tile is tallied by zone -- zones by c columns, zonal_hist elements of
    // class blocks (0: no column has classes);
    // domain (sknnr_stream_set_domain): the tile's distances are coded against the table and tallied; domain_mask: the
    // prediction rows of beyond pixels become NaN in front of the conversion and the zonal tally.
    struct Products {
        bool tally = false, zonal = false, domain = false;
        int zonal_zones = 0, zonal_c = 0;
        size_t zonal_hist = 0;
        bool domain_mask = false;
        DomainSpec domain_spec{};
    } prod;
    long push_no = -1;  // the push in progress (Push::push_no): every push counts, an empty one too -- the caller's tile numbers
    // neighbour replay (sknnr_replay_begin): the tiles are stored neighbours, decoded on the device where a search would
    // run (replay_tile); replay_tot / replay_first: pixels, masked and unknown pixels of the tiles that have left so far,
    // and the first push that held unknown values (-1: none yet)
    ReplaySpec replay{};
    int64_t replay_tot[3] = {};
    long replay_first = -1;
    size_t x_esz = sizeof(double);  // bytes per element of the caller's rows (opts->query_dtype)
    // nodata front end: every tile is masked behind its host-to-device copy, and o.row_offset advances by its VALID rows
    const double* nodata_dev = nullptr;  // (d_x) on the device, or null: no mask
    long fill_index = -1;
    long row_offset0 = 0;                // o.row_offset when the pipeline was opened
    // The reduction of this pipeline's tiles: a one-shot call's, or what sknnr_stream_set_statistics, _set_plan or
    // _set_bootstrap installed (a stream takes one of the three).  The prediction lane is red.cols(t) wide.  With a
    // bootstrap the search (or the stored lists) has k = kw columns.
    Reduction red;
    struct Pending {
        bool live = false;
        Push push;         // the tile: pixels [off, off + n) of this push
        long off = 0, n = 0;
        std::future<int> out_done;  // copy-out job of the slot's tile (w_out)
    } pending[kHostSlots];
    int slot_of = 0;
    std::packaged_task<int()> deferred[kHostSlots];  // SKNNR_PIPE_WORKERS=0: the copy-out jobs, run when the slot is drained
    // look-ahead copy-in (a push knows its next tile): the job that stages tile (ahead_push_no, ahead_off) into slot ahead_slot
    std::future<int> ahead_done;
    long ahead_push_no = -1, ahead_off = 0;
    int ahead_slot = -1;
    int d2h_slot = -1;  // slot whose kernels are enqueued and whose device-to-host copies are not yet (pipe_enqueue_d2h)
    double ms_copy_in = 0, ms_copy_out = 0, ms_wait = 0, ms_enqueue = 0;  // host-thread time per phase (SKNNR_PIPE_TRACE=1)
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
bool pipe_trace() {
    static const bool v = std::getenv("SKNNR_PIPE_TRACE") != nullptr;
    return v;
}
// SKNNR_PIPE_WORKERS=0 (A/B runs): no copy-in look-ahead, and the copy-out jobs run on the calling thread
bool pipe_workers() {
    static const bool v = [] { const char* e = std::getenv("SKNNR_PIPE_WORKERS"); return !(e && std::atoi(e) == 0); }();
    return v;
}

int pipe_open(HostPipe& p, sknnr_index* ix, const sknnr_query_opts* o, const Reduction& red, bool want_dist, bool want_pred) {
    p = HostPipe{};
    p.ix = ix;
    p.o = *o;
    p.k = o->n_neighbors;
    p.t = ix->t;
    p.red = red;
    // The indices are always wanted (so their pinned buffer is sized even for pushes that leave them out), and the search
    // writes indices and distances whether or not the distances leave.
    p.lane[kLaneIdx] = {true, true, p.k, kNarrowIndex};  // (want, search_out, cols, kind)
    p.lane[kLaneDist] = {want_dist, true, p.k, kNarrowValue};
    p.lane[kLanePred] = {want_pred, false, red.cols(ix->t), kNarrowValue};
    p.mask_dist = want_dist || want_pred;
    p.d_x = query_cols(ix, o);
    p.x_esz = (size_t)dtype_bytes(o->query_dtype);
    p.row_offset0 = o->row_offset;
    // (each object on its own: a creation that failed half way is completed by the next call, never skipped)
    for (hipStream_t* h : {&ix->st_h2d, &ix->st_run, &ix->st_d2h})
        if (!*h) HIP_TRY(hipStreamCreateWithFlags(h, hipStreamNonBlocking));
    for (auto& sl : ix->slot)
        for (hipEvent_t* e : {&sl.ev_h2d, &sl.ev_done, &sl.ev_d2h})
            if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (!ix->w_in) ix->w_in.reset(new HostWorker());
    if (!ix->w_out) ix->w_out.reset(new HostWorker());
    return SKNNR_OK;
}

// Slot b's previous tile has left (its copy-out job, on w_out, is done): the slot's buffers may be reused.
int pipe_enqueue_d2h(HostPipe& p);
int pipe_drain(HostPipe& p, int b) {
    auto& pd = p.pending[b];
    if (!pd.live) return SKNNR_OK;
    if (p.d2h_slot == b) {  // (its results have not even been sent yet)
        int rc = pipe_enqueue_d2h(p);
        if (rc) return rc;
    }
    const double t0 = now_ms();
    if (p.deferred[b].valid()) {
        p.deferred[b]();
        p.deferred[b] = std::packaged_task<int()>();
    }
    const int rc = pd.out_done.valid() ? pd.out_done.get() : SKNNR_OK;
    p.ms_wait += now_ms() - t0;
    pd.live = false;
    if (rc) return fail(rc, "host pipeline: copying a tile's results out failed (HIP error while waiting for the device-to-host copy)");
    if (p.replay.on) {
        // (the tile's record arrived with its results: the copy-out job waited for the event behind both)
        const unsigned long long* rec = p.ix->pin_replay + (size_t)b * kReplayRecWords;
        for (int w = 0; w < 3; ++w) p.ix->last_replay[w] = (int64_t)rec[w];
        for (int w = 0; w < 3; ++w) p.replay_tot[w] += (int64_t)rec[w];
        if (rec[kReplayRecUnknown] && p.replay_first < 0) p.replay_first = pd.push.push_no;
    }
    return SKNNR_OK;
}

// Drain slot b and size its pinned / device buffers for a tile of n pixels of push u.
int pipe_prepare_slot(HostPipe& p, int b, const Push& u, long n) {
    sknnr_index* ix = p.ix;
    auto& sl = ix->slot[b];
    const bool planes = u.band_first;
    int rc = pipe_drain(p, b);  // the slot's previous tile must have left before its buffers are reused
    if (rc) return rc;
    // the tile's rows -- or, replayed, its stored neighbours -- in 8-byte units
    const size_t x_f64 = (u.staged_bytes(n) + 7) / 8;
    if ((rc = ensure_pinned(sl.pin_x, sl.pin_x_n, x_f64))) return rc;
    HIP_TRY(sl.dev_x.ensure(x_f64));
    if (u.source == Push::kBands) HIP_TRY(sl.dev_xp.ensure(x_f64));  // (band-first rows only: the uploaded planes)
    if (p.replay.on) HIP_TRY(sl.mask.valid.ensure((size_t)n));     // (the decode's bad-pixel flags)
    if (p.prod.zonal) {
        if ((rc = ensure_pinned(sl.pin_z, sl.pin_z_n, (size_t)n))) return rc;
        HIP_TRY(sl.dev_z.ensure((size_t)n));
    }
    if (p.prod.domain) {
        if ((rc = ensure_pinned(sl.pin_dom, sl.pin_dom_n, (size_t)n))) return rc;
        HIP_TRY(sl.dev_dom.ensure((size_t)n));
    }
    for (int l = 0; l < kLanes; ++l) {
        const HostPipe::Lane& ln = p.lane[l];
        auto& sb = sl.lane[l];
        // (a wanted output leaves at its own width: 8-byte units of n * cols * element bytes; n * cols without a type)
        const size_t wide = (size_t)n * ln.cols, units = lane_units(n, ln.cols, ln.esz);
        if (ln.want && (rc = ensure_pinned(sb.pin, sb.pin_n, units))) return rc;
        if (ln.want || ln.search_out) HIP_TRY(sb.dev.ensure(wide));
        if (ln.want && ln.converts()) HIP_TRY(sb.nar.ensure(units));
        if (ln.want && !ln.converts() && planes) HIP_TRY(sb.planes.ensure(wide));  // (the untyped results as planes)
    }
    if (p.nodata_dev && (rc = mask_ensure(sl.mask, n, (size_t)p.d_x * p.x_esz, p.k, p.lane[kLanePred].cols, p.mask_dist, p.lane[kLanePred].want)))
        return rc;
    return SKNNR_OK;
}

// Device-to-host copies and the copy-out job of the tile whose kernels were enqueued last (slot p.d2h_slot), if any.
// BOTH directions use one stream (st_h2d), tile j's rows in front of tile j-1's results: on this stack a device-to-host
// copy that runs while a host-to-device copy is active is not given a DMA engine but executed by a blit kernel
// (__amd_rocclr_copyBuffer, six pieces of ~0.5 ms per tile in a rocprofv3 trace) that shares the CUs with the hot path
// -- the prep kernel beside it took 1.18 ms instead of 0.30, a tile 7.75 ms instead of 5.8 (profiles/r03_host_pipeline.txt).
// One stream keeps every transfer on the DMA engine; per tile 4.5 ms in + 1.4 ms out still fit beside 5.8 ms of kernels.
int pipe_enqueue_d2h(HostPipe& p) {
    const int b = p.d2h_slot;
    if (b < 0) return SKNNR_OK;
    p.d2h_slot = -1;
    sknnr_index* ix = p.ix;
    auto& sl = ix->slot[b];
    auto& pd = p.pending[b];
    const long n = pd.n;
    static const bool one_stream = [] { const char* e = std::getenv("SKNNR_PIPE_ONE_STREAM"); return !(e && std::atoi(e) == 0); }();
    hipStream_t st = one_stream ? ix->st_h2d : ix->st_d2h;
    HIP_TRY(hipStreamWaitEvent(st, sl.ev_done, 0));
    const bool planes = pd.push.band_first;  // (then the plane buffers hold the untyped results, packed (k or t, n))
    const long out_stride = pd.push.out_stride;
    struct Leg {  // one requested output on its way out: the caller's array (null: none), the pinned bytes, the lane's shape
        void* dst;
        const void* pin;
        int cols;
        size_t esz;
    };
    std::array<Leg, kLanes> legs{};
    size_t moved = 0;
    for (int l = 0; l < kLanes; ++l) {
        if (!pd.push.out[l]) continue;
        const HostPipe::Lane& ln = p.lane[l];
        const auto& sb = sl.lane[l];
        // (a converted output leaves from its narrow buffer, rows or planes alike, at its own element size)
        const void* src = ln.converts() ? sb.nar.p : planes ? sb.planes.p : sb.dev.p;
        const size_t bytes = lane_bytes(n, ln.cols, ln.esz);
        HIP_TRY(hipMemcpyAsync(sb.pin, src, bytes, hipMemcpyDeviceToHost, st));
        moved += bytes;
        legs[l] = Leg{pd.push.out_at(l, pd.off, ln.cols, ln.esz), sb.pin, ln.cols, ln.esz};
    }
    ix->last_narrow[5] = (int64_t)moved;
    uint8_t* const dom_dst = pd.push.domain_at(pd.off);  // (a domain pipeline's code plane: n bytes in pixel order in either layout)
    const uint8_t* const dom_pin = sl.pin_dom;
    if (dom_dst) HIP_TRY(hipMemcpyAsync(sl.pin_dom, sl.dev_dom.p, (size_t)n, hipMemcpyDeviceToHost, st));
    if (p.replay.on)  // (the tile's record: pipe_drain adds it up once the copy-out job has waited for ev_d2h)
        HIP_TRY(hipMemcpyAsync(ix->pin_replay + (size_t)b * kReplayRecWords, ix->replay_rec.p + (size_t)b * kReplayRecWords,
                               kReplayRecWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(sl.ev_d2h, st));
    // the copy-out leg: wait for the tile's device-to-host copies, then pinned -> the caller's arrays (w_out, in order)
    {
        const int device = ix->device;
        hipEvent_t ev = sl.ev_d2h;
        auto job = [=]() -> int {
            if (hipSetDevice(device) != hipSuccess || hipEventSynchronize(ev) != hipSuccess) return SKNNR_ERR_HIP;
            for (const Leg& g : legs) {
                if (!g.dst) continue;
                // (planes: k (or t) contiguous segments of n elements, each to its plane of the caller's array)
                if (planes) unstage_planes(g.dst, g.pin, g.cols, n, out_stride, g.esz);
                else parallel_copy(g.dst, g.pin, lane_bytes(n, g.cols, g.esz));
            }
            if (dom_dst) parallel_copy(dom_dst, dom_pin, (size_t)n);
            return SKNNR_OK;
        };
        if (pipe_workers()) {
            pd.out_done = ix->w_out->post(job);
        } else {  // (A/B: the round-2 behaviour -- the copy runs on this thread when the slot is drained)
            std::packaged_task<int()> task(job);
            pd.out_done = task.get_future();
            p.deferred[b] = std::move(task);
        }
    }
    return SKNNR_OK;
}

// The replayed tile of slot b on st_run, where a search tile has its search, tally and reduction: the decode of the
// uploaded stored neighbours into d_idx (n, k) / d_dist (n, k; null without stored distances); with d_pred the reduction
// on the provisional tile and the blanking pass behind it (replay.hip.h); then the tally, on the tile's final state, whose
// negative indices it skips.
int replay_tile(HostPipe& p, int b, long n, bool planes, long* d_idx, double* d_dist, double* d_pred) {
    sknnr_index* ix = p.ix;
    auto& sl = ix->slot[b];
    const ReplaySpec& r = p.replay;
    hipStream_t st = ix->st_run;
    unsigned long long* rec = ix->replay_rec.p + (size_t)b * kReplayRecWords;
    HIP_TRY(hipMemsetAsync(rec, 0, kReplayRecWords * sizeof(unsigned long long), st));
    ReplayArgs a{};
    a.idx = sl.dev_x.p;
    a.dist = d_dist ? (const char*)sl.dev_x.p + replay_dist_offset(r.layout(), n) : nullptr;
    a.n = n;
    a.ks = r.ks;
    a.k = p.k;
    a.in_stride = n;  // (the staged planes are packed)
    a.fill_index = r.fill_index;
    a.n_ref = ix->n_ref;
    a.id_sorted = r.ids ? ix->r_id_sorted.p : nullptr;
    a.id_perm = r.ids ? ix->r_id_perm.p : nullptr;
    a.m = r.ids ? ix->r_id_n : 0;
    a.provisional = d_pred ? 1 : 0;
    a.out_idx = d_idx;
    a.out_dist = d_dist;
    a.bad = sl.mask.valid.p;
    a.rec = rec;
    HIP_TRY(launch::replay(a, r.idx_bytes, r.dist_kind, planes, st));
    int rc;
    if (d_pred) {
        // (the skip flags -- a bootstrap stage: the provisional rows of bad pixels enter no tally)
        rc = launch_predict(ix, p.red, d_dist, d_idx, nullptr, n, p.k, p.o.weight_mode, p.o.weight_law, d_pred, st, sl.mask.valid.p);
        if (rc) return rc;
        const ReplayBlankArgs ba{sl.mask.valid.p, n, p.k, p.lane[kLanePred].cols, d_idx, d_dist, d_pred};
        HIP_TRY(launch::replay_blank(ba, st));
    }
    if (p.prod.tally && (rc = tally_tile(ix, d_dist, d_idx, n, p.k, st))) return rc;
    const int64_t lr[8] = {0, 0, 0, replay_instance(r.idx_bytes, r.dist_kind, planes), r.ids ? 1 : 0,
                           0, p.k, r.ks};  // ([0 .. 2]: pipe_drain, when the tile has left; [5]: pipe_submit)
    std::copy(lr + 3, lr + 8, ix->last_replay + 3);
    return SKNNR_OK;
}

// One tile of at most host_chunk_rows() pixels: [off, off + n) of push u.  Its input pixels may be reused by the caller as
// soon as this returns.
// n_next: the pixels of the tile the same push will submit next (0: none): they are staged into the next slot's pinned
// buffer by the copy-in worker while this tile is enqueued and the caller waits for older results.
int pipe_submit(HostPipe& p, const Push& u, long off, long n, long n_next) {
    sknnr_index* ix = p.ix;
    const bool planes = u.band_first, planes_in = u.source == Push::kBands;  // (stored planes are decoded as they are)
    const int b = p.slot_of;
    p.slot_of = (p.slot_of + 1) % kHostSlots;
    auto& sl = ix->slot[b];
    const auto& idx = sl.lane[kLaneIdx];
    const auto& dist = sl.lane[kLaneDist];
    const auto& pred = sl.lane[kLanePred];
    const bool want_pred = p.lane[kLanePred].want;
    const int k = p.k, d_x = p.d_x;
    const long searches0 = ix->search_calls;
    int rc;
    const double t_in = now_ms();
    if (p.ahead_slot == b && p.ahead_push_no == u.push_no && p.ahead_off == off && p.ahead_done.valid()) {
        rc = p.ahead_done.get();  // staged ahead by the worker (the slot was prepared when the job was posted)
        p.ahead_slot = -1;
        if (rc) return rc;
    } else {
        if ((rc = pipe_prepare_slot(p, b, u, n))) return rc;
        u.stage(sl.pin_x, off, n);
        if (u.zones) parallel_copy(sl.pin_z, u.zones + off, (size_t)n * sizeof(int32_t));
    }
    const double t_enq = now_ms();
    p.ms_copy_in += t_enq - t_in;
    HIP_TRY(hipMemcpyAsync(planes_in ? sl.dev_xp.p : sl.dev_x.p, sl.pin_x, u.staged_bytes(n), hipMemcpyHostToDevice, ix->st_h2d));
    if (planes_in) {  // behind the copy, in front of the mask: dev_x as an uploaded row tile would have filled it
        PlanesArgs pa{sl.dev_xp.p, sl.dev_x.p, n, d_x, n};
        HIP_TRY(launch::planes_to_rows(pa, (int)p.x_esz, ix->st_h2d));
    }
    if (p.prod.zonal)  // (behind the tile's rows, in front of ev_h2d)
        HIP_TRY(hipMemcpyAsync(sl.dev_z.p, sl.pin_z, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ix->st_h2d));
    long nv = n;  // rows the tile adds to the row offset
    if (p.nodata_dev) {
        // Mask (and, when some rows but not all are masked, compaction) on the copy stream behind the tile's rows: the host
        // waits for this tile's copy and mask only -- not for the previous tile's search, which is on st_run -- and reads
        // the valid count, on which the launches below depend.
        if ((rc = mask_front(sl.mask, sl.dev_x.p, n, d_x, p.o.query_dtype, p.nodata_dev, ix->st_h2d))) return rc;
        HIP_TRY(hipEventRecord(sl.ev_h2d, ix->st_h2d));
        HIP_TRY(hipEventSynchronize(sl.ev_h2d));
        nv = *sl.mask.pin_nv;
        if (nv > 0 && nv < n && (rc = mask_compact(sl.mask, sl.dev_x.p, n, (size_t)d_x * p.x_esz, ix->st_h2d))) return rc;
    }
    HIP_TRY(hipEventRecord(sl.ev_h2d, ix->st_h2d));
    // the PREVIOUS tile's results travel behind this tile's rows, on the same stream (see pipe_enqueue_d2h)
    if ((rc = pipe_enqueue_d2h(p))) return rc;
    HIP_TRY(hipStreamWaitEvent(ix->st_run, sl.ev_h2d, 0));
    if (p.replay.on) {
        // stored neighbours: the decode leaves the tile as a search and its nodata expansion would; nothing of the search runs
        rc = replay_tile(p, b, n, planes, idx.i64(), p.replay.dist_kind != kReplayDistNone ? dist.f64() : nullptr,
                         want_pred ? pred.f64() : nullptr);
        if (rc) return rc;
    } else if (p.nodata_dev) {
        // (distances only where the slot has packed distances to expand from: mask_ensure sizes them by the same rule)
        rc = mask_finish(ix, p.red, sl.mask, sl.dev_x.p, n, nv, &p.o, p.fill_index, p.mask_dist ? dist.f64() : nullptr, idx.i64(),
                         want_pred ? pred.f64() : nullptr, p.o.row_offset - p.row_offset0, ix->st_run, p.prod.tally);
        if (rc) return rc;
    } else {
        rc = search_tile(ix, p.red, sl.dev_x.p, n, &p.o, dist.f64(), idx.i64(), want_pred ? pred.f64() : nullptr, p.prod.tally, ix->st_run);
        if (rc) return rc;
    }
    // distance domain: the full-layout float64 distance tile (masked rows are NaN), whether or not the distances leave;
    // with the mask, the prediction rows of beyond pixels become NaN here, in front of the zonal tally and the conversion
    if (p.prod.domain) {
        rc = domain_tile(ix, p.prod.domain_spec, dist.f64(), n, k, u.domain_out ? sl.dev_dom.p : nullptr,
                         p.prod.domain_mask ? pred.f64() : nullptr, p.lane[kLanePred].cols, ix->st_run);
        if (rc) return rc;
    }
    // zonal statistics: the full-layout float64 prediction tile (masked rows are NaN), whether or not this push asked for
    // the predictions, and before any conversion: the kernel converts with the conversion's own device function
    if (p.prod.zonal) {
        const HostPipe::Lane& pl = p.lane[kLanePred];
        const ZonalSpec zs{p.prod.zonal_zones, p.prod.zonal_c, pl.dtype, pl.scale, pl.offset, p.prod.zonal_hist > 0};
        if ((rc = zonal_tile(ix, zs, pred.f64(), sl.dev_z.p, n, ix->st_run))) return rc;
    }
    // The requested results in the form they leave in, behind everything that produces them: a typed output, and the
    // indices of a stream with an id table, typed or not, is converted (and, band-first, transposed in the same pass) into
    // its narrow buffer; an untyped band-first one is transposed; an
    // untyped row output leaves from where it was computed, with no kernel here.
    int planes_out = 0, wide_mask = 0, narrowed = 0, crosswalked = 0;
    for (int l = 0; l < kLanes; ++l) {
        if (!u.out[l]) continue;
        const HostPipe::Lane& ln = p.lane[l];
        const auto& sb = sl.lane[l];
        if (ln.converts()) {
            NarrowArgs na{sb.dev.p, sb.nar.p, n, ln.cols, planes ? n : 0, ln.scale, ln.offset, ln.has_fill, ln.fill, ln.table, ln.fill_id};
            const int dst_bytes = launch::narrow_dst_bytes(ln.kind, ln.dtype, ln.table != nullptr);
            const bool wide = narrow_wide_ok(na.src, na.dst, dst_bytes, n, ln.cols, na.stride);
            HIP_TRY(launch::narrow(na, ln.kind, ln.dtype, wide, ix->st_run));
            narrowed = 1;
            if (ln.table) crosswalked = 1;
            if (wide) wide_mask |= 1 << l;
            if (planes) planes_out += ln.cols;
        } else if (planes) {
            PlanesArgs pa{sb.dev.p, sb.planes.p, n, ln.cols, n};
            HIP_TRY(launch::rows_to_planes(pa, ix->st_run));
            planes_out += ln.cols;
        }
    }
    {
        const int64_t rec[8] = {narrowed, n, p.lane[kLaneIdx].dtype, p.lane[kLaneDist].dtype, p.lane[kLanePred].dtype, 0,
                                wide_mask, crosswalked};  // ([5]: pipe_enqueue_d2h)
        std::copy(std::begin(rec), std::end(rec), ix->last_narrow);
    }
    {
        const int64_t rec[8] = {planes_in ? 1 : 0, n, d_x, (int64_t)p.x_esz, planes ? 1 : 0, planes_out,
                                planes_in ? planes_chunk_cols((int)p.x_esz) : 0, 0};
        std::copy(std::begin(rec), std::end(rec), ix->last_planes);
    }
    HIP_TRY(hipEventRecord(sl.ev_done, ix->st_run));
    auto& pd = p.pending[b];
    pd.live = true;
    pd.push = u;
    pd.off = off;
    pd.n = n;
    if (p.replay.on) ix->last_replay[5] = ix->search_calls - searches0;  // (searches this tile's submission ran: none)
    p.d2h_slot = b;  // its device-to-host copies are enqueued behind the next tile's rows, or by the flush
    p.o.row_offset += nv;
    p.ms_enqueue += now_ms() - t_enq;
    if (pipe_workers() && n_next > 0) {
        // the copy-in leg of the next tile (w_in): its slot is drained and sized here, on this thread
        const int b2 = p.slot_of;
        const long off2 = off + n;
        if ((rc = pipe_prepare_slot(p, b2, u, n_next))) return rc;
        double* dst = ix->slot[b2].pin_x;
        int32_t* dst_z = ix->slot[b2].pin_z;  // (the next tile's zone codes travel with its rows)
        p.ahead_done = ix->w_in->post([u, dst, dst_z, off2, n_next]() -> int {
            u.stage(dst, off2, n_next);
            if (u.zones) parallel_copy(dst_z, u.zones + off2, (size_t)n_next * sizeof(int32_t));
            return SKNNR_OK;
        });
        p.ahead_push_no = u.push_no;
        p.ahead_off = off2;
        p.ahead_slot = b2;
    }
    return SKNNR_OK;
}

// What a push takes from its pipeline: the shape of its source, and its number among the pipeline's pushes.
Push& pipe_adopt(HostPipe& p, Push& u) {
    u.cols = p.d_x;
    u.esz = p.x_esz;
    u.layout = p.replay.layout();
    u.push_no = ++p.push_no;
    return u;
}

// Submit the nq pixels of push u in tiles of at most host_chunk_rows(), cut by tile_cuts (host_stage.h): a pipeline that
// starts empty ramps up.
int pipe_submit_rows(HostPipe& p, const Push& u, long nq) {
    bool idle = p.d2h_slot < 0;
    for (const auto& pd : p.pending) idle = idle && !pd.live;
    const std::vector<long> cuts = tile_cuts(nq, host_chunk_rows(), idle, !std::getenv("SKNNR_PIPE_NO_RAMP"), kRowQuantum);
    long c0 = 0;
    for (size_t i = 0; i < cuts.size(); ++i) {
        const long c1 = cuts[i];
        int rc = pipe_submit(p, u, c0, c1 - c0, i + 1 < cuts.size() ? cuts[i + 1] - c1 : 0);
        if (rc) return rc;
        c0 = c1;
    }
    return SKNNR_OK;
}

// Everything submitted so far is in the caller's arrays when this returns; reports non-finite input.
int pipe_flush(HostPipe& p) {
    if (p.ahead_done.valid()) {  // (a look-ahead copy nobody consumed: only after a failed submit)
        (void)p.ahead_done.get();
        p.ahead_slot = -1;
    }
    {
        int rc = pipe_enqueue_d2h(p);  // the last tile's results have nobody behind them
        if (rc) return rc;
    }
    for (int i = 0; i < kHostSlots; ++i) {
        int rc = pipe_drain(p, (p.slot_of + i) % kHostSlots);  // oldest tile first (the next slot to be reused)
        if (rc) return rc;
    }
    if (pipe_trace()) {
        std::fprintf(stderr, "[pipe] host thread: copy-in %.1f ms, copy-out %.1f ms, waiting for results %.1f ms, enqueue %.1f ms\n",
                     p.ms_copy_in, p.ms_copy_out, p.ms_wait, p.ms_enqueue);
        p.ms_copy_in = p.ms_copy_out = p.ms_wait = p.ms_enqueue = 0;
    }
    if (p.o.check_finite) {
        HIP_TRY(hipStreamSynchronize(p.ix->st_run));
        return poll_status(p.ix);
    }
    return SKNNR_OK;
}

// After a failed submit: no posted job may still touch the caller's memory or the slots when the call returns.
void pipe_abort(HostPipe& p) {
    if (p.ahead_done.valid()) (void)p.ahead_done.get();
    p.ahead_slot = -1;
    p.d2h_slot = -1;
    for (int b = 0; b < kHostSlots; ++b) {
        auto& pd = p.pending[b];
        if (p.deferred[b].valid()) {
            p.deferred[b]();
            p.deferred[b] = std::packaged_task<int()>();
        }
        if (pd.out_done.valid()) (void)pd.out_done.get();
        pd.live = false;
    }
}

// The way out of a failed submit or flush: the error's message survives the clean-up, and nothing of the failed call is
// still in flight on the slots when the caller hears of it.
int pipe_fail(HostPipe& p, int rc) {
    const std::string msg = g_last_error;
    pipe_abort(p);
    (void)hipDeviceSynchronize();
    g_last_error = msg;
    return rc;
}

// Fresh output arrays (numpy's np.empty) are untouched memory: the first write to every page is a fault, and the
// copy-out leg would take them one by one in the middle of the pipeline.  MADV_POPULATE_WRITE (Linux >= 5.14) makes the
// pages present and writable without changing what they hold, so it may run beside the copies; a few threads, because
// the kernel zero-fills the pages it hands out.  Unsupported kernels answer EINVAL: then the copies fault as before.
struct Prefault {
    std::vector<std::thread> th;
    void add(void* ptr, size_t bytes) {
        if (!ptr || bytes < (8u << 20)) return;
        const uintptr_t lo = ((uintptr_t)ptr + 4095) & ~(uintptr_t)4095, hi = ((uintptr_t)ptr + bytes) & ~(uintptr_t)4095;
        if (hi <= lo) return;
        const unsigned n = 4;
        const size_t per = (((hi - lo) / n) + 4095) & ~(size_t)4095;
        for (unsigned i = 0; i < n; ++i) {
            const uintptr_t a = lo + (uintptr_t)i * per;
            if (a >= hi) break;
            const size_t len = std::min<size_t>(per, hi - a);
            th.emplace_back([a, len] { (void)madvise((void*)a, len, 23 /* MADV_POPULATE_WRITE */); });
        }
    }
    ~Prefault() {
        for (auto& t : th) t.join();
    }
};

// nodata (host, one value per column of q) / fill_index / out_n_valid: the masked call; nodata == null: no mask
int run_host_pipeline(sknnr_index* ix, const Reduction& red, const void* q, long nq, const sknnr_query_opts* o, void* out_dist,
                      void* out_idx, void* out_pred, const double* nodata = nullptr, long fill_index = -1,
                      int64_t* out_n_valid = nullptr) {
    if (ix->stream_open) return fail(SKNNR_ERR_INVALID, "a query stream is open on this handle: end it first");
    HostPipe p;
    Push u(Push::kRows, false, out_idx, out_dist, out_pred, 0);  // (the call is one push of rows)
    u.rows = q;
    int rc = pipe_open(p, ix, o, red, out_dist != nullptr, out_pred != nullptr);
    if (!rc && nodata) {
        HIP_TRY(hipDeviceSynchronize());  // (m_nodata belongs to the workspace)
        HIP_TRY(ix->m_nodata.ensure((size_t)p.d_x));
        HIP_TRY(hipMemcpy(ix->m_nodata.p, nodata, (size_t)p.d_x * sizeof(double), hipMemcpyHostToDevice));
        p.nodata_dev = ix->m_nodata.p;
        p.fill_index = fill_index;
    }
    Prefault pf;  // (joined when the call returns)
    if (!rc && std::getenv("SKNNR_PREFAULT")) {  // (measured: 96 ms without, 115 ms with -- the populate threads take bandwidth the copies need)
        for (int l = 0; l < kLanes; ++l) pf.add(u.out[l], lane_bytes(nq, p.lane[l].cols, p.lane[l].esz));
    }
    if (!rc) rc = pipe_submit_rows(p, pipe_adopt(p, u), nq);
    if (!rc) rc = pipe_flush(p);
    if (rc) pipe_fail(p, rc);
    if (out_n_valid) *out_n_valid = p.o.row_offset - p.row_offset0;
    return rc;
}

// X=None (the query rows are the handle's own reference rows, already on the device): only the results
// travel.  Runs on the default stream, chunk by chunk.
int run_self_rows(sknnr_index* ix, const Reduction& red, long nq, const sknnr_query_opts* o, double* out_dist, long* out_idx,
                  double* out_pred) {
    hipStream_t st = nullptr;
    const int k = o->n_neighbors, pc = red.cols(ix->t);
    for (long c0 = 0; c0 < nq; c0 += kChunkRows) {
        const long n = std::min<long>(kChunkRows, nq - c0);
        HIP_TRY(ix->dist_stage.ensure((size_t)n * k));
        HIP_TRY(ix->idx_stage.ensure((size_t)n * k));
        if (out_pred) HIP_TRY(ix->pred_stage.ensure((size_t)n * pc));
        sknnr_query_opts oc = *o;
        oc.row_offset = o->row_offset + c0;
        int rc = search_tile(ix, red, nullptr, n, &oc, ix->dist_stage.p, ix->idx_stage.p, out_pred ? ix->pred_stage.p : nullptr, false, st);
        if (rc) return rc;
        if (out_pred)
            HIP_TRY(hipMemcpyAsync(out_pred + c0 * pc, ix->pred_stage.p, (size_t)n * pc * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out_dist)
            HIP_TRY(hipMemcpyAsync(out_dist + c0 * k, ix->dist_stage.p, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out_idx)
            HIP_TRY(hipMemcpyAsync(out_idx + c0 * k, ix->idx_stage.p, (size_t)n * k * sizeof(long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SKNNR_OK;
}

}  // namespace

// ----------------------------------------------------------------------------------------
// the forest map alone
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_forest_apply(sknnr_index* ix, const void* q, int64_t nq, int32_t query_dtype, int32_t mem,
                                  double* out_ids) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_forest_apply");
    if (!ix->has_forest) return fail(SKNNR_ERR_INVALID, "sknnr_forest_apply needs sknnr_index_set_forest first");
    if (query_dtype < 0 || query_dtype >= kDtypeCount) return fail(SKNNR_ERR_INVALID, "unknown query_dtype %d", query_dtype);
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (nq == 0) return SKNNR_OK;
    if (!q || !out_ids) return fail(SKNNR_ERR_INVALID, "q / out_ids is NULL");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // (the default stream: calls of the handle on other streams are done first)
    DevBuf<int> status;
    HIP_TRY(status.ensure(1));
    HIP_TRY(hipMemset(status.p, 0, sizeof(int)));
    const size_t row_bytes = (size_t)ix->f_d_in * dtype_bytes(query_dtype);
    if (mem == SKNNR_MEM_DEVICE) {
        HIP_TRY(launch::forest_apply(forest_args(ix, q, nq, query_dtype, out_ids, status.p), nullptr));
    } else {
        const long chunk = forest_chunk_rows(ix->d);
        const long cap = std::min<long>(chunk, nq);
        DevBuf<char> dq;
        DevBuf<double> dout;
        HIP_TRY(dq.ensure((size_t)cap * row_bytes));
        HIP_TRY(dout.ensure((size_t)cap * ix->d));
        for (long c0 = 0; c0 < nq; c0 += chunk) {
            const long n = std::min(chunk, nq - c0);
            HIP_TRY(hipMemcpy(dq.p, (const char*)q + (size_t)c0 * row_bytes, (size_t)n * row_bytes, hipMemcpyHostToDevice));
            HIP_TRY(launch::forest_apply(forest_args(ix, dq.p, n, query_dtype, dout.p, status.p), nullptr));
            HIP_TRY(hipMemcpy(out_ids + (size_t)c0 * ix->d, dout.p, (size_t)n * ix->d * sizeof(double), hipMemcpyDeviceToHost));
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    int bits = 0;
    HIP_TRY(hipMemcpy(&bits, status.p, sizeof bits, hipMemcpyDeviceToHost));
    return bits ? nonfinite_error(bits) : SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// kneighbors
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_kneighbors(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o,
                                double* out_dist, int64_t* out_idx, int32_t mem, void* stream) {
    int rc = validate_call(ix, q, nq, o, out_idx);
    if (rc) return rc;
    if (nq == 0) return SKNNR_OK;
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    if (mem == SKNNR_MEM_DEVICE) return run_device(ix, q, nq, o, out_dist, (long*)out_idx, (hipStream_t)stream);
    if (q) return run_host_pipeline(ix, Reduction{}, q, nq, o, out_dist, out_idx, nullptr);  // (out_pred is null: never read)
    return run_self_rows(ix, Reduction{}, nq, o, out_dist, (long*)out_idx, nullptr);
}

// ----------------------------------------------------------------------------------------
// leave-group-out neighbours (groups.hip.h)
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_index_set_groups(sknnr_index* ix, const int32_t* codes, int64_t n) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_index_set_groups");
    if (!codes) {  // clear
        std::lock_guard<std::mutex> lock(ix->mtx);
        ix->has_groups = false;
        ix->g_largest = ix->g_count = 0;
        ix->b_excl_valid = false;
        return SKNNR_OK;
    }
    if (n != ix->n_ref) return fail(SKNNR_ERR_INVALID, "codes must hold one group code per reference row (%ld), got %ld", ix->n_ref, (long)n);
    std::vector<int32_t> sorted(codes, codes + n);
    std::sort(sorted.begin(), sorted.end());
    if (n > 0 && sorted[0] < 0) return fail(SKNNR_ERR_INVALID, "group codes must be >= 0, got %d", (int)sorted[0]);
    long largest = 0, count = 0;
    for (int64_t i = 0; i < n;) {
        int64_t j = i;
        while (j < n && sorted[j] == sorted[i]) ++j;
        largest = std::max<long>(largest, j - i);
        ++count;
        i = j;
    }
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // (a grouped call on another stream may still read the codes held so far)
    HIP_TRY(ix->g_codes.ensure((size_t)n));
    HIP_TRY(hipMemcpy(ix->g_codes.p, codes, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    ix->g_largest = largest;
    ix->g_count = count;
    ix->has_groups = true;
    ix->b_excl_valid = false;
    return SKNNR_OK;
}

extern "C" int sknnr_index_set_buffer(sknnr_index* ix, const double* coords, int64_t n, int32_t c, double radius) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_index_set_buffer");
    if (!coords) {  // clear
        std::lock_guard<std::mutex> lock(ix->mtx);
        ix->has_buffer = false;
        ix->b_cols = 0;
        ix->b_radius = ix->b_r2 = 0.0;
        ix->b_excl_valid = false;
        return SKNNR_OK;
    }
    if (n != ix->n_ref) return fail(SKNNR_ERR_INVALID, "coords must hold one position per reference row (%ld), got %ld", ix->n_ref, (long)n);
    if (c < 1 || c > kPosCols) return fail(SKNNR_ERR_INVALID, "positions have 1 to %d columns, got %d", kPosCols, (int)c);
    if (!std::isfinite(radius) || radius < 0.0) return fail(SKNNR_ERR_INVALID, "radius must be finite and >= 0, got %g", radius);
    // (3, n) column-major like refT; a missing column is +0.0 for every row
    std::vector<double> pos((size_t)kPosCols * (size_t)n, 0.0);
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < c; ++j) {
            const double v = coords[i * c + j];
            if (!std::isfinite(v)) return fail(SKNNR_ERR_INVALID, "positions must be finite, got %g at row %ld, column %d", v, (long)i, j);
            pos[(size_t)j * (size_t)n + (size_t)i] = v;
        }
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // (a grouped call on another stream may still read the positions held so far)
    HIP_TRY(ix->b_pos.ensure(pos.size()));
    HIP_TRY(hipMemcpy(ix->b_pos.p, pos.data(), pos.size() * sizeof(double), hipMemcpyHostToDevice));
    ix->b_cols = c;
    ix->b_radius = radius;
    ix->b_r2 = radius * radius;
    ix->has_buffer = true;
    ix->b_excl_valid = false;
    return SKNNR_OK;
}

namespace {

// excluded[] under the masks now set, counted by buffer_count_kernel once per change of either mask: b_excl on the
// device, its extremes on the host.  Synchronous (the counts come back for the extremes); the caller holds the lock.
int ensure_excluded(sknnr_index* ix) {
    if (ix->b_excl_valid) return SKNNR_OK;
    const long n = ix->n_ref;
    HIP_TRY(ix->b_excl.ensure((size_t)n));
    BufferCountArgs a{};
    a.pos = ix->has_buffer ? ix->b_pos.p : nullptr;
    a.codes = ix->has_groups ? ix->g_codes.p : nullptr;
    a.r2 = ix->b_r2;
    a.n_ref = n;
    a.out = ix->b_excl.p;
    HIP_TRY(launch::buffer_count(a, nullptr));
    std::vector<unsigned long long> h((size_t)n);
    HIP_TRY(hipMemcpy(h.data(), ix->b_excl.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    long mx = 0, mn = n, arg = 0;
    for (long i = 0; i < n; ++i) {
        const long v = (long)h[(size_t)i];
        if (v > mx) mx = v, arg = i;
        mn = std::min(mn, v);
    }
    const BufferCountGrid g = buffer_count_grid(n);
    ix->b_max = mx;
    ix->b_min = mn;
    ix->b_argmax = arg;
    ix->b_count_wg = g.row_blocks * g.splits;
    ix->b_excl_valid = true;
    return SKNNR_OK;
}

// Device-resident core of sknnr_kneighbors_grouped: reference rows [o->row_offset, + nq), outputs on the device.  One
// launch: passes of kGroupNq rows, one workgroup each, taken grid-stride by at most kScanGridWg workgroups; never sliced.
// The masks set on the handle (groups, buffer, both) pick the instantiation.
int run_grouped_device(sknnr_index* ix, long nq, const sknnr_query_opts* o, double* d_dist, long* d_idx, hipStream_t st) {
    zero_records(ix);
    const int mask = (ix->has_groups ? kMaskGroups : 0) | (ix->has_buffer ? kMaskBuffer : 0);
    // (every accepted call fits: the LDS grows with min(d, kScanColChunk) and k <= kScanMaxKK only)
    static_assert(group_scan_bytes(kScanColChunk, kScanMaxKK, kMaskGroups) <= kLdsLimit &&
                      group_scan_bytes(kScanColChunk, kScanMaxKK, kMaskBoth) <= kLdsLimit,
                  "the widest grouped call fits a workgroup's LDS, the positions of a buffered one included");
    const size_t sh = group_scan_bytes(ix->d, o->n_neighbors, mask);
    if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));  // (the staged outputs of host calls are workspace)
    GroupScanArgs a{};
    a.s = make_select_args(ix, o, o->n_neighbors, nullptr, nq, d_dist, d_idx);
    a.refT = ix->refT.p;
    a.codes = ix->has_groups ? ix->g_codes.p : nullptr;
    a.pos = ix->has_buffer ? ix->b_pos.p : nullptr;
    a.r2 = ix->b_r2;
    sknnr_index::CallTiming& ct = ix->timing[ix->timing_next];
    ix->timing_next = (ix->timing_next + 1) % sknnr_index::kTimingRing;
    resolve_call(ix, ct);
    if (!ct.e0) {
        HIP_TRY(hipEventCreate(&ct.e0));
        HIP_TRY(hipEventCreate(&ct.e1));
    }
    ct.coarse_used = 0;
    ct.coarse_rows = 0;
    HIP_TRY(hipEventRecord(ct.e0, st));
    const long passes = (nq + kGroupNq - 1) / kGroupNq;
    const long blocks = std::max<long>(1, std::min<long>(passes, kScanGridWg));
    const int64_t rec[8] = {o->formula + 1, o->n_neighbors, blocks, (int64_t)sh, nq, 1, ix->g_largest, ix->g_count};
    std::copy(std::begin(rec), std::end(rec), ix->last.grouped);
    // (groups alone are never counted by a search call: their record shows the largest group as max(excluded))
    const bool counted = ix->b_excl_valid;
    const int64_t brec[8] = {mask, ix->has_buffer ? ix->b_cols : 0, counted ? ix->b_max : ix->g_largest, counted ? ix->b_min : 0,
                             counted ? ix->b_count_wg : 0, counted ? (int64_t)kCountLdsBytes : 0, counted ? ix->b_argmax : 0, 0};
    std::copy(std::begin(brec), std::end(brec), ix->last.buffer);
    const bool chunked = ix->d > kScanColChunk;  // wide rows: in column chunks
    if (mask == kMaskGroups) HIP_TRY(launch::group_scan(o->formula, chunked, a, blocks, sh, st));
    else HIP_TRY(launch::buffer_scan(mask, o->formula, chunked, a, blocks, sh, st));
    HIP_TRY(hipEventRecord(ct.e1, st));
    ct.pending = true;
    HIP_TRY(hipEventRecord(ix->ev_ws, st));
    ix->ws_busy = true;
    ix->stats.queries += nq;
    ix->stats.exact_only_queries += nq;
    return SKNNR_OK;
}

}  // namespace

extern "C" int sknnr_kneighbors_grouped(sknnr_index* ix, int64_t nq, const sknnr_query_opts* o, double* out_dist,
                                        int64_t* out_idx, int32_t mem, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_kneighbors_grouped");
    if (!o) return fail(SKNNR_ERR_INVALID, "opts is NULL");
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (!out_idx && nq > 0) return fail(SKNNR_ERR_INVALID, "out_idx is NULL");
    if (o->n_neighbors <= 0) return fail(SKNNR_ERR_INVALID, "Expected n_neighbors > 0. Got %d", o->n_neighbors);
    if (!o->exclude_self) return fail(SKNNR_ERR_INVALID, "the rows of a grouped search are reference rows: exclude_self must be 1");
    if (o->apply_affine || o->query_dtype != SKNNR_DTYPE_F64)
        return fail(SKNNR_ERR_INVALID, "a grouped search reads the handle's own rows: apply_affine and query_dtype must be 0");
    if (o->formula != SKNNR_FORMULA_EXPANDED && o->formula != SKNNR_FORMULA_DIRECT && o->formula != SKNNR_FORMULA_HAMMING)
        return fail(SKNNR_ERR_INVALID, "unknown formula %d", o->formula);
    if (o->formula == SKNNR_FORMULA_HAMMING && !ix->has_hw)
        return fail(SKNNR_ERR_INVALID, "formula = HAMMING needs sknnr_index_set_hamming_weights first");
    if (std::abs(o->decimals) > 300) return fail(SKNNR_ERR_INVALID, "decimals out of range");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (!ix->has_groups && !ix->has_buffer) return fail(SKNNR_ERR_INVALID, "sknnr_kneighbors_grouped needs sknnr_index_set_groups first");
    const long n_fit = ix->n_ref;
    if (o->row_offset < 0 || o->row_offset + nq > n_fit)
        return fail(SKNNR_ERR_INVALID, "grouped query rows [%ld, %ld) outside the %ld reference rows", (long)o->row_offset,
                    (long)(o->row_offset + nq), n_fit);
    if (!ix->has_buffer) {  // max(excluded) is the largest group
        if (o->n_neighbors > n_fit - ix->g_largest)
            return fail(SKNNR_ERR_K_TOO_LARGE,
                        "Expected n_neighbors <= n_samples_fit - largest group, but n_neighbors = %d, n_samples_fit = %ld, largest group = %ld",
                        o->n_neighbors, n_fit, ix->g_largest);
    } else {
        HIP_TRY(hipSetDevice(ix->device));
        int rc = ensure_excluded(ix);
        if (rc) return rc;
        if (o->n_neighbors > n_fit - ix->b_max)
            return fail(SKNNR_ERR_K_TOO_LARGE,
                        "Expected n_neighbors <= n_samples_fit - max(excluded), but n_neighbors = %d, n_samples_fit = %ld, "
                        "max(excluded) = %ld (row %ld)",
                        o->n_neighbors, n_fit, ix->b_max, ix->b_argmax);
    }
    if (o->n_neighbors > kScanMaxKK)
        return fail(SKNNR_ERR_UNSUPPORTED, "n_neighbors = %d exceeds the HIP backend's limit of %d%s", o->n_neighbors, kScanMaxKK, "");
    if (nq == 0) return SKNNR_OK;
    HIP_TRY(hipSetDevice(ix->device));
    if (mem == SKNNR_MEM_DEVICE) return run_grouped_device(ix, nq, o, out_dist, (long*)out_idx, (hipStream_t)stream);
    hipStream_t st = nullptr;
    const int k = o->n_neighbors;
    for (long c0 = 0; c0 < nq; c0 += kChunkRows) {
        const long n = std::min<long>(kChunkRows, nq - c0);
        if (out_dist) HIP_TRY(ix->dist_stage.ensure((size_t)n * k));
        HIP_TRY(ix->idx_stage.ensure((size_t)n * k));
        sknnr_query_opts oc = *o;
        oc.row_offset = o->row_offset + c0;
        int rc = run_grouped_device(ix, n, &oc, out_dist ? ix->dist_stage.p : nullptr, ix->idx_stage.p, st);
        if (rc) return rc;
        if (out_dist)
            HIP_TRY(hipMemcpyAsync(out_dist + c0 * k, ix->dist_stage.p, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx + c0 * k, ix->idx_stage.p, (size_t)n * k * sizeof(long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SKNNR_OK;
}

extern "C" int sknnr_buffer_counts(sknnr_index* ix, int64_t* out, int32_t mem, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_buffer_counts");
    if (!out) return fail(SKNNR_ERR_INVALID, "out is NULL");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (!ix->has_groups && !ix->has_buffer)
        return fail(SKNNR_ERR_INVALID, "sknnr_buffer_counts needs sknnr_index_set_buffer or sknnr_index_set_groups first");
    HIP_TRY(hipSetDevice(ix->device));
    int rc = ensure_excluded(ix);
    if (rc) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "excluded[] is copied out as it is");
    const size_t bytes = (size_t)ix->n_ref * sizeof(int64_t);
    if (mem == SKNNR_MEM_DEVICE) HIP_TRY(hipMemcpyAsync(out, ix->b_excl.p, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else HIP_TRY(hipMemcpy(out, ix->b_excl.p, bytes, hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// nodata rows: the mask alone, and the masked calls
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_mask_rows(const void* q, int64_t nq, int32_t d_in, int32_t query_dtype, const double* nodata,
                               int32_t device, int32_t mem, void* stream, uint8_t* out_valid, int64_t* out_n_valid) {
    if (query_dtype < 0 || query_dtype >= kDtypeCount) return fail(SKNNR_ERR_INVALID, "unknown query_dtype %d", query_dtype);
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (d_in < 1 || d_in > kMaskMaxCols) return fail(SKNNR_ERR_INVALID, "d_in = %d outside [1, %d]", d_in, kMaskMaxCols);
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 rows in one call");
    if (!nodata) return fail(SKNNR_ERR_INVALID, "nodata is NULL");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    if (nq == 0) {
        if (out_n_valid) *out_n_valid = 0;
        return SKNNR_OK;
    }
    if (!q || !out_valid) return fail(SKNNR_ERR_INVALID, "q / out_valid is NULL");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr;
    const size_t row_bytes = (size_t)d_in * dtype_bytes(query_dtype);
    DevBuf<double> nd;
    DevBuf<int> blk;
    DevBuf<long> nv;
    Staged<char> dq;
    Staged<unsigned char> dvalid;
    HIP_TRY(nd.ensure((size_t)d_in));
    HIP_TRY(blk.ensure((size_t)mask_blocks(nq)));
    HIP_TRY(nv.ensure(1));
    HIP_TRY(hipMemcpy(nd.p, nodata, (size_t)d_in * sizeof(double), hipMemcpyHostToDevice));
    int rc;
    if ((rc = dq.stage(q, (size_t)nq * row_bytes, mem, kStageIn)) || (rc = dvalid.stage(out_valid, (size_t)nq, mem, kStageOut)))
        return rc;
    MaskArgs a{};
    a.x = dq.p;
    a.valid = dvalid.p;
    a.x_dtype = query_dtype;
    a.nq = nq;
    a.d_in = d_in;
    a.nodata = nd.p;
    a.blk = blk.p;
    HIP_TRY(launch::row_mask(a, nv.p, st));
    HIP_TRY(hipStreamSynchronize(st));
    long n_valid = 0;
    HIP_TRY(hipMemcpy(&n_valid, nv.p, sizeof n_valid, hipMemcpyDeviceToHost));
    if (out_n_valid) *out_n_valid = n_valid;
    return dvalid.download();
}

// ----------------------------------------------------------------------------------------
// band-first tiles: the two transpositions alone, on device pointers
// ----------------------------------------------------------------------------------------
static int validate_planes(const void* src, int64_t n, int32_t c, int32_t elem_bytes, int64_t stride, const void* dst) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
        return fail(SKNNR_ERR_INVALID, "elem_bytes = %d: must be 1, 2, 4 or 8", elem_bytes);
    if (n < 0) return fail(SKNNR_ERR_INVALID, "n must be >= 0");
    if (c < 1 || c > kMaskMaxCols) return fail(SKNNR_ERR_INVALID, "c = %d outside [1, %d]", c, kMaskMaxCols);
    if (stride < n) return fail(SKNNR_ERR_INVALID, "the stride between planes (%lld) is below n (%lld)", (long long)stride, (long long)n);
    if (n == 0) return SKNNR_OK;
    if (!src || !dst) return fail(SKNNR_ERR_INVALID, "src / dst is NULL");
    if (n > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels in one call");
    return SKNNR_OK;
}

extern "C" int sknnr_planes_to_rows(const void* src, int64_t n, int32_t c, int32_t elem_bytes, int64_t src_stride, void* dst,
                                    int32_t device, void* stream) {
    int rc = validate_planes(src, n, c, elem_bytes, src_stride, dst);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(device));
    PlanesArgs a{src, dst, n, c, src_stride};
    HIP_TRY(launch::planes_to_rows(a, elem_bytes, (hipStream_t)stream));
    return SKNNR_OK;
}

extern "C" int sknnr_rows_to_planes(const void* src, int64_t n, int32_t c, void* dst, int64_t dst_stride, int32_t device,
                                    void* stream) {
    int rc = validate_planes(src, n, c, 8, dst_stride, dst);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(device));
    PlanesArgs a{src, dst, n, c, dst_stride};
    HIP_TRY(launch::rows_to_planes(a, (hipStream_t)stream));
    return SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// typed outputs: the conversion alone, on device pointers
// ----------------------------------------------------------------------------------------
// `fill` as an element of a narrow output type: an integer inside the type's range, or any float32 value
static bool narrow_fill_ok(int dtype, double fill) {
    if (dtype == SKNNR_DTYPE_F32) return fill != fill || (double)(float)fill == fill;
    double lo, hi;
    switch (dtype) {
        case SKNNR_DTYPE_I16: lo = -32768.0, hi = 32767.0; break;
        case SKNNR_DTYPE_U16: lo = 0.0, hi = 65535.0; break;
        case SKNNR_DTYPE_U8: lo = 0.0, hi = 255.0; break;
        case SKNNR_DTYPE_I32: lo = -2147483648.0, hi = 2147483647.0; break;
        default: return false;
    }
    return fill >= lo && fill <= hi && std::nearbyint(fill) == fill;
}

extern "C" int sknnr_narrow(const void* src, int32_t kind, int64_t n, int32_t c, void* dst, int32_t dst_dtype,
                            int64_t dst_stride, const double* scale, const double* offset, int32_t has_fill, double fill,
                            int32_t device, void* stream, int32_t* out_wide) {
    if (out_wide) *out_wide = 0;
    const int esz = launch::narrow_dst_bytes(kind, dst_dtype);
    if (!esz) return fail(SKNNR_ERR_INVALID, "no conversion of kind %d to sknnr_dtype %d", kind, dst_dtype);
    if (n < 0) return fail(SKNNR_ERR_INVALID, "n must be >= 0");
    if (c < 1 || c > kMaskMaxCols) return fail(SKNNR_ERR_INVALID, "c = %d outside [1, %d]", c, kMaskMaxCols);
    if (dst_stride != 0 && dst_stride < n)
        return fail(SKNNR_ERR_INVALID, "the stride between planes (%lld) is below n (%lld)", (long long)dst_stride, (long long)n);
    if (!scale != !offset) return fail(SKNNR_ERR_INVALID, "scale and offset come together");
    if (kind == kNarrowIndex && (scale || has_fill)) return fail(SKNNR_ERR_INVALID, "indices take no scale / offset and no fill");
    if (has_fill && kind == kNarrowValue && !narrow_fill_ok(dst_dtype, fill))
        return fail(SKNNR_ERR_INVALID, "fill = %.17g is not representable in sknnr_dtype %d", fill, dst_dtype);
    if (n == 0) return SKNNR_OK;
    if (!src || !dst) return fail(SKNNR_ERR_INVALID, "src / dst is NULL");
    if (n > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels in one call");
    HIP_TRY(hipSetDevice(device));
    NarrowArgs a{src, dst, n, c, dst_stride, scale, offset, has_fill != 0, fill};
    const bool wide = narrow_wide_ok(src, dst, esz, n, c, dst_stride);
    HIP_TRY(launch::narrow(a, kind, dst_dtype, wide, (hipStream_t)stream));
    if (out_wide) *out_wide = wide ? 1 : 0;
    return SKNNR_OK;
}

extern "C" int sknnr_narrow_ids(const int64_t* src, int64_t n, int32_t c, const int64_t* table, int64_t n_table,
                                int32_t has_fill, int64_t fill_id, void* dst, int32_t dst_dtype, int64_t dst_stride,
                                int32_t device, void* stream, int32_t* out_wide) {
    if (out_wide) *out_wide = 0;
    const int esz = launch::narrow_dst_bytes(kNarrowIndex, dst_dtype, true);
    if (!esz) return fail(SKNNR_ERR_INVALID, "dst_dtype = %d: ids leave as int64 (0) or int32 (SKNNR_DTYPE_I32)", dst_dtype);
    if (!table) return fail(SKNNR_ERR_INVALID, "table is NULL");
    if (n_table < 1) return fail(SKNNR_ERR_INVALID, "n_table must be >= 1");
    if (n < 0) return fail(SKNNR_ERR_INVALID, "n must be >= 0");
    if (c < 1 || c > kMaskMaxCols) return fail(SKNNR_ERR_INVALID, "c = %d outside [1, %d]", c, kMaskMaxCols);
    if (dst_stride != 0 && dst_stride < n)
        return fail(SKNNR_ERR_INVALID, "the stride between planes (%lld) is below n (%lld)", (long long)dst_stride, (long long)n);
    if (n == 0) return SKNNR_OK;
    if (!src || !dst) return fail(SKNNR_ERR_INVALID, "src / dst is NULL");
    if (n > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels in one call");
    HIP_TRY(hipSetDevice(device));
    NarrowArgs a{src, dst, n, c, dst_stride, nullptr, nullptr, has_fill != 0, 0.0, (const long*)table, (long)fill_id};
    const bool wide = narrow_wide_ok(src, dst, esz, n, c, dst_stride);
    HIP_TRY(launch::narrow(a, kNarrowIndex, dst_dtype, wide, (hipStream_t)stream));
    if (out_wide) *out_wide = wide ? 1 : 0;
    return SKNNR_OK;
}

// what the masked calls add to validate_call
static int validate_masked(const sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o, const double* nodata) {
    if (o->exclude_self) return fail(SKNNR_ERR_INVALID, "a masked call answers the rows it is given: exclude_self is not available");
    if (!q && nq > 0) return fail(SKNNR_ERR_INVALID, "q is NULL");
    if (!nodata) return fail(SKNNR_ERR_INVALID, "nodata is NULL");
    if (query_cols(ix, o) > kMaskMaxCols) return fail(SKNNR_ERR_UNSUPPORTED, "more than %d input columns with a nodata mask", kMaskMaxCols);
    return SKNNR_OK;
}

extern "C" int sknnr_kneighbors_masked(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o,
                                       const double* nodata, int64_t fill_index, double* out_dist, int64_t* out_idx,
                                       int32_t mem, void* stream, int64_t* out_n_valid) {
    static const double dummy_q = 0.0;
    int rc = validate_call(ix, q ? q : &dummy_q, nq, o, out_idx);
    if (!rc) rc = validate_masked(ix, q, nq, o, nodata);
    if (rc) return rc;
    if (out_n_valid) *out_n_valid = 0;
    if (nq == 0) return SKNNR_OK;
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    if (mem == SKNNR_MEM_DEVICE)
        return run_device_masked(ix, Reduction{}, q, nq, o, nodata, fill_index, out_dist, (long*)out_idx, nullptr,
                                 (hipStream_t)stream, out_n_valid);
    return run_host_pipeline(ix, Reduction{}, q, nq, o, out_dist, out_idx, nullptr, nodata, fill_index, out_n_valid);
}

// ----------------------------------------------------------------------------------------
// full weighted-Hamming distance rows (the reference's own choice among exactly tied rows: np.argpartition on the host)
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_hamming_distances(sknnr_index* ix, const double* q, int64_t nq, const int64_t* rows, int64_t n_rows,
                                       double* out, int32_t mem, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->targets_only) return refuse_targets_only("sknnr_hamming_distances");
    if (!ix->has_hw) return fail(SKNNR_ERR_INVALID, "sknnr_hamming_distances needs sknnr_index_set_hamming_weights first");
    if (n_rows < 0 || nq < 0) return fail(SKNNR_ERR_INVALID, "negative row count");
    if (n_rows == 0) return SKNNR_OK;
    if (!out) return fail(SKNNR_ERR_INVALID, "out is NULL");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    const long n_src = q ? nq : ix->n_ref;  // rows that `rows` may name
    if (!rows && n_rows > n_src) return fail(SKNNR_ERR_INVALID, "n_rows = %ld exceeds the %ld query rows", (long)n_rows, n_src);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HammingRowsArgs a{};
    a.refT = ix->refT.p;
    a.d = ix->d;
    a.n_ref = (int)ix->n_ref;
    a.hw = ix->hw.p;
    a.hw_sum = ix->hw_sum;
    if (mem == SKNNR_MEM_DEVICE) {
        a.xq = q ? q : ix->ref64.p;
        a.rows = (const long*)rows;  // (device memory: the caller vouches for the values)
        a.n_rows = n_rows;
        a.out = out;
        HIP_TRY(launch::hamming_distance_rows(a, (hipStream_t)stream));
        return SKNNR_OK;
    }
    for (int64_t i = 0; rows && i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= n_src) return fail(SKNNR_ERR_INVALID, "rows[%ld] = %ld outside [0, %ld)", (long)i, (long)rows[i], n_src);
    // host buffers: the selected rows only travel in, their distance rows out, at most ~256 MB of them at a time
    const long per = std::max<long>(1, std::min<long>(n_rows, (256L << 20) / (8 * std::max<long>(1, ix->n_ref))));
    DevBuf<double> dq, dout;
    DevBuf<long> drows;
    HIP_TRY(dout.ensure((size_t)per * ix->n_ref));
    if (q) HIP_TRY(dq.ensure((size_t)per * ix->d));
    else HIP_TRY(drows.ensure((size_t)per));
    std::vector<double> gathered;
    std::vector<long> sel;
    for (long c0 = 0; c0 < n_rows; c0 += per) {
        const long n = std::min<long>(per, n_rows - c0);
        if (q) {
            gathered.resize((size_t)n * ix->d);
            for (long i = 0; i < n; ++i) {
                const long r = rows ? rows[c0 + i] : c0 + i;
                std::memcpy(&gathered[(size_t)i * ix->d], q + (size_t)r * ix->d, (size_t)ix->d * sizeof(double));
            }
            HIP_TRY(hipMemcpy(dq.p, gathered.data(), gathered.size() * sizeof(double), hipMemcpyHostToDevice));
            a.xq = dq.p;
            a.rows = nullptr;
        } else {
            sel.resize((size_t)n);
            for (long i = 0; i < n; ++i) sel[(size_t)i] = rows ? rows[c0 + i] : c0 + i;
            HIP_TRY(hipMemcpy(drows.p, sel.data(), (size_t)n * sizeof(long), hipMemcpyHostToDevice));
            a.xq = ix->ref64.p;
            a.rows = drows.p;
        }
        a.n_rows = n;
        a.out = dout.p;
        HIP_TRY(launch::hamming_distance_rows(a, nullptr));
        HIP_TRY(hipMemcpy(out + (size_t)c0 * ix->n_ref, dout.p, (size_t)n * ix->n_ref * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// reference-sharded search: per-shard candidates, then the merge
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_shard_candidates(sknnr_index* ix, const double* q, int64_t nq, const sknnr_query_opts* o,
                                      int64_t index_offset, double* out_val, int64_t* out_idx, int32_t mem, void* stream) {
    int rc = validate_call(ix, q, nq, o, out_idx);
    if (rc) return rc;
    if (o->query_dtype != SKNNR_DTYPE_F64) return fail(SKNNR_ERR_UNSUPPORTED, "the sharded entry points take float64 rows (query_dtype = 0)");
    if (uses_forest(ix, o)) return fail(SKNNR_ERR_UNSUPPORTED, "the sharded entry points take node ids: the forest map is not applied there");
    if (!q || o->exclude_self)
        return fail(SKNNR_ERR_INVALID, "shard candidates are searched for given rows: the caller adds the self slot (n_neighbors + 1) and the merge drops it");
    if (!out_val && nq > 0) return fail(SKNNR_ERR_INVALID, "out_val is NULL");
    if (index_offset < 0 || index_offset + ix->n_ref > 0x7fffff00L) return fail(SKNNR_ERR_INVALID, "index_offset out of range");
    if (nq == 0) return SKNNR_OK;
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    // host buffers: one staged round trip (a shard's candidates are an intermediate of a multi-GPU call, not a hot host path)
    const size_t n_el = (size_t)nq * o->n_neighbors;
    const int d_x = o->apply_affine ? ix->d_in : ix->d;
    Staged<double> dq, dv;
    Staged<long> di;
    if ((rc = dq.stage(q, (size_t)nq * d_x, mem, kStageIn)) || (rc = dv.stage(out_val, n_el, mem, kStageOut)) ||
        (rc = di.stage(out_idx, n_el, mem, kStageOut)))
        return rc;
    rc = run_device(ix, dq.p, nq, o, dv.p, di.p, mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr, 1, index_offset);
    if (rc || mem == SKNNR_MEM_DEVICE) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (o->check_finite && (rc = poll_status(ix))) return rc;
    if ((rc = dv.download())) return rc;
    return di.download();
}

namespace {

int merge_shards_formula(sknnr_index* ix, const SelectArgs& call, int n_shards, long nq, hipStream_t st) {
    ScanArgs a{call, ix->refT.p, nullptr, nullptr, ix->slice_v.p, ix->slice_i.p, ix->fail_list2.p, ix->fail_count.p + 2};
    HIP_TRY(launch::scan_merge(call.formula, a, (nq + 3) / 4, scan_merge_bytes(call.kk), 0, n_shards, st));
    // rows whose merged answer is not unique (exact ties that the reference's heap settles by its history): the
    // sequential scan over ALL reference rows of this handle, as for any other tied row
    const size_t sh = scan_block_bytes(call.d, call.kk, call.formula);
    if (sh > kLdsLimit) return fail(SKNNR_ERR_UNSUPPORTED, "n_neighbors = %d with d = %d does not fit the exact scan kernel", call.k, call.d);
    ScanArgs b{call, ix->refT.p, ix->fail_list2.p, ix->fail_count.p + 2, nullptr, nullptr, nullptr, nullptr};
    const bool chunked = call.d > kScanColChunk;
    const int nq_pass = scan_nq(call.formula);
    const long blocks = std::max<long>(1, std::min<long>((nq + nq_pass - 1) / nq_pass, kScanGridWg));
    const int64_t rec[8] = {call.formula + 1, chunked ? 1 : 0, call.kk, blocks, (int64_t)sh, nq, n_shards, 1};
    std::copy(std::begin(rec), std::end(rec), ix->last.scan);
    HIP_TRY(launch::exact_scan(call.formula, chunked, b, blocks, sh, st));
    return SKNNR_OK;
}

// Device-resident core of sknnr_merge_shards.
int merge_shards_device(sknnr_index* ix, const double* xdev, long nq, const sknnr_query_opts* o, int n_shards,
                        const double* shard_val, const long* shard_idx, double* d_dist, long* d_idx, hipStream_t st) {
    // No pre-filter, rescue or integer Hamming pass runs on this path (and fail_count no longer holds the last one's count);
    // the finaliser's and the mask's records stay what the call before left.
    SearchRecords fresh;
    std::copy(std::begin(ix->last.finalize), std::end(ix->last.finalize), fresh.finalize);
    std::copy(std::begin(ix->last.mask), std::end(ix->last.mask), fresh.mask);
    ix->last = fresh;
    const int kk = o->n_neighbors + (o->exclude_self ? 1 : 0);
    const bool affine = o->apply_affine != 0 && xdev != nullptr;
    const bool self_rows = xdev == nullptr;
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 query rows in one call");
    if (affine && ix->ks == 0) return fail(SKNNR_ERR_UNSUPPORTED, "d = %d > 128 with an affine map is outside the HIP envelope", ix->d);
    if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));
    // the transformed rows (the tied rows are re-scanned in them)
    const double* xq_call = self_rows ? ix->ref64.p + o->row_offset * ix->d : xdev;
    if (affine) {
        HIP_TRY(ix->xt.ensure((size_t)nq * ix->d));
        const long chunk = chunk_rows(ix->ks, 2);
        const long cap_pad = pad_rows(std::min(chunk, nq));
        HIP_TRY(ix->qimg.ensure((size_t)(cap_pad / 32) * 2 * ix->ks * 64));
        HIP_TRY(ix->qnc.ensure(cap_pad));
        SearchPlan prep{};  // (the map alone: nothing is searched in these rows' image)
        prep.affine = true;
        prep.check_finite = o->check_finite != 0;
        for (long c0 = 0; c0 < nq; c0 += chunk) {
            const long n = std::min(chunk, nq - c0);
            int rc = launch_prep(ix, prep, xdev + c0 * ix->d_in, n, pad_rows(n), ix->xt.p + c0 * ix->d, st);
            if (rc) return rc;
        }
        xq_call = ix->xt.p;
    }
    const SelectArgs call = make_select_args(ix, o, kk, xq_call, nq, d_dist, d_idx);
    const size_t heaps = (size_t)nq * n_shards * kk;
    HIP_TRY(ix->slice_v.ensure(heaps));
    HIP_TRY(ix->slice_i.ensure(heaps));
    HIP_TRY(ix->fail_list2.ensure((size_t)nq));
    HIP_TRY(hipMemsetAsync(ix->fail_count.p, 0, 16, st));
    HIP_TRY(launch::pack_shards(shard_val, shard_idx, nq, n_shards, kk, ix->slice_v.p, ix->slice_i.p, st));
    int rc = merge_shards_formula(ix, call, n_shards, nq, st);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ix->ev_ws, st));
    ix->ws_busy = true;
    ix->stats.queries += nq;
    ix->stats.exact_only_queries += nq;
    return SKNNR_OK;
}

}  // namespace

extern "C" int sknnr_merge_shards(sknnr_index* ix, const double* q, int64_t nq, const sknnr_query_opts* o, int32_t n_shards,
                                  const double* shard_val, const int64_t* shard_idx, double* out_dist, int64_t* out_idx,
                                  int32_t mem, void* stream) {
    int rc = validate_call(ix, q, nq, o, out_idx);
    if (rc) return rc;
    if (o->query_dtype != SKNNR_DTYPE_F64) return fail(SKNNR_ERR_UNSUPPORTED, "the sharded entry points take float64 rows (query_dtype = 0)");
    if (uses_forest(ix, o)) return fail(SKNNR_ERR_UNSUPPORTED, "the sharded entry points take node ids: the forest map is not applied there");
    if (n_shards < 1 || n_shards > 64) return fail(SKNNR_ERR_INVALID, "n_shards must be in [1, 64], got %d", n_shards);
    if ((!shard_val || !shard_idx) && nq > 0) return fail(SKNNR_ERR_INVALID, "shard candidate arrays are NULL");
    const int kk = o->n_neighbors + (o->exclude_self ? 1 : 0);
    if (kk > kScanSliceMaxKK) return fail(SKNNR_ERR_UNSUPPORTED, "the shard merge serves n_neighbors (+ self) <= %d", kScanSliceMaxKK);
    if (nq == 0) return SKNNR_OK;
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    const size_t n_el = (size_t)nq * o->n_neighbors;
    const int d_x = o->apply_affine ? ix->d_in : ix->d;
    const size_t n_cand = (size_t)nq * n_shards * kk;
    Staged<double> dq, dv, dd;
    Staged<long> dsi, di;
    if ((rc = dq.stage(q, (size_t)nq * d_x, mem, kStageIn)) || (rc = dv.stage(shard_val, n_cand, mem, kStageIn)) ||
        (rc = dsi.stage(shard_idx, n_cand, mem, kStageIn)) || (rc = dd.stage(out_dist, n_el, mem, kStageOut)) ||
        (rc = di.stage(out_idx, n_el, mem, kStageOut)))
        return rc;
    rc = merge_shards_device(ix, dq.p, nq, o, n_shards, dv.p, dsi.p, dd.p, di.p, mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr);
    if (rc || mem == SKNNR_MEM_DEVICE) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (o->check_finite && q && (rc = poll_status(ix))) return rc;
    if ((rc = dd.download())) return rc;
    return di.download();
}

// ----------------------------------------------------------------------------------------
// predict
// ----------------------------------------------------------------------------------------
// A weight_mode: one sknnr_weight_mode in the low byte, flag bits above it.  explicit_ok: SKNNR_WEIGHTS_EXPLICIT (and
// its F32_WEIGHTS flag) allowed.
static bool weight_mode_ok(int mode, bool explicit_ok) {
    const int base = mode & SKNNR_WEIGHTS_BASE_MASK, flags = mode & ~SKNNR_WEIGHTS_BASE_MASK;
    if (flags & ~(SKNNR_WEIGHTS_F32_TARGETS | SKNNR_WEIGHTS_F32_WEIGHTS)) return false;
    if (base == SKNNR_WEIGHTS_EXPLICIT) return explicit_ok;
    return (base == SKNNR_WEIGHTS_UNIFORM || base == SKNNR_WEIGHTS_DISTANCE) && !(flags & SKNNR_WEIGHTS_F32_WEIGHTS);
}

// The distance-weight law of a predicting call: 0 = none (the caller goes on with the checks it always made), 1 = a law
// that may run (explicit base mode, F32_TARGETS at most, the law the handle holds parameters for), else the failure's status.
static int weight_law_check(const sknnr_index* ix, const sknnr_query_opts* o) {
    if (o->weight_law == kLawNone) return 0;
    if (o->weight_law < 0 || o->weight_law >= kLawCount)
        return fail(SKNNR_ERR_INVALID, "unknown weight law %d", o->weight_law);
    if ((o->weight_mode & SKNNR_WEIGHTS_BASE_MASK) != SKNNR_WEIGHTS_EXPLICIT ||
        (o->weight_mode & ~SKNNR_WEIGHTS_BASE_MASK & ~SKNNR_WEIGHTS_F32_TARGETS))
        return fail(SKNNR_ERR_INVALID, "a weight law takes weight mode SKNNR_WEIGHTS_EXPLICIT (with F32_TARGETS at most), got %d",
                    o->weight_mode);
    if (o->weight_law != ix->law_code)
        return fail(SKNNR_ERR_INVALID, "opts->weight_law = %d, but the handle holds the parameters of law %d "
                    "(sknnr_index_set_weight_law_params)", o->weight_law, ix->law_code);
    return 1;
}

extern "C" int sknnr_index_set_weight_law_params(sknnr_index* ix, int32_t law, double p0, double p1) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (law < 0 || law >= kLawCount) return fail(SKNNR_ERR_INVALID, "unknown weight law %d", law);
    if (law != kLawNone && !(std::isfinite(p0) && p0 > 0.0 && std::isfinite(p1)))
        return fail(SKNNR_ERR_INVALID, "weight law %d: p0 must be finite and > 0 and p1 finite (got %g, %g)", law, p0, p1);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (law == ix->law_code && p0 == ix->law_p0 && p1 == ix->law_p1) return SKNNR_OK;
    if (ix->stream_open)
        return fail(SKNNR_ERR_INVALID, "a query stream is open on this handle: its tiles read the weight law's parameters");
    ix->law_code = law;
    ix->law_p0 = law != kLawNone ? p0 : 0.0;
    ix->law_p1 = law != kLawNone ? p1 : 0.0;
    return SKNNR_OK;
}

extern "C" int sknnr_debug_weight_law(int32_t law, double p0, double p1, const double* dist, int64_t n, double* out,
                                      int32_t mem, int32_t device) {
    if (law <= kLawNone || law >= kLawCount) return fail(SKNNR_ERR_INVALID, "unknown weight law %d", law);
    if (n < 0) return fail(SKNNR_ERR_INVALID, "n must be >= 0");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    if (n == 0) return SKNNR_OK;
    if (!dist || !out) return fail(SKNNR_ERR_INVALID, "dist / out is NULL");
    HIP_TRY(hipSetDevice(device));
    WeightLawArgs a{};
    a.n = n;
    a.law = law;
    a.p0 = p0;
    a.p1 = p1;
    Staged<double> dd, dw;
    int rc;
    if ((rc = dd.stage(dist, (size_t)n, mem, kStageIn)) || (rc = dw.stage(out, (size_t)n, mem, kStageOut))) return rc;
    a.dist = dd.p;
    a.w = dw.p;
    HIP_TRY(launch::weight_law(a, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return dw.download();
}

// The fields the predict, plan and summary kernels' arguments share, and the predict kernels' two float32 flags
template <class Args>
static Args reduce_args(const sknnr_index* ix, const double* dist, const long* idx, const double* w, long nq, int k, int mode) {
    Args a{};
    a.y = ix->y64.p;
    a.dist = dist;
    a.idx = idx;
    a.w = w;
    a.nq = nq;
    a.k = k;
    a.t = ix->t;
    a.mode = mode & SKNNR_WEIGHTS_BASE_MASK;
    if constexpr (std::is_same<Args, PredictArgs>::value) {
        a.y32 = (mode & SKNNR_WEIGHTS_F32_TARGETS) ? 1 : 0;
        a.w32 = (mode & SKNNR_WEIGHTS_F32_WEIGHTS) ? 1 : 0;
    }
    return a;
}

// The reduction `red` of one launch's rows.  Mean and per-target statistics: the predict kernels give every column its
// mean unless no column wants it, then the summary kernel overwrites the columns of red.stat.
//
// law (sknnr_weight_law of the call's opts; kLawNone: nothing here changes): the weights are law(dist), written by
// weight_law_kernel into the handle's law_w in front of the reduction, which then is the explicit one on that buffer
// (the F32_TARGETS flag stays).  law_w belongs to the workspace: `st` first waits for the workspace's last user.
static int launch_bootstrap(sknnr_index* ix, const Reduction& red, const double* dist, const long* idx, long nq, int kw,
                            int mode, int law, double* out, const unsigned char* skip, hipStream_t st);
static int launch_predict(sknnr_index* ix, const Reduction& red, const double* dist, const long* idx, const double* w, long nq,
                          int k, int mode, int law, double* out, hipStream_t st, const unsigned char* skip) {
    if (red.kind == kReduceBoot)  // (the k columns are the kw candidates, and nothing below runs)
        return launch_bootstrap(ix, red, dist, idx, nq, k, mode, law, out, skip, st);
    if (law != kLawNone) {
        if (!dist) return fail(SKNNR_ERR_INVALID, "a distance-weight law needs the distances");
        if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));
        HIP_TRY(ix->law_w.ensure((size_t)nq * k));
        WeightLawArgs wa{};
        wa.dist = dist;
        wa.w = ix->law_w.p;
        wa.n = nq * k;
        wa.law = law;
        wa.p0 = ix->law_p0;
        wa.p1 = ix->law_p1;
        HIP_TRY(launch::weight_law(wa, st));
        w = ix->law_w.p;
        mode = SKNNR_WEIGHTS_EXPLICIT | (mode & SKNNR_WEIGHTS_F32_TARGETS);
    }
    const int64_t law_rec[8] = {law, nq, k, law != kLawNone ? 1 : 0, 0, 0, 0, 0};
    std::copy(std::begin(law_rec), std::end(law_rec), ix->last_law);
    if (red.kind == kReducePlan) {
        // An output plan: `out` is (nq, n_out).  The unchanged predict kernels give the plan's `mean` entries their values
        // through the handle's (nq, t) mean_stage -- a workspace buffer, so `st` first waits for the workspace's last user
        // -- and plan_kernel writes every entry.
        const OutputPlan* op = &red.plan;
        const bool means = op->n_mean > 0;
        if (means) {
            if (ix->ws_busy && law == kLawNone) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));
            HIP_TRY(ix->mean_stage.ensure((size_t)nq * ix->t));
            PredictArgs a = reduce_args<PredictArgs>(ix, dist, idx, w, nq, k, mode);
            a.out = ix->mean_stage.p;
            HIP_TRY(launch::predict(a, st));
        }
        PlanArgs a = reduce_args<PlanArgs>(ix, dist, idx, w, nq, k, mode);
        a.cols = op->cols;
        a.codes = op->codes;
        a.param = op->param;
        a.n_out = op->n_out;
        a.mean = means ? ix->mean_stage.p : nullptr;
        a.out = out;
        HIP_TRY(launch::plan(a, st));
        const int64_t prec[8] = {1, k <= kSummarySmallK ? 1 : 2, nq, op->n_out, k, op->n_mean, means ? 1 : 0, 0};
        std::copy(std::begin(prec), std::end(prec), ix->last_plan);
        const int64_t srec[8] = {0, nq, 0, k, means ? 1 : 0, ix->t, mode & SKNNR_WEIGHTS_BASE_MASK, 0};  // (no summary kernel)
        std::copy(std::begin(srec), std::end(srec), ix->last_summary);
        HIP_TRY(hipEventRecord(ix->ev_ws, st));
        ix->ws_busy = true;
        return SKNNR_OK;
    }
    std::fill(std::begin(ix->last_plan), std::end(ix->last_plan), 0);  // (host record only: no plan kernel in this reduction)
    const SummaryPlan* sp = red.kind == kReduceStats ? &red.stat : nullptr;  // (null: all mean)
    const bool means = !sp || sp->n_mean > 0;
    if (means) {
        PredictArgs a = reduce_args<PredictArgs>(ix, dist, idx, w, nq, k, mode);
        a.out = out;
        HIP_TRY(launch::predict(a, st));
    }
    const int nc = sp ? sp->nc : 0;
    if (nc) {
        SummaryArgs a = reduce_args<SummaryArgs>(ix, dist, idx, w, nq, k, mode);
        a.tab = sp->tab;
        a.nc = nc;
        a.out = out;
        HIP_TRY(launch::summary(a, st));
    }
    const int64_t rec[8] = {nc ? (k <= kSummarySmallK ? 1 : 2) : 0, nq, nc, k, means ? 1 : 0, ix->t,
                            mode & SKNNR_WEIGHTS_BASE_MASK, 0};
    std::copy(std::begin(rec), std::end(rec), ix->last_summary);
    // the reduction may read the handle's staging buffers: it is now the workspace's last user
    HIP_TRY(hipEventRecord(ix->ev_ws, st));
    ix->ws_busy = true;
    return SKNNR_OK;
}

// The reduction as a caller hands it over: the kind and the host arrays that belong to it -- (t) codes in `stat` for
// per-target statistics; `cols` / `stat` / `param` of n_out entries for an output plan.
struct ReduceSpec {
    int kind = kReduceMean;
    const int32_t* stat = nullptr;
    const int32_t* cols = nullptr;
    const double* param = nullptr;
    int32_t n_out = 0;
    std::vector<int> tab;  // reduce_check leaves the host image of a statistics table here
};
// The spec checked before any device work; red: its kind and counts, the device pointers still null (reduce_upload).
static int reduce_check(const sknnr_index* ix, ReduceSpec& rs, Reduction& red) {
    red = Reduction{};
    red.kind = rs.kind;
    if (rs.kind == kReduceStats) {  // stat must be given and hold sknnr_statistic codes
        if (!rs.stat) return fail(SKNNR_ERR_INVALID, "stat is NULL");
        int bad = 0;
        if (!summary_table(rs.stat, ix->t, rs.tab, &bad))
            return fail(SKNNR_ERR_INVALID, "stat[%d] = %d is no sknnr_statistic", bad, rs.stat[bad]);
        red.stat.nc = (int)rs.tab.size() / 2;
        red.stat.n_mean = ix->t - red.stat.nc;
    } else if (rs.kind == kReducePlan) {
        if (!rs.cols || !rs.stat || !rs.param) return fail(SKNNR_ERR_INVALID, "cols / stat / param is NULL");
        if (rs.n_out < 1 || rs.n_out > kPlanMaxOut)
            return fail(SKNNR_ERR_INVALID, "n_out = %d outside [1, %d]", rs.n_out, kPlanMaxOut);
        for (int e = 0; e < rs.n_out; ++e) {
            if (rs.cols[e] < 0 || rs.cols[e] >= ix->t)
                return fail(SKNNR_ERR_INVALID, "cols[%d] = %d: the handle has %d targets", e, rs.cols[e], ix->t);
            if (rs.stat[e] < 0 || rs.stat[e] >= kPlanStatCount)
                return fail(SKNNR_ERR_INVALID, "stat[%d] = %d is no sknnr_statistic", e, rs.stat[e]);
            if (rs.stat[e] == kStatQuantile && !(rs.param[e] >= 0.0 && rs.param[e] <= 1.0))
                return fail(SKNNR_ERR_INVALID, "param[%d] = %g: a quantile's q lies in [0, 1]", e, rs.param[e]);
            if (rs.stat[e] == kStatMean) ++red.plan.n_mean;
        }
        red.plan.n_out = rs.n_out;
    }
    return SKNNR_OK;
}
// The checked spec's table or arrays into the buffer of its kind, and red's device pointers: the open stream's s_stat /
// s_plan, or a one-shot call's c_stat / c_plan (reduce_upload_call).  A mean, or a table that is all mean, uploads nothing.
static int reduce_upload(const ReduceSpec& rs, DevBuf<int>& stat_buf, DevBuf<double>& plan_buf, Reduction& red) {
    if (rs.kind == kReduceStats && red.stat.nc) {
        if (int rc = stat_buf.upload(rs.tab.data(), rs.tab.size())) return rc;
        red.stat.tab = stat_buf.p;
    } else if (rs.kind == kReducePlan) {
        const std::vector<double> img = plan_image(rs.cols, rs.stat, rs.param, rs.n_out);
        if (int rc = plan_buf.upload(img.data(), img.size())) return rc;
        red.plan.param = plan_buf.p;
        red.plan.cols = (const int*)(plan_buf.p + rs.n_out);
        red.plan.codes = red.plan.cols + rs.n_out;
    }
    return SKNNR_OK;
}
// A one-shot call's upload.  c_stat and c_plan belong to the workspace: the previous reduction may still read them, so
// wait for the workspace's last user first.
static int reduce_upload_call(sknnr_index* ix, const ReduceSpec& rs, Reduction& red) {
    const bool uploads = rs.kind == kReducePlan || (rs.kind == kReduceStats && red.stat.nc);
    if (uploads && ix->ws_busy) HIP_TRY(hipEventSynchronize(ix->ev_ws));
    return reduce_upload(rs, ix->c_stat, ix->c_plan, red);
}

// sknnr_predict_from_neighbors (a mean), sknnr_summarize_from_neighbors (per-target statistics) and
// sknnr_summarize_plan_from_neighbors (an output plan: out_pred is (nq, n_out))
static int reduce_from_neighbors(sknnr_index* ix, const double* dist, const int64_t* idx, const double* w, int64_t nq,
                                 int32_t k, int32_t mode, ReduceSpec rs, double* out_pred, int32_t mem, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->t < 1) return fail(SKNNR_ERR_NO_TARGETS, "the index was created without targets");
    Reduction red;
    if (const int rc = reduce_check(ix, rs, red)) return rc;
    if (nq < 0 || k < 1 || !idx || !out_pred) return fail(SKNNR_ERR_INVALID, "bad argument");
    if (!weight_mode_ok(mode, true)) return fail(SKNNR_ERR_INVALID, "unknown weight mode %d", mode);
    if ((mode & SKNNR_WEIGHTS_BASE_MASK) == SKNNR_WEIGHTS_DISTANCE && !dist)
        return fail(SKNNR_ERR_INVALID, "distance weights need dist");
    if ((mode & SKNNR_WEIGHTS_BASE_MASK) == SKNNR_WEIGHTS_EXPLICIT && !w)
        return fail(SKNNR_ERR_INVALID, "explicit weights need w");
    if (k > kScanMaxKK)  // the reduction follows numpy's pairwise sum up to this many terms
        return fail(SKNNR_ERR_UNSUPPORTED, "k = %d exceeds the HIP backend's limit of %d", k, kScanMaxKK);
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    if (nq == 0) return SKNNR_OK;
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    if (const int rc = reduce_upload_call(ix, rs, red)) return rc;
    hipStream_t st = mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr;
    const size_t n_el = (size_t)nq * k;
    Staged<long> di;
    Staged<double> dd, dw, dout;
    int rc;
    if ((rc = di.stage(idx, n_el, mem, kStageIn)) || (rc = dout.stage(out_pred, (size_t)nq * red.cols(ix->t), mem, kStageOut)) ||
        (rc = dd.stage(dist, n_el, mem, kStageIn)) || (rc = dw.stage(w, n_el, mem, kStageIn)))
        return rc;
    if ((rc = launch_predict(ix, red, dd.p, di.p, dw.p, nq, k, mode, kLawNone, dout.p, st))) return rc;
    return dout.download();
}

extern "C" int sknnr_predict_from_neighbors(sknnr_index* ix, const double* dist, const int64_t* idx, const double* w,
                                            int64_t nq, int32_t k, int32_t mode, double* out_pred, int32_t mem,
                                            void* stream) {
    return reduce_from_neighbors(ix, dist, idx, w, nq, k, mode, ReduceSpec{}, out_pred, mem, stream);
}

extern "C" int sknnr_summarize_from_neighbors(sknnr_index* ix, const double* dist, const int64_t* idx, const double* w,
                                              int64_t nq, int32_t k, int32_t mode, const int32_t* stat, double* out,
                                              int32_t mem, void* stream) {
    return reduce_from_neighbors(ix, dist, idx, w, nq, k, mode, ReduceSpec{kReduceStats, stat}, out, mem, stream);
}

extern "C" int sknnr_summarize_plan_from_neighbors(sknnr_index* ix, const double* dist, const int64_t* idx, const double* w,
                                                   int64_t nq, int32_t k, int32_t mode, const int32_t* cols,
                                                   const int32_t* stat, const double* param, int32_t n_out, double* out,
                                                   int32_t mem, void* stream) {
    return reduce_from_neighbors(ix, dist, idx, w, nq, k, mode, ReduceSpec{kReducePlan, stat, cols, param, n_out}, out, mem, stream);
}

// sknnr_predict (a mean), sknnr_summarize (per-target statistics) and sknnr_summarize_plan (an output plan: out_pred is
// (nq, n_out))
static int search_and_reduce(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o, ReduceSpec rs,
                             double* out_pred, double* out_dist, int64_t* out_idx, int32_t mem, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->t < 1) return fail(SKNNR_ERR_NO_TARGETS, "the index was created without targets");
    Reduction red;
    if (const int rc0 = reduce_check(ix, rs, red)) return rc0;
    if (!o) return fail(SKNNR_ERR_INVALID, "opts is NULL");
    if (!out_pred && nq > 0) return fail(SKNNR_ERR_INVALID, "out_pred is NULL");
    const int law = weight_law_check(ix, o);
    if (law < 0) return law;
    if (!law) {
        if ((o->weight_mode & SKNNR_WEIGHTS_BASE_MASK) == SKNNR_WEIGHTS_EXPLICIT)
            return fail(SKNNR_ERR_INVALID, "explicit weights go through sknnr_predict_from_neighbors");
        if (!weight_mode_ok(o->weight_mode, false))
            return fail(SKNNR_ERR_INVALID, "unknown weight mode %d", o->weight_mode);
    }
    static int64_t dummy_idx;
    int rc = validate_call(ix, q, nq, o, out_idx ? out_idx : &dummy_idx);
    if (rc) return rc;
    if (nq == 0) return SKNNR_OK;
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    const int k = o->n_neighbors;
    if ((rc = reduce_upload_call(ix, rs, red))) return rc;

    if (mem == SKNNR_MEM_DEVICE) {
        hipStream_t st = (hipStream_t)stream;
        double* dd = out_dist;
        long* di = (long*)out_idx;
        if (!dd || !di) {
            // the staging buffers below belong to the workspace: wait for its previous user first
            if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));
        }
        if (!dd) {
            HIP_TRY(ix->dist_stage.ensure((size_t)nq * k));
            dd = ix->dist_stage.p;
        }
        if (!di) {
            HIP_TRY(ix->idx_stage.ensure((size_t)nq * k));
            di = ix->idx_stage.p;
        }
        return search_tile(ix, red, q, nq, o, dd, di, out_pred, false, st);
    }
    if (q) return run_host_pipeline(ix, red, q, nq, o, out_dist, out_idx, out_pred);
    return run_self_rows(ix, red, nq, o, out_dist, (long*)out_idx, out_pred);
}

extern "C" int sknnr_predict(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o, double* out_pred,
                             double* out_dist, int64_t* out_idx, int32_t mem, void* stream) {
    return search_and_reduce(ix, q, nq, o, ReduceSpec{}, out_pred, out_dist, out_idx, mem, stream);
}

extern "C" int sknnr_summarize(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o, const int32_t* stat,
                               double* out, double* out_dist, int64_t* out_idx, int32_t mem, void* stream) {
    return search_and_reduce(ix, q, nq, o, ReduceSpec{kReduceStats, stat}, out, out_dist, out_idx, mem, stream);
}

extern "C" int sknnr_summarize_plan(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o,
                                    const int32_t* cols, const int32_t* stat, const double* param, int32_t n_out, double* out,
                                    double* out_dist, int64_t* out_idx, int32_t mem, void* stream) {
    return search_and_reduce(ix, q, nq, o, ReduceSpec{kReducePlan, stat, cols, param, n_out}, out, out_dist, out_idx, mem, stream);
}

extern "C" int sknnr_predict_masked(sknnr_index* ix, const void* q, int64_t nq, const sknnr_query_opts* o,
                                    const double* nodata, int64_t fill_index, double* out_pred, double* out_dist,
                                    int64_t* out_idx, int32_t mem, void* stream, int64_t* out_n_valid) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (ix->t < 1) return fail(SKNNR_ERR_NO_TARGETS, "the index was created without targets");
    if (!o) return fail(SKNNR_ERR_INVALID, "opts is NULL");
    if (!out_pred && nq > 0) return fail(SKNNR_ERR_INVALID, "out_pred is NULL");
    const int law = weight_law_check(ix, o);
    if (law < 0) return law;
    if (!law && !weight_mode_ok(o->weight_mode, false))
        return fail(SKNNR_ERR_INVALID, "a masked call predicts with uniform or distance weights only (weight mode %d)", o->weight_mode);
    static int64_t dummy_idx;
    static const double dummy_q = 0.0;
    int rc = validate_call(ix, q ? q : &dummy_q, nq, o, out_idx ? out_idx : &dummy_idx);
    if (!rc) rc = validate_masked(ix, q, nq, o, nodata);
    if (rc) return rc;
    if (out_n_valid) *out_n_valid = 0;
    if (nq == 0) return SKNNR_OK;
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    if (mem == SKNNR_MEM_DEVICE)
        return run_device_masked(ix, Reduction{}, q, nq, o, nodata, fill_index, out_dist, (long*)out_idx, out_pred,
                                 (hipStream_t)stream, out_n_valid);
    return run_host_pipeline(ix, Reduction{}, q, nq, o, out_dist, out_idx, out_pred, nodata, fill_index, out_n_valid);
}

// ----------------------------------------------------------------------------------------
// streamed query tiles (raster ingestion)
// ----------------------------------------------------------------------------------------
struct sknnr_stream {
    HostPipe pipe;
    int64_t rows_pushed = 0;
    bool pushed = false;  // a push was accepted: the nodata mask can no longer change
    // What the caller named for the next push (which products the stream carries: pipe.prod).  A zonal stream: the zone
    // codes (sknnr_stream_next_zones), the stream's own copy.  A domain stream: the caller's code plane
    // (sknnr_stream_next_domain_out).
    struct {
        std::vector<int32_t> zones;
        bool have_zones = false;
        uint8_t* domain_out = nullptr;
        int64_t domain_out_n = 0;
    } next;
};

// What every collecting entry of a stream does behind its own refusals: takes the handle's lock (held through `lock` when
// this returns), flushes the pipeline and waits for the stream the tiles' launches ran on; the copies are the caller's.
static int collect_begin(HostPipe& p, std::unique_lock<std::mutex>& lock) {
    lock = std::unique_lock<std::mutex>(p.ix->mtx);
    HIP_TRY(hipSetDevice(p.ix->device));
    const int rc = pipe_flush(p);
    if (rc) return pipe_fail(p, rc);
    HIP_TRY(hipStreamSynchronize(p.ix->st_run));
    return SKNNR_OK;
}

extern "C" int sknnr_stream_set_nodata(sknnr_stream* s, const double* nodata, int64_t fill_index) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    if (!nodata) return fail(SKNNR_ERR_INVALID, "nodata is NULL");
    HostPipe& p = s->pipe;
    if (p.replay.on)
        return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_nodata: a replay stream has no feature rows to mask; its mask is the fill index of sknnr_replay_begin");
    std::lock_guard<std::mutex> lock(p.ix->mtx);
    if (s->pushed) return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_nodata is allowed only before the first push");
    if (p.d_x > kMaskMaxCols) return fail(SKNNR_ERR_UNSUPPORTED, "more than %d input columns with a nodata mask", kMaskMaxCols);
    HIP_TRY(hipSetDevice(p.ix->device));
    if (int rc = p.ix->s_nodata.upload(nodata, (size_t)p.d_x)) return rc;
    p.nodata_dev = p.ix->s_nodata.p;
    p.fill_index = fill_index;
    return SKNNR_OK;
}

// The stream's reduction stage refuses what a setter would add, or nothing (SKNNR_OK).  own: the kind the setter installs
// (the same kind again replaces the stage), or kReduceMean for a setter of another stage, which only a bootstrap excludes.
static int stage_refusal(const HostPipe& p, int own, const char* what) {
    static const char* const has[] = {nullptr, "per-target statistics (sknnr_stream_set_statistics)",
                                      "an output plan (sknnr_stream_set_plan)", "a bootstrap stage (sknnr_stream_set_bootstrap)"};
    const int kind = p.red.kind;
    if (kind == kReduceMean || kind == own || (own == kReduceMean && kind != kReduceBoot)) return SKNNR_OK;
    return fail(SKNNR_ERR_INVALID, "the stream has %s: it takes no %s", has[kind], what);
}

// What every setter of a stage or a side product does behind its own argument checks: takes the handle's lock (held
// through `lock` when this returns), refuses after the first push under the entry's name, asks the reduction stage
// (stage_refusal with the setter's kind and label) and selects the device.
static int setter_begin(sknnr_stream* s, std::unique_lock<std::mutex>& lock, const char* entry, int own, const char* what) {
    lock = std::unique_lock<std::mutex>(s->pipe.ix->mtx);
    if (s->pushed) return fail(SKNNR_ERR_INVALID, "%s is allowed only before the first push", entry);
    if (int no = stage_refusal(s->pipe, own, what)) return no;
    HIP_TRY(hipSetDevice(s->pipe.ix->device));
    return SKNNR_OK;
}

extern "C" int sknnr_stream_set_statistics(sknnr_stream* s, const int32_t* stat, int32_t t) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    if (!p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without predictions");
    if (t != p.t) return fail(SKNNR_ERR_INVALID, "t = %d: the handle has %d targets", t, p.t);
    ReduceSpec rs{kReduceStats, stat};
    Reduction red;
    int rc = reduce_check(p.ix, rs, red);
    if (rc) return rc;
    std::unique_lock<std::mutex> lock;
    if ((rc = setter_begin(s, lock, "sknnr_stream_set_statistics", kReduceStats, "per-target statistics"))) return rc;
    if ((rc = reduce_upload(rs, p.ix->s_stat, p.ix->s_plan, red))) return rc;
    p.red = red;  // (an all-mean table: the stream enqueues what it did without one, and still takes no other stage)
    return SKNNR_OK;
}

extern "C" int sknnr_stream_set_plan(sknnr_stream* s, const int32_t* cols, const int32_t* stat, const double* param,
                                     int32_t n_out) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    if (!p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without predictions");
    ReduceSpec rs{kReducePlan, stat, cols, param, n_out};
    Reduction red;
    int rc = reduce_check(p.ix, rs, red);
    if (rc) return rc;
    std::unique_lock<std::mutex> lock;
    if ((rc = setter_begin(s, lock, "sknnr_stream_set_plan", kReducePlan, "output plan"))) return rc;
    if (p.prod.zonal) return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_plan comes before sknnr_stream_set_zonal: n_classes holds one value per output plane");
    if (p.lane[kLanePred].scale)
        return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_plan comes before sknnr_stream_set_output: the scale / offset hold one value per output plane");
    if ((rc = reduce_upload(rs, p.ix->s_stat, p.ix->s_plan, red))) return rc;
    p.red = red;
    p.lane[kLanePred].cols = n_out;  // from now on the prediction lane is n_out wide
    return SKNNR_OK;
}

extern "C" int sknnr_stream_set_output(sknnr_stream* s, int32_t idx_dtype, int32_t dist_dtype, int32_t pred_dtype,
                                       const double* pred_scale, const double* pred_offset, int32_t has_pred_fill,
                                       double pred_fill) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    if (idx_dtype != SKNNR_DTYPE_F64 && idx_dtype != SKNNR_DTYPE_I32)
        return fail(SKNNR_ERR_INVALID, "idx_dtype = %d: indices leave as int64 (0) or int32 (SKNNR_DTYPE_I32)", idx_dtype);
    if (dist_dtype != SKNNR_DTYPE_F64 && dist_dtype != SKNNR_DTYPE_F32)
        return fail(SKNNR_ERR_INVALID, "dist_dtype = %d: distances leave as float64 (0) or float32 (SKNNR_DTYPE_F32)", dist_dtype);
    if (pred_dtype < SKNNR_DTYPE_F64 || pred_dtype > SKNNR_DTYPE_I32)
        return fail(SKNNR_ERR_INVALID, "pred_dtype = %d is no sknnr_dtype", pred_dtype);
    if (!pred_scale != !pred_offset) return fail(SKNNR_ERR_INVALID, "pred_scale and pred_offset come together");
    if (pred_dtype == SKNNR_DTYPE_F64 && (pred_scale || has_pred_fill))
        return fail(SKNNR_ERR_INVALID, "a scale / offset or a fill needs a narrow pred_dtype");
    if (has_pred_fill && !narrow_fill_ok(pred_dtype, pred_fill))
        return fail(SKNNR_ERR_INVALID, "pred_fill = %.17g is not representable in pred_dtype %d", pred_fill, pred_dtype);
    HostPipe& p = s->pipe;
    if (dist_dtype && !p.lane[kLaneDist].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without distances");
    if (pred_dtype && !p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without predictions");
    std::lock_guard<std::mutex> lock(p.ix->mtx);
    if (s->pushed) return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_output is allowed only before the first push");
    HostPipe::Lane& pl = p.lane[kLanePred];
    pl.scale = pl.offset = nullptr;
    if (pred_scale) {
        HIP_TRY(hipSetDevice(p.ix->device));
        const size_t pc = (size_t)p.lane[kLanePred].cols;  // (one value per output plane: the plan's entries, or the targets)
        if (int rc = p.ix->s_scale.upload(pred_scale, pc)) return rc;
        if (int rc = p.ix->s_offset.upload(pred_offset, pc)) return rc;
        pl.scale = p.ix->s_scale.p;
        pl.offset = p.ix->s_offset.p;
    }
    const int32_t dtype[kLanes] = {idx_dtype, dist_dtype, pred_dtype};  // (lane order)
    for (int l = 0; l < kLanes; ++l) {
        p.lane[l].dtype = dtype[l];
        p.lane[l].esz = (size_t)dtype_bytes(dtype[l]);
    }
    pl.has_fill = has_pred_fill != 0;
    pl.fill = pred_fill;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_set_id_table(sknnr_stream* s, const int64_t* table, int64_t n_table, int64_t fill_id) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    if (!table) return fail(SKNNR_ERR_INVALID, "table is NULL");
    HostPipe& p = s->pipe;
    if (n_table != p.ix->n_ref)
        return fail(SKNNR_ERR_INVALID, "n_table = %lld: the handle has %lld reference rows", (long long)n_table, (long long)p.ix->n_ref);
    std::lock_guard<std::mutex> lock(p.ix->mtx);
    if (s->pushed) return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_id_table is allowed only before the first push");
    HIP_TRY(hipSetDevice(p.ix->device));
    if (int rc = p.ix->s_id_table.upload(table, (size_t)n_table)) return rc;
    HostPipe::Lane& il = p.lane[kLaneIdx];
    il.table = p.ix->s_id_table.p;
    il.has_fill = 1;  // (every negative index of a tile is the nodata expansion's fill_index)
    il.fill_id = fill_id;
    return SKNNR_OK;
}

// ---- neighbour usage (tally.hip.h) ------------------------------------------------------------------------------------
// One launch into cnt / maxbits on `st`; `half`: the device record's words it adds to (0 one-shot calls, 1 the open stream).
static int launch_tally(sknnr_index* ix, const double* dist, const long* idx, long n, int k, unsigned long long* cnt,
                        unsigned long long* maxbits, int half, hipStream_t st) {
    TallyArgs a{};
    a.idx = idx;
    a.dist = maxbits ? dist : nullptr;
    a.n = n;
    a.k = k;
    a.n_ref = ix->n_ref;
    a.cnt = cnt;
    a.maxbits = maxbits;
    a.rec = ix->tally.rec.at(half);
    HIP_TRY(launch::tally(a, st));
    return SKNNR_OK;
}

static int tally_tile(sknnr_index* ix, const double* dist, const long* idx, long n, int k, hipStream_t st) {
    if (!dist) return fail(SKNNR_ERR_INVALID, "a tallied tile needs its distances");
    const int rc = launch_tally(ix, dist, idx, n, k, ix->tally.stream.cnt.p, ix->tally.stream.max.p, 1, st);
    if (rc) return rc;
    ix->tally.rec.ran(1, n);
    ix->tally.rec.host[2] = k;
    return SKNNR_OK;
}

static int tally_check_shape(const sknnr_index* ix, int32_t k) {
    if (k < 1) return fail(SKNNR_ERR_INVALID, "k must be >= 1");
    if ((double)ix->n_ref * (double)k >= 4294967296.0)
        return fail(SKNNR_ERR_UNSUPPORTED, "n_ref * k = %lld * %d does not fit the tally's 32-bit keys", (long long)ix->n_ref, k);
    return SKNNR_OK;
}

extern "C" int sknnr_tally_from_neighbors(sknnr_index* ix, const double* dist, const int64_t* idx, int64_t nq, int32_t k,
                                          int64_t* counts, double* max_dist, int32_t accumulate, int32_t mem, void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    int rc = tally_check_shape(ix, k);
    if (rc) return rc;
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 rows in one call");
    if (!counts) return fail(SKNNR_ERR_INVALID, "counts is NULL");
    if (!idx && nq > 0) return fail(SKNNR_ERR_INVALID, "idx is NULL");
    if (!dist != !max_dist) return fail(SKNNR_ERR_INVALID, "dist and max_dist come together (both NULL: counts only)");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    const size_t n_cnt = (size_t)ix->n_ref * k, n_max = (size_t)ix->n_ref, n_el = (size_t)nq * k;
    hipStream_t st = mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr;
    HIP_TRY(ix->tally.rec.ensure());
    HIP_TRY(ix->tally.rec.reset(0, st, {nq > 0 ? 1 : 0, nq, k}));
    // (int64 counts and float64 maxima ARE the accumulators: the same 8-byte patterns)
    const int acc_dir = accumulate ? kStageInOut : kStageOut;
    Staged<long> di;
    Staged<double> dd;
    Staged<unsigned long long> cnt, mx;
    if ((rc = di.stage(idx, n_el, mem, kStageIn)) || (rc = dd.stage(dist, n_el, mem, kStageIn)) ||
        (rc = cnt.stage(counts, n_cnt, mem, acc_dir)) || (rc = mx.stage(max_dist, n_max, mem, acc_dir)))
        return rc;
    if (!accumulate) {
        HIP_TRY(hipMemsetAsync(cnt.p, 0, n_cnt * 8, st));
        if (mx.p) HIP_TRY(hipMemsetAsync(mx.p, 0, n_max * 8, st));
    } else if (mx.p) {
        HIP_TRY(launch::tally_clean((double*)mx.p, (long)n_max, st));
    }
    if ((rc = launch_tally(ix, dd.p, di.p, nq, k, cnt.p, mx.p, 0, st))) return rc;
    if (mem == SKNNR_MEM_HOST) HIP_TRY(hipStreamSynchronize(st));
    if ((rc = cnt.download())) return rc;
    return mx.download();
}

extern "C" int sknnr_stream_set_tally(sknnr_stream* s) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    const int rc = tally_check_shape(ix, p.k);
    if (rc) return rc;
    if (p.replay.on && p.replay.dist_kind == kReplayDistNone)
        return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_tally: the replay stream was opened without stored distances, and the tally keeps their maxima");
    std::unique_lock<std::mutex> lock;
    if (int no = setter_begin(s, lock, "sknnr_stream_set_tally", kReduceMean, "usage tally")) return no;
    const size_t n_cnt = (size_t)ix->n_ref * p.k, n_max = (size_t)ix->n_ref;
    auto& ts = ix->tally.stream;
    HIP_TRY(ts.cnt.ensure(n_cnt));
    HIP_TRY(ts.max.ensure(n_max));
    HIP_TRY(ix->tally.rec.ensure());
    // (on the stream every tile's tally runs on: zeroed in front of the first of them)
    HIP_TRY(hipMemsetAsync(ts.cnt.p, 0, n_cnt * 8, ix->st_run));
    HIP_TRY(hipMemsetAsync(ts.max.p, 0, n_max * 8, ix->st_run));
    HIP_TRY(ix->tally.rec.reset(1, ix->st_run, {0, 0, p.k}));
    p.prod.tally = true;
    p.mask_dist = true;  // the masked path keeps the search's distances whether or not they leave
    return SKNNR_OK;
}

extern "C" int sknnr_stream_get_tally(sknnr_stream* s, int64_t* counts, double* max_dist) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    if (!p.prod.tally) return fail(SKNNR_ERR_INVALID, "the stream tallies nothing: sknnr_stream_set_tally was not called");
    if (!counts && !max_dist) return fail(SKNNR_ERR_INVALID, "counts and max_dist are both NULL");
    std::unique_lock<std::mutex> lock;
    if (const int rc = collect_begin(p, lock)) return rc;
    if (counts) HIP_TRY(hipMemcpy(counts, ix->tally.stream.cnt.p, (size_t)ix->n_ref * p.k * 8, hipMemcpyDeviceToHost));
    if (max_dist) HIP_TRY(hipMemcpy(max_dist, ix->tally.stream.max.p, (size_t)ix->n_ref * 8, hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_tally(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    unsigned long long w[kTallyRecWords];
    if (const int rc = ix->tally.rec.read(ix->mtx, ix->device, out, w)) return rc;
    out[7] = kTallySlots;
    out[3] = (int64_t)w[kTallyRecTallied];
    out[4] = (int64_t)w[kTallyRecSkipped];
    out[5] = (int64_t)w[kTallyRecAtomics];
    out[6] = (int64_t)w[kTallyRecOverflow];
    return SKNNR_OK;
}

// ---- zonal statistics (zonal.hip.h) -----------------------------------------------------------------------------------
// One launch into acc / hist on `st`; cls / off: the class table on the device (null: no class planes); `half`: the device
// record's words it adds to (0 one-shot calls, 1 the open stream).
static int launch_zonal(sknnr_index* ix, const ZonalSpec& z, const double* v, const int32_t* zones, long n, const int* cls,
                        const long* off, long long* acc, long long* hist, int half, hipStream_t st) {
    ZonalArgs a{};
    a.v = v;
    a.zones = zones;
    a.n = n;
    a.c = z.c;
    a.n_zones = z.n_zones;
    a.na.scale = z.scale;
    a.na.offset = z.offset;
    a.n_classes = z.classes ? cls : nullptr;
    a.hist_off = z.classes ? off : nullptr;
    a.acc = acc;
    a.hist = z.classes ? hist : nullptr;
    a.rec = ix->zonal.rec.at(half);
    HIP_TRY(launch::zonal(a, z.dtype, st));
    return SKNNR_OK;
}

static int zonal_tile(sknnr_index* ix, const ZonalSpec& z, const double* pred, const int32_t* zones, long n, hipStream_t st) {
    if (!pred || !zones) return fail(SKNNR_ERR_INVALID, "a zonal tile needs its predictions and its zone codes");
    const auto& zs = ix->zonal.stream;
    const int rc = launch_zonal(ix, z, pred, zones, n, zs.cls.p, zs.off.p, zs.acc.p, zs.hist.p, 1, st);
    if (rc) return rc;
    ix->zonal.rec.ran(1, n);
    ix->zonal.rec.host[2] = z.c;
    return SKNNR_OK;
}

// The two refusals and the class table: off[j] where column j's block begins in hist, *n_hist its length in all.
static int zonal_check_shape(int64_t n_zones, int32_t c, const int32_t* n_classes, std::vector<long>& off, size_t* n_hist) {
    if (n_zones < 1) return fail(SKNNR_ERR_INVALID, "n_zones must be >= 1");
    if (c < 1) return fail(SKNNR_ERR_INVALID, "c must be >= 1");
    if ((double)n_zones * (double)c >= 4294967296.0)
        return fail(SKNNR_ERR_UNSUPPORTED, "n_zones * c = %lld * %d does not fit the zonal kernel's 32-bit keys", (long long)n_zones, c);
    if (n_zones > 0x7fffffffL)
        return fail(SKNNR_ERR_UNSUPPORTED, "n_zones = %lld: zone codes are int32", (long long)n_zones);
    off.assign((size_t)c, 0);
    *n_hist = 0;
    if (!n_classes) return SKNNR_OK;
    for (int j = 0; j < c; ++j) {
        if (n_classes[j] < 0) return fail(SKNNR_ERR_INVALID, "n_classes[%d] = %d is negative", j, n_classes[j]);
        if ((double)n_zones * (double)n_classes[j] >= 4294967296.0)
            return fail(SKNNR_ERR_UNSUPPORTED, "n_zones * n_classes[%d] = %lld * %d does not fit the zonal kernel's 32-bit keys", j,
                        (long long)n_zones, n_classes[j]);
        off[(size_t)j] = (long)*n_hist;
        *n_hist += (size_t)n_zones * (size_t)n_classes[j];
    }
    return SKNNR_OK;
}

extern "C" int sknnr_zonal_from_values(sknnr_index* ix, const double* values, const int32_t* zones, int64_t n, int32_t c,
                                       int32_t dst_dtype, const double* scale, const double* offset, int64_t n_zones,
                                       const int32_t* n_classes, int64_t* acc, int64_t* hist, int32_t accumulate, int32_t mem,
                                       void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    std::vector<long> off;
    size_t n_hist = 0;
    int rc = zonal_check_shape(n_zones, c, n_classes, off, &n_hist);
    if (rc) return rc;
    if (n < 0) return fail(SKNNR_ERR_INVALID, "n must be >= 0");
    if (n > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels in one call");
    if (dst_dtype < SKNNR_DTYPE_I16 || dst_dtype > SKNNR_DTYPE_I32)
        return fail(SKNNR_ERR_INVALID, "dst_dtype = %d: zonal sums are over stored integers (SKNNR_DTYPE_I16 / U16 / U8 / I32)", dst_dtype);
    if (!scale != !offset) return fail(SKNNR_ERR_INVALID, "scale and offset come together");
    if (!acc) return fail(SKNNR_ERR_INVALID, "acc is NULL");
    if (n_hist > 0 && !hist) return fail(SKNNR_ERR_INVALID, "hist is NULL and a column has classes");
    if (n > 0 && (!values || !zones)) return fail(SKNNR_ERR_INVALID, "values / zones is NULL");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr;
    const size_t n_acc = (size_t)n_zones * c * kZonalFields, n_el = (size_t)n * c;
    const bool classes = n_hist > 0;
    // the handle's parameter buffers: an earlier call on `st` may still read them
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(ix->zonal.rec.ensure());
    auto& zc = ix->zonal.call;
    ZonalSpec z{(int)n_zones, c, dst_dtype, nullptr, nullptr, classes};
    if (scale) {
        HIP_TRY(zc.par.ensure(2 * (size_t)c));
        HIP_TRY(hipMemcpy(zc.par.p, scale, (size_t)c * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(zc.par.p + c, offset, (size_t)c * sizeof(double), hipMemcpyHostToDevice));
        z.scale = zc.par.p;
        z.offset = zc.par.p + c;
    }
    if (classes && ((rc = zc.cls.upload(n_classes, (size_t)c)) || (rc = zc.off.upload(off.data(), (size_t)c)))) return rc;
    HIP_TRY(ix->zonal.rec.reset(0, st, {n > 0 ? 1 : 0, n, c}));
    const int acc_dir = accumulate ? kStageInOut : kStageOut;
    Staged<double> dv;
    Staged<int32_t> dz;
    Staged<long long> da, dh;
    if ((rc = dv.stage(values, n_el, mem, kStageIn)) || (rc = dz.stage(zones, (size_t)n, mem, kStageIn)) ||
        (rc = da.stage(acc, n_acc, mem, acc_dir)) || (rc = dh.stage(classes ? hist : nullptr, n_hist, mem, acc_dir)))
        return rc;
    if (!accumulate) {
        HIP_TRY(launch::zonal_init(da.p, (long)((size_t)n_zones * c), st));
        if (classes) HIP_TRY(hipMemsetAsync(dh.p, 0, n_hist * 8, st));
    }
    if ((rc = launch_zonal(ix, z, dv.p, dz.p, n, zc.cls.p, zc.off.p, da.p, dh.p, 0, st))) return rc;
    if (mem == SKNNR_MEM_HOST) HIP_TRY(hipStreamSynchronize(st));
    if ((rc = da.download())) return rc;
    return dh.download();
}

extern "C" int sknnr_stream_set_zonal(sknnr_stream* s, int64_t n_zones, const int32_t* n_classes) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    if (!p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without predictions");
    const int c = p.lane[kLanePred].cols;  // (the plan's entries, or the targets)
    std::vector<long> off;
    size_t n_hist = 0;
    const int rc = zonal_check_shape(n_zones, c, n_classes, off, &n_hist);
    if (rc) return rc;
    std::unique_lock<std::mutex> lock;
    if (int no = setter_begin(s, lock, "sknnr_stream_set_zonal", kReduceMean, "zonal statistics")) return no;
    const size_t n_keys = (size_t)n_zones * c;
    auto& zs = ix->zonal.stream;
    HIP_TRY(zs.acc.ensure(n_keys * kZonalFields));
    HIP_TRY(zs.hist.ensure(n_hist));
    HIP_TRY(ix->zonal.rec.ensure());
    if (n_hist) {
        if (int no = zs.cls.upload(n_classes, (size_t)c)) return no;
        if (int no = zs.off.upload(off.data(), (size_t)c)) return no;
    }
    // (on the stream every tile's launch runs on: initialised in front of the first of them)
    HIP_TRY(launch::zonal_init(zs.acc.p, (long)n_keys, ix->st_run));
    if (n_hist) HIP_TRY(hipMemsetAsync(zs.hist.p, 0, n_hist * 8, ix->st_run));
    HIP_TRY(ix->zonal.rec.reset(1, ix->st_run, {0, 0, c}));
    p.prod.zonal = true;
    p.prod.zonal_zones = (int)n_zones;
    p.prod.zonal_c = c;
    p.prod.zonal_hist = n_hist;
    s->next.have_zones = false;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_next_zones(sknnr_stream* s, const int32_t* zones, int64_t nq) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    if (!s->pipe.prod.zonal) return fail(SKNNR_ERR_INVALID, "the stream has no zones: sknnr_stream_set_zonal was not called");
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (nq == 0) return SKNNR_OK;  // (a push of no rows takes none)
    if (!zones) return fail(SKNNR_ERR_INVALID, "zones is NULL");
    std::lock_guard<std::mutex> lock(s->pipe.ix->mtx);
    s->next.zones.assign(zones, zones + nq);
    s->next.have_zones = true;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_get_zonal(sknnr_stream* s, int64_t* acc, int64_t* hist) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    if (!p.prod.zonal) return fail(SKNNR_ERR_INVALID, "the stream has no zones: sknnr_stream_set_zonal was not called");
    if (!acc && !hist) return fail(SKNNR_ERR_INVALID, "acc and hist are both NULL");
    if (hist && !p.prod.zonal_hist) return fail(SKNNR_ERR_INVALID, "hist is given and no column has classes");
    std::unique_lock<std::mutex> lock;
    if (const int rc = collect_begin(p, lock)) return rc;
    const auto& zs = ix->zonal.stream;
    if (acc) HIP_TRY(hipMemcpy(acc, zs.acc.p, (size_t)p.prod.zonal_zones * p.prod.zonal_c * kZonalFields * 8, hipMemcpyDeviceToHost));
    if (hist) HIP_TRY(hipMemcpy(hist, zs.hist.p, p.prod.zonal_hist * 8, hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_zonal(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    unsigned long long w[kZonalRecWords];
    if (const int rc = ix->zonal.rec.read(ix->mtx, ix->device, out, w)) return rc;
    // (eight words: the sixth counter, entries without a slot, does not fit; they show in the atomics)
    out[3] = (int64_t)w[kZonalRecTallied];
    out[4] = (int64_t)w[kZonalRecNan];
    out[5] = (int64_t)w[kZonalRecOutside];
    out[6] = (int64_t)w[kZonalRecOther];
    out[7] = (int64_t)w[kZonalRecAtomics];
    return SKNNR_OK;
}

extern "C" int sknnr_debug_zonal_geometry(int32_t c, int64_t out[4]) {
    if (!out || c < 1) return fail(SKNNR_ERR_INVALID, "bad argument");
    out[0] = zonal_pixels_per_wg(c);
    out[1] = kZonalSlots;
    out[2] = kZonalHistSlots;
    out[3] = kZonalProbes;
    return SKNNR_OK;
}

// ---- distance domain (domain.hip.h) -----------------------------------------------------------------------------------
// One launch into codes / acc on `st`; `half`: the device record's words it adds to (0 one-shot calls, 1 the open stream).
static int launch_domain(sknnr_index* ix, const DomainSpec& d, const double* table, const double* dist, long n, int k,
                         uint8_t* codes, unsigned long long* acc, double* pred, int pred_cols, int half, hipStream_t st) {
    DomainArgs a{};
    a.dist = dist;
    a.n = n;
    a.k = k;
    a.rank0 = d.rank0;
    a.table = table;
    a.m = d.m;
    a.has_threshold = d.has_threshold;
    a.threshold = d.threshold;
    a.codes = codes;
    a.acc = acc;
    a.pred = pred;
    a.pred_cols = pred_cols;
    a.rec = ix->domain.rec.at(half);
    HIP_TRY(launch::domain(a, st));
    return SKNNR_OK;
}

static int domain_tile(sknnr_index* ix, const DomainSpec& d, const double* dist, long n, int k, uint8_t* codes, double* pred,
                       int pred_cols, hipStream_t st) {
    if (!dist) return fail(SKNNR_ERR_INVALID, "a domain tile needs its distances");
    const auto& ds = ix->domain.stream;
    const int rc = launch_domain(ix, d, ds.table.p, dist, n, k, codes, ds.acc.p, pred, pred_cols, 1, st);
    if (rc) return rc;
    ix->domain.rec.ran(1, n);
    return SKNNR_OK;
}

// The contract's refusals, all on the host: the table, the rank against k, the threshold.
static int domain_check(const double* table, int64_t m, int32_t k, int32_t rank, int32_t has_threshold, double threshold) {
    if (k < 1) return fail(SKNNR_ERR_INVALID, "k must be >= 1");
    if (rank < 1 || rank > k) return fail(SKNNR_ERR_INVALID, "rank = %d outside [1, k = %d]", rank, k);
    if (!table) return fail(SKNNR_ERR_INVALID, "table is NULL");
    if (m < 1 || m > 0x7fffffffL) return fail(SKNNR_ERR_INVALID, "m = %lld outside [1, 2^31 - 1]", (long long)m);
    if (has_threshold && !(std::isfinite(threshold) && threshold >= 0.0))
        return fail(SKNNR_ERR_INVALID, "the threshold must be finite and >= 0");
    for (int64_t j = 0; j < m; ++j) {
        if (!(std::isfinite(table[j]) && table[j] >= 0.0))
            return fail(SKNNR_ERR_INVALID, "table[%lld] is not a finite value >= 0", (long long)j);
        if (j > 0 && table[j] < table[j - 1])
            return fail(SKNNR_ERR_INVALID, "the table is not sorted: table[%lld] < table[%lld]", (long long)j, (long long)(j - 1));
    }
    return SKNNR_OK;
}

extern "C" int sknnr_domain_from_neighbors(sknnr_index* ix, const double* dist, int64_t nq, int32_t k, int32_t rank,
                                           const double* table, int64_t m, int32_t has_threshold, double threshold,
                                           uint8_t* codes, int64_t* acc, int32_t accumulate, int32_t mem, void* stream) {
    // (the contract's own refusals first: they need no handle)
    int rc = domain_check(table, m, k, rank, has_threshold, threshold);
    if (rc) return rc;
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels in one call");
    if (!acc) return fail(SKNNR_ERR_INVALID, "acc is NULL");
    if (!dist && nq > 0) return fail(SKNNR_ERR_INVALID, "dist is NULL");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr;
    // the handle's table: an earlier call on `st` may still read it
    HIP_TRY(hipStreamSynchronize(st));
    DevBuf<double>& dtable = ix->domain.call.table;
    if ((rc = dtable.upload(table, (size_t)m))) return rc;
    HIP_TRY(ix->domain.rec.ensure());
    HIP_TRY(ix->domain.rec.reset(0, st, {nq > 0 ? 1 : 0, nq, k, rank, m}));
    const DomainSpec d{rank - 1, (long)m, has_threshold != 0, threshold};
    Staged<double> dd;
    Staged<uint8_t> dc;
    Staged<unsigned long long> da;  // (int64 counters ARE the accumulators: the same 8-byte patterns)
    if ((rc = dd.stage(dist, (size_t)nq * k, mem, kStageIn)) || (rc = dc.stage(codes, (size_t)nq, mem, kStageOut)) ||
        (rc = da.stage(acc, kDomainAcc, mem, accumulate ? kStageInOut : kStageOut)))
        return rc;
    if (!accumulate) HIP_TRY(hipMemsetAsync(da.p, 0, kDomainAcc * 8, st));
    if ((rc = launch_domain(ix, d, dtable.p, dd.p, nq, k, dc.p, da.p, nullptr, 0, 0, st))) return rc;
    if (mem == SKNNR_MEM_HOST) HIP_TRY(hipStreamSynchronize(st));
    if ((rc = da.download())) return rc;
    return dc.download();
}

extern "C" int sknnr_stream_set_domain(sknnr_stream* s, const double* table, int64_t m, int32_t rank, int32_t has_threshold,
                                       double threshold, int32_t mask_beyond) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    const int rc = domain_check(table, m, p.k, rank, has_threshold, threshold);
    if (rc) return rc;
    if (mask_beyond && !has_threshold) return fail(SKNNR_ERR_INVALID, "mask_beyond needs a threshold");
    if (mask_beyond && !p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "mask_beyond: the stream was opened without predictions");
    if (p.replay.on && p.replay.dist_kind == kReplayDistNone)
        return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_domain: the replay stream was opened without stored distances");
    std::unique_lock<std::mutex> lock;
    if (int no = setter_begin(s, lock, "sknnr_stream_set_domain", kReduceMean, "distance domain")) return no;
    auto& ds = ix->domain.stream;
    if (int no = ds.table.upload(table, (size_t)m)) return no;
    HIP_TRY(ds.acc.ensure(kDomainAcc));
    HIP_TRY(ix->domain.rec.ensure());
    // (on the stream every tile's launch runs on: zeroed in front of the first of them)
    HIP_TRY(hipMemsetAsync(ds.acc.p, 0, kDomainAcc * 8, ix->st_run));
    HIP_TRY(ix->domain.rec.reset(1, ix->st_run, {0, 0, p.k, rank, m}));
    p.prod.domain = true;
    p.prod.domain_mask = mask_beyond != 0;
    p.prod.domain_spec = DomainSpec{rank - 1, (long)m, has_threshold != 0, threshold};
    p.mask_dist = true;  // the masked path keeps the search's distances whether or not they leave
    s->next.domain_out = nullptr;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_next_domain_out(sknnr_stream* s, uint8_t* out, int64_t nq) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    if (!s->pipe.prod.domain) return fail(SKNNR_ERR_INVALID, "the stream has no domain: sknnr_stream_set_domain was not called");
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (nq == 0) return SKNNR_OK;  // (a push of no rows writes none)
    if (!out) return fail(SKNNR_ERR_INVALID, "out is NULL");
    std::lock_guard<std::mutex> lock(s->pipe.ix->mtx);
    s->next.domain_out = out;
    s->next.domain_out_n = nq;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_get_domain(sknnr_stream* s, int64_t acc[103]) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    if (!p.prod.domain) return fail(SKNNR_ERR_INVALID, "the stream has no domain: sknnr_stream_set_domain was not called");
    if (!acc) return fail(SKNNR_ERR_INVALID, "acc is NULL");
    std::unique_lock<std::mutex> lock;
    if (const int rc = collect_begin(p, lock)) return rc;
    HIP_TRY(hipMemcpy(acc, ix->domain.stream.acc.p, kDomainAcc * 8, hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_domain(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    unsigned long long w[kDomainRecWords];
    if (const int rc = ix->domain.rec.read(ix->mtx, ix->device, out, w)) return rc;
    // (the pixels the kernels counted, not the host's: the two agree when every launch ran)
    out[1] = (int64_t)w[kDomainRecPixels];
    out[5] = (int64_t)w[kDomainRecNodata];
    out[6] = (int64_t)w[kDomainRecAtomics];
    out[7] = (int64_t)w[kDomainRecBlanked];
    return SKNNR_OK;
}

extern "C" int sknnr_debug_domain_geometry(int64_t m, int64_t out[4]) {
    if (!out || m < 1 || m > 0x7fffffffL) return fail(SKNNR_ERR_INVALID, "bad argument");
    out[0] = kDomainWgPixels;
    out[1] = kDomainSkel;
    out[2] = domain_stride(m);
    out[3] = domain_skel_entries(m);
    return SKNNR_OK;
}

extern "C" int sknnr_stream_valid_rows(const sknnr_stream* s, int64_t* out_valid_rows) {
    if (!s || !out_valid_rows) return fail(SKNNR_ERR_INVALID, "stream / out_valid_rows is NULL");
    std::lock_guard<std::mutex> lock(s->pipe.ix->mtx);
    *out_valid_rows = s->pipe.o.row_offset - s->pipe.row_offset0;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_begin(sknnr_index* ix, const sknnr_query_opts* o, int32_t want_dist, int32_t want_pred,
                                  sknnr_stream** out) {
    if (!out) return fail(SKNNR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    static int64_t dummy_idx;
    static const double dummy_q = 0.0;
    int rc = validate_call(ix, &dummy_q, 0, o, &dummy_idx);
    if (rc) return rc;
    if (o->exclude_self) return fail(SKNNR_ERR_INVALID, "a stream answers pushed rows: exclude_self is not available");
    if (want_pred) {
        if (ix->t < 1) return fail(SKNNR_ERR_NO_TARGETS, "the index was created without targets");
        const int law = weight_law_check(ix, o);
        if (law < 0) return law;
        if (!law && !weight_mode_ok(o->weight_mode, false))
            return fail(SKNNR_ERR_INVALID, "a stream predicts with uniform or distance weights only");
    }
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (ix->stream_open) return fail(SKNNR_ERR_INVALID, "a query stream is already open on this handle");
    HIP_TRY(hipSetDevice(ix->device));
    sknnr_stream* s = new (std::nothrow) sknnr_stream();
    if (!s) return fail(SKNNR_ERR_INVALID, "out of host memory");
    rc = pipe_open(s->pipe, ix, o, Reduction{}, want_dist != 0, want_pred != 0);
    if (rc) {
        delete s;
        return rc;
    }
    ix->stream_open = true;
    *out = s;
    return SKNNR_OK;
}

static bool stream_typed(const sknnr_stream* s) {
    for (const auto& ln : s->pipe.lane)
        if (ln.dtype) return true;
    return false;
}
static const char* const kTypedStreamMsg =
    "the stream has typed outputs (sknnr_stream_set_output): use sknnr_stream_push_typed / sknnr_stream_push_planes_typed";

// The body of every push of nq pixels.  The entry points name the source, the layout and the caller's output arrays (in
// elements of the stream's type for each lane) and check what is theirs alone; s, nq, the zone codes and the code plane
// named for this push, and the push's number are this function's.
static int stream_push(sknnr_stream* s, Push u, int64_t nq) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    HostPipe& p = s->pipe;
    const bool stored = u.source == Push::kStored;
    if (p.replay.on != stored)
        return fail(SKNNR_ERR_INVALID, stored ? "sknnr_replay_push: the stream was opened by sknnr_stream_begin and takes feature rows"
                                              : "a replay stream takes stored neighbours: use sknnr_replay_push / sknnr_replay_push_planes");
    pipe_adopt(p, u);
    if (nq == 0) return SKNNR_OK;
    // (a replayed push may ask for nothing: its tile still feeds the tally, the zonal tables and the domain)
    if (!stored && !u.out[kLaneIdx] && !u.out[kLanePred]) return fail(SKNNR_ERR_INVALID, "a push needs out_idx or out_pred");
    if (u.out[kLaneDist] && !p.lane[kLaneDist].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without distances");
    if (u.out[kLanePred] && !p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without predictions");
    std::lock_guard<std::mutex> lock(p.ix->mtx);
    if (p.prod.zonal) {
        if (!s->next.have_zones) return fail(SKNNR_ERR_INVALID, "a push on a zonal stream needs sknnr_stream_next_zones first");
        if ((int64_t)s->next.zones.size() != nq)
            return fail(SKNNR_ERR_INVALID, "sknnr_stream_next_zones gave %lld zone codes, the push has %lld rows", (long long)s->next.zones.size(), (long long)nq);
        const int dt = p.lane[kLanePred].dtype;
        if (dt < SKNNR_DTYPE_I16 || dt > SKNNR_DTYPE_I32)
            return fail(SKNNR_ERR_INVALID, "a zonal stream needs an integer pred_dtype (sknnr_stream_set_output): zonal sums are over stored integers");
        s->next.have_zones = false;  // (consumed, whatever becomes of the push)
        u.zones = s->next.zones.data();
    }
    if (p.prod.domain) {
        uint8_t* const dst = s->next.domain_out;
        const int64_t dst_n = s->next.domain_out_n;
        s->next.domain_out = nullptr;  // (consumed, whatever becomes of the push)
        if (dst && dst_n != nq)
            return fail(SKNNR_ERR_INVALID, "sknnr_stream_next_domain_out named %lld codes, the push has %lld rows", (long long)dst_n, (long long)nq);
        u.domain_out = dst;
    }
    HIP_TRY(hipSetDevice(p.ix->device));
    s->pushed = true;
    const int rc = pipe_submit_rows(p, u, nq);
    if (rc) return pipe_fail(p, rc);
    s->rows_pushed += nq;
    return SKNNR_OK;
}

extern "C" int sknnr_stream_push_typed(sknnr_stream* s, const void* q, int64_t nq, void* out_dist, void* out_idx,
                                       void* out_pred) {
    if (s && nq > 0 && !q) return fail(SKNNR_ERR_INVALID, "q is NULL");
    Push u(Push::kRows, false, out_idx, out_dist, out_pred, 0);
    u.rows = q;
    return stream_push(s, u, nq);
}

extern "C" int sknnr_stream_push(sknnr_stream* s, const void* q, int64_t nq, double* out_dist, int64_t* out_idx,
                                 double* out_pred) {
    if (s && stream_typed(s)) return fail(SKNNR_ERR_INVALID, "%s", kTypedStreamMsg);
    return sknnr_stream_push_typed(s, q, nq, out_dist, out_idx, out_pred);
}

extern "C" int sknnr_stream_push_planes_typed(sknnr_stream* s, const void* const* planes, int64_t nq, void* out_dist,
                                              void* out_idx, void* out_pred, int64_t out_stride) {
    if (s && nq > 0) {
        if (!planes) return fail(SKNNR_ERR_INVALID, "planes is NULL");
        const int d_x = s->pipe.d_x;
        for (int j = 0; j < d_x; ++j)
            if (!planes[j]) return fail(SKNNR_ERR_INVALID, "planes[%d] is NULL", j);
        if (out_stride < nq) return fail(SKNNR_ERR_INVALID, "out_stride (%lld) is below nq (%lld)", (long long)out_stride, (long long)nq);
        if (d_x > kMaskMaxCols) return fail(SKNNR_ERR_UNSUPPORTED, "more than %d input columns in a band-first push", kMaskMaxCols);
    }
    Push u(Push::kBands, true, out_idx, out_dist, out_pred, (long)out_stride);
    u.bands = planes;
    return stream_push(s, u, nq);
}

extern "C" int sknnr_stream_push_planes(sknnr_stream* s, const void* const* planes, int64_t nq, double* out_dist,
                                        int64_t* out_idx, double* out_pred, int64_t out_stride) {
    if (s && stream_typed(s)) return fail(SKNNR_ERR_INVALID, "%s", kTypedStreamMsg);
    return sknnr_stream_push_planes_typed(s, planes, nq, out_dist, out_idx, out_pred, out_stride);
}

extern "C" int sknnr_stream_flush(sknnr_stream* s) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    std::lock_guard<std::mutex> lock(s->pipe.ix->mtx);
    HIP_TRY(hipSetDevice(s->pipe.ix->device));
    return pipe_flush(s->pipe);
}

extern "C" int sknnr_stream_end(sknnr_stream* s, int64_t* rows_pushed) {
    if (!s) return SKNNR_OK;
    int rc;
    {
        std::lock_guard<std::mutex> lock(s->pipe.ix->mtx);
        rc = hipSetDevice(s->pipe.ix->device) == hipSuccess ? pipe_flush(s->pipe) : fail(SKNNR_ERR_HIP, "hipSetDevice failed");
        s->pipe.ix->stream_open = false;
    }
    if (rows_pushed) *rows_pushed = s->rows_pushed;
    delete s;
    return rc;
}

// ----------------------------------------------------------------------------------------
// neighbour replay (replay.hip.h): streams whose tiles are stored neighbours
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_index_create_targets(const double* y, int64_t n_ref, int32_t t, int32_t device, sknnr_index** out) {
    if (!out) return fail(SKNNR_ERR_INVALID, "sknnr_index_create_targets: out is NULL");
    *out = nullptr;
    if (!y || n_ref < 1 || t < 1) return fail(SKNNR_ERR_INVALID, "sknnr_index_create_targets: y must be a non-empty (n_ref, t) matrix");
    if (n_ref > 0x7fffff00L) return fail(SKNNR_ERR_UNSUPPORTED, "sknnr_index_create_targets: n_ref = %ld exceeds 2^31 - 256", (long)n_ref);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return fail(SKNNR_ERR_NO_DEVICE, "no HIP device is visible");
    if (device < 0 || device >= n_dev) return fail(SKNNR_ERR_INVALID, "device %d out of range [0, %d)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    sknnr_index* ix = new (std::nothrow) sknnr_index();
    if (!ix) return fail(SKNNR_ERR_INVALID, "out of host memory");
    struct Guard {
        sknnr_index* p;
        ~Guard() { delete p; }
    } guard{ix};
    ix->device = device;
    ix->n_ref = n_ref;
    ix->t = t;
    ix->targets_only = true;
    HIP_TRY(ix->y64.ensure((size_t)n_ref * t));
    HIP_TRY(hipMemcpy(ix->y64.p, y, (size_t)n_ref * t * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipEventCreateWithFlags(&ix->ev_ws, hipEventDisableTiming));
    guard.p = nullptr;
    *out = ix;
    return SKNNR_OK;
}

extern "C" int sknnr_index_set_replay_ids(sknnr_index* ix, const int64_t* ids, int64_t n) {
    // (the table itself is checked first, before the handle is even looked at)
    if (ids && (n < 1 || n > 0x7fffff00L)) return fail(SKNNR_ERR_INVALID, "sknnr_index_set_replay_ids: n = %lld outside [1, 2^31 - 256]", (long long)n);
    std::vector<std::pair<long, int>> tab;
    if (ids) {
        tab.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) tab[(size_t)i] = {(long)ids[i], (int)i};
        std::sort(tab.begin(), tab.end());
        for (size_t i = 1; i < tab.size(); ++i)
            if (tab[i].first == tab[i - 1].first)
                return fail(SKNNR_ERR_INVALID, "sknnr_index_set_replay_ids: id %lld names rows %d and %d: the ids must be unique",
                            (long long)tab[i].first, tab[i - 1].second, tab[i].second);
    }
    if (!ix) return fail(SKNNR_ERR_INVALID, "sknnr_index_set_replay_ids: index is NULL");
    if (ids && n != ix->n_ref)
        return fail(SKNNR_ERR_INVALID, "sknnr_index_set_replay_ids: n = %lld, the handle has %lld reference rows", (long long)n, (long long)ix->n_ref);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (ix->stream_open) return fail(SKNNR_ERR_INVALID, "sknnr_index_set_replay_ids: a stream is open on this handle: end it first");
    ix->r_id_n = 0;
    if (!ids) return SKNNR_OK;
    std::vector<long> sorted(tab.size());
    std::vector<int> perm(tab.size());
    for (size_t i = 0; i < tab.size(); ++i) {
        sorted[i] = tab[i].first;
        perm[i] = tab[i].second;
    }
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(ix->r_id_sorted.ensure(sorted.size()));
    HIP_TRY(ix->r_id_perm.ensure(perm.size()));
    HIP_TRY(hipMemcpy(ix->r_id_sorted.p, sorted.data(), sorted.size() * sizeof(long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ix->r_id_perm.p, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
    ix->r_id_n = (long)n;
    return SKNNR_OK;
}

extern "C" int sknnr_replay_begin(sknnr_index* ix, int32_t k, int32_t ks, int32_t weight_mode, int32_t weight_law,
                                  int32_t idx_dtype, int32_t dist_dtype, int64_t fill_index, int32_t ids, int32_t want_dist,
                                  int32_t want_pred, sknnr_stream** out) {
    if (!out) return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: out is NULL");
    *out = nullptr;
    if (!ix) return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: index is NULL");
    if (ks < 1 || k < 1 || k > ks) return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: k = %d outside [1, ks = %d]", k, ks);
    if (idx_dtype != SKNNR_DTYPE_F64 && idx_dtype != SKNNR_DTYPE_I32)
        return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: idx_dtype = %d: stored indices are int64 (0) or int32 (SKNNR_DTYPE_I32)", idx_dtype);
    if (dist_dtype != SKNNR_REPLAY_NO_DIST && dist_dtype != SKNNR_DTYPE_F64 && dist_dtype != SKNNR_DTYPE_F32)
        return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: dist_dtype = %d: stored distances are float64 (0), float32 (SKNNR_DTYPE_F32) or absent (SKNNR_REPLAY_NO_DIST)", dist_dtype);
    const bool has_dist = dist_dtype != SKNNR_REPLAY_NO_DIST;
    if (want_dist && !has_dist) return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: want_dist without stored distances");
    if (ids && ix->r_id_n == 0)
        return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: ids = 1 needs the id table (sknnr_index_set_replay_ids) first");
    sknnr_query_opts o{};
    o.n_neighbors = k;
    o.weight_mode = weight_mode;
    o.weight_law = weight_law;
    if (want_pred) {
        if (ix->t < 1) return fail(SKNNR_ERR_NO_TARGETS, "sknnr_replay_begin: the index was created without targets");
        if (k > kScanMaxKK) return fail(SKNNR_ERR_UNSUPPORTED, "sknnr_replay_begin: k = %d exceeds the HIP backend's limit of %d", k, kScanMaxKK);
        const int law = weight_law_check(ix, &o);
        if (law < 0) return law;
        if (!law && !weight_mode_ok(weight_mode, false))
            return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: a stream predicts with uniform or distance weights, or a weight law, only");
        if (!has_dist && (law || (weight_mode & SKNNR_WEIGHTS_BASE_MASK) == SKNNR_WEIGHTS_DISTANCE))
            return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: distance weights and weight laws need the stored distances");
    }
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (ix->stream_open) return fail(SKNNR_ERR_INVALID, "sknnr_replay_begin: a query stream is already open on this handle");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(ix->replay_rec.ensure((size_t)kHostSlots * kReplayRecWords));
    if (!ix->pin_replay)
        HIP_TRY(hipHostMalloc((void**)&ix->pin_replay, (size_t)kHostSlots * kReplayRecWords * sizeof(unsigned long long), hipHostMallocDefault));
    sknnr_stream* s = new (std::nothrow) sknnr_stream();
    if (!s) return fail(SKNNR_ERR_INVALID, "out of host memory");
    const int rc = pipe_open(s->pipe, ix, &o, Reduction{}, want_dist != 0, want_pred != 0);
    if (rc) {
        delete s;
        return rc;
    }
    HostPipe& p = s->pipe;
    p.replay.on = true;
    p.replay.ks = ks;
    p.replay.idx_bytes = idx_dtype == SKNNR_DTYPE_I32 ? 4 : 8;
    p.replay.dist_kind = !has_dist ? kReplayDistNone : (dist_dtype == SKNNR_DTYPE_F32 ? kReplayDistF32 : kReplayDistF64);
    p.replay.ids = ids != 0;
    p.replay.fill_index = (long)fill_index;
    p.lane[kLaneDist].search_out = has_dist;  // (the decode writes the distance tile only when distances are stored)
    std::fill(std::begin(ix->last_replay), std::end(ix->last_replay), 0);
    ix->stream_open = true;
    *out = s;
    return SKNNR_OK;
}

extern "C" int sknnr_replay_push(sknnr_stream* s, const void* idx, const void* dist, int64_t nq, void* out_dist, void* out_idx,
                                 void* out_pred) {
    if (s && s->pipe.replay.on && nq > 0) {
        if (!idx) return fail(SKNNR_ERR_INVALID, "sknnr_replay_push: idx is NULL");
        if (!dist != (s->pipe.replay.dist_kind == kReplayDistNone))
            return fail(SKNNR_ERR_INVALID, "sknnr_replay_push: dist is given exactly when the stream was opened with stored distances");
    }
    Push u(Push::kStored, false, out_idx, out_dist, out_pred, 0);
    u.stored = {(const char*)idx, (const char*)dist, 0};
    return stream_push(s, u, nq);
}

extern "C" int sknnr_replay_push_planes(sknnr_stream* s, const void* idx, const void* dist, int64_t nq, int64_t in_stride,
                                        void* out_dist, void* out_idx, void* out_pred, int64_t out_stride) {
    if (s && s->pipe.replay.on && nq > 0) {
        if (!idx) return fail(SKNNR_ERR_INVALID, "sknnr_replay_push_planes: idx is NULL");
        if (!dist != (s->pipe.replay.dist_kind == kReplayDistNone))
            return fail(SKNNR_ERR_INVALID, "sknnr_replay_push_planes: dist is given exactly when the stream was opened with stored distances");
        if (in_stride < nq) return fail(SKNNR_ERR_INVALID, "sknnr_replay_push_planes: in_stride (%lld) is below nq (%lld)", (long long)in_stride, (long long)nq);
        if (out_stride < nq) return fail(SKNNR_ERR_INVALID, "sknnr_replay_push_planes: out_stride (%lld) is below nq (%lld)", (long long)out_stride, (long long)nq);
    }
    Push u(Push::kStored, true, out_idx, out_dist, out_pred, (long)out_stride);
    u.stored = {(const char*)idx, (const char*)dist, (long)in_stride};
    return stream_push(s, u, nq);
}

extern "C" int sknnr_replay_get_counts(sknnr_stream* s, int64_t out[4]) {
    if (!s) return fail(SKNNR_ERR_INVALID, "sknnr_replay_get_counts: stream is NULL");
    if (!out) return fail(SKNNR_ERR_INVALID, "sknnr_replay_get_counts: out is NULL");
    HostPipe& p = s->pipe;
    if (!p.replay.on) return fail(SKNNR_ERR_INVALID, "sknnr_replay_get_counts: the stream was opened by sknnr_stream_begin");
    std::unique_lock<std::mutex> lock;
    if (const int rc = collect_begin(p, lock)) return rc;
    std::copy(p.replay_tot, p.replay_tot + 3, out);
    out[3] = p.replay_first;
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_replay(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "sknnr_debug_last_replay: NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    std::copy(ix->last_replay, ix->last_replay + 8, out);
    return SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// bootstrap
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_index_set_bootstrap(sknnr_index* ix, const uint8_t* table, int32_t B, int64_t n) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "sknnr_index_set_bootstrap: index is NULL");
    if (table) {
        if (B < 1 || B > kBootMaxB)
            return fail(SKNNR_ERR_INVALID, "sknnr_index_set_bootstrap: B = %d outside [1, %d]", B, kBootMaxB);
        if (n != ix->n_ref)
            return fail(SKNNR_ERR_INVALID, "sknnr_index_set_bootstrap: the table has %lld rows per replicate, the handle has %lld reference rows",
                        (long long)n, (long long)ix->n_ref);
    }
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (ix->stream_open) return fail(SKNNR_ERR_INVALID, "sknnr_index_set_bootstrap: a stream is open on this handle: end it first");
    ix->boot_B = 0;
    if (!table) return SKNNR_OK;
    const int bpad = (B + 63) / 64 * 64;
    std::vector<unsigned char> mt((size_t)n * bpad, 0);
    for (int64_t r0 = 0; r0 < n; r0 += 64)  // (64 x 64 blocks: both sides stay in cache)
        for (int b0 = 0; b0 < B; b0 += 64)
            for (int b = b0; b < std::min(B, b0 + 64); ++b)
                for (int64_t r = r0; r < std::min<int64_t>(n, r0 + 64); ++r) mt[(size_t)r * bpad + b] = table[(size_t)b * n + r];
    HIP_TRY(hipSetDevice(ix->device));
    if (ix->ws_busy) HIP_TRY(hipEventSynchronize(ix->ev_ws));  // (a reduction of an earlier call may still read the old table)
    if (int rc = ix->boot_mt.upload(mt.data(), mt.size())) return rc;
    ix->boot_B = B;
    ix->boot_bpad = bpad;
    return SKNNR_OK;
}

// A bootstrap plan as the kernel reads it: the distinct columns, every entry's place among them, the codes.
struct BootPlan {
    std::vector<int> ucols, uidx, codes;
};
static int boot_plan_check(const sknnr_index* ix, const int32_t* cols, const int32_t* stat, int32_t n_out, BootPlan& bp) {
    if (n_out < 1 || n_out > kBootMaxOut)
        return fail(SKNNR_ERR_INVALID, "a bootstrap plan has 1 to %d entries, got %d", kBootMaxOut, n_out);
    if (!cols || !stat) return fail(SKNNR_ERR_INVALID, "a bootstrap plan needs cols and stat");
    bp.uidx.assign((size_t)n_out, 0);
    bp.codes.assign(stat, stat + n_out);
    std::vector<int> place((size_t)ix->t, -1);
    for (int e = 0; e < n_out; ++e) {
        if (stat[e] < 0 || stat[e] >= kBootStatCount)
            return fail(SKNNR_ERR_INVALID, "bootstrap plan entry %d: unknown statistic %d", e, stat[e]);
        if (stat[e] == kBootCount) continue;  // (takes no column)
        if (cols[e] < 0 || cols[e] >= ix->t)
            return fail(SKNNR_ERR_INVALID, "bootstrap plan entry %d: column %d outside [0, %d)", e, cols[e], ix->t);
        if (place[(size_t)cols[e]] < 0) {
            place[(size_t)cols[e]] = (int)bp.ucols.size();
            bp.ucols.push_back(cols[e]);
        }
        bp.uidx[(size_t)e] = place[(size_t)cols[e]];
    }
    if (bp.ucols.empty()) bp.ucols.push_back(0);  // (counts only: the walk still needs a column to carry)
    return SKNNR_OK;
}

// The caps of a bootstrap reduction over lists of kw columns with replicates of k copies
static int boot_shape_check(const sknnr_index* ix, int32_t kw, int32_t k, int32_t mode, int32_t law) {
    if (ix->t < 1) return fail(SKNNR_ERR_NO_TARGETS, "the index was created without targets");
    if (ix->boot_B < 1) return fail(SKNNR_ERR_INVALID, "the handle has no bootstrap table (sknnr_index_set_bootstrap)");
    if (k < 1 || k > kw || kw > kBootMaxKw)
        return fail(SKNNR_ERR_INVALID, "a bootstrap needs 1 <= k <= kw <= %d, got k = %d, kw = %d", kBootMaxKw, k, kw);
    if (kw > ix->n_ref)
        return fail(SKNNR_ERR_INVALID, "kw = %d exceeds the handle's %lld reference rows", kw, (long long)ix->n_ref);
    if (mode & ~SKNNR_WEIGHTS_BASE_MASK)
        return fail(SKNNR_ERR_INVALID, "a bootstrap reduces in float64: weight mode flags are refused (mode %d)", mode);
    if (law == kLawNone) {
        if (mode == SKNNR_WEIGHTS_EXPLICIT) return fail(SKNNR_ERR_INVALID, "a bootstrap takes no explicit weights");
        if (mode != SKNNR_WEIGHTS_UNIFORM && mode != SKNNR_WEIGHTS_DISTANCE)
            return fail(SKNNR_ERR_INVALID, "unknown weight mode %d", mode);
        return SKNNR_OK;
    }
    sknnr_query_opts o{};
    o.weight_mode = mode;
    o.weight_law = law;
    const int rc = weight_law_check(ix, &o);
    return rc < 0 ? rc : SKNNR_OK;
}

// The kernel's arguments for lists of kw columns with the plan arrays at `plan` (ucols, uidx, codes back to back) and the
// launch; tally is added to.  Under the handle's lock.
static int enqueue_bootstrap(sknnr_index* ix, const double* dist, const long* idx, long nq, int kw, int k, int mode, int law,
                             const int* plan, int n_u, int n_out, double* out, unsigned long long* tally,
                             const unsigned char* skip, hipStream_t st) {
    BootstrapArgs a{};
    a.y = ix->y64.p;
    a.dist = mode == SKNNR_WEIGHTS_UNIFORM && law == kLawNone ? nullptr : dist;
    a.idx = idx;
    a.mt = ix->boot_mt.p;
    a.skip = skip;
    a.nq = nq;
    a.n_ref = ix->n_ref;
    a.kw = kw;
    a.k = k;
    a.t = ix->t;
    a.mode = law != kLawNone ? 2 : mode;
    a.law = law;
    a.p0 = ix->law_p0;
    a.p1 = ix->law_p1;
    a.B = ix->boot_B;
    a.bpad = ix->boot_bpad;
    a.ucols = plan;
    a.uidx = a.ucols + n_u;
    a.codes = a.uidx + n_out;
    a.n_u = n_u;
    a.n_out = n_out;
    a.out = out;
    a.tally = tally;
    a.ppw = bootstrap_ppw(a.B, kw);
    HIP_TRY(launch::bootstrap(a, st));
    const int64_t rec[8] = {nq, a.B, k, kw, n_out, a.ppw, nq > 0 ? 1 : 0, 0};
    std::copy(rec, rec + 8, ix->last_boot);
    return SKNNR_OK;
}

static std::vector<int> boot_plan_image(const BootPlan& bp) {
    std::vector<int> img;
    img.insert(img.end(), bp.ucols.begin(), bp.ucols.end());
    img.insert(img.end(), bp.uidx.begin(), bp.uidx.end());
    img.insert(img.end(), bp.codes.begin(), bp.codes.end());
    return img;
}

// The plan's arrays into `buf` (a one-shot call's boot.call.plan, or the open stream's boot.stream.plan) and the bootstrap
// of replicates of k copies over them; the caller names the tally words.
static int boot_upload(DevBuf<int>& buf, const BootPlan& bp, int k, Reduction& red) {
    const std::vector<int> img = boot_plan_image(bp);
    if (int rc = buf.upload(img.data(), img.size())) return rc;
    red = Reduction{};
    red.kind = kReduceBoot;
    red.boot.n_out = (int)bp.codes.size();
    red.boot.n_u = (int)bp.ucols.size();
    red.boot.k = k;
    red.boot.ucols = buf.p;
    red.boot.uidx = red.boot.ucols + red.boot.n_u;
    red.boot.codes = red.boot.uidx + red.boot.n_out;
    return SKNNR_OK;
}

// The bootstrap `red` of one launch's rows (launch_predict; a one-shot call comes here directly): red.boot_tally is added
// to; always float64, whatever flags the weight mode carries.  skip (or null): rows that enter no tally.
static int launch_bootstrap(sknnr_index* ix, const Reduction& red, const double* dist, const long* idx, long nq, int kw,
                            int mode, int law, double* out, const unsigned char* skip, hipStream_t st) {
    const BootStage& b = red.boot;
    const int base = law != kLawNone ? SKNNR_WEIGHTS_EXPLICIT : (mode & SKNNR_WEIGHTS_BASE_MASK);
    if (base != SKNNR_WEIGHTS_UNIFORM && !dist) return fail(SKNNR_ERR_INVALID, "these weights need the distances");
    const int rc = enqueue_bootstrap(ix, dist, idx, nq, kw, b.k, base, law, b.ucols, b.n_u, b.n_out, out, red.boot_tally, skip, st);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ix->ev_ws, st));
    ix->ws_busy = true;
    return SKNNR_OK;
}

extern "C" int sknnr_bootstrap_from_neighbors(sknnr_index* ix, const double* dist, const int64_t* idx, int64_t nq, int32_t kw,
                                              int32_t k, int32_t weight_mode, int32_t weight_law, const int32_t* cols,
                                              const int32_t* stat, int32_t n_out, double* out, int64_t* tally, int32_t mem,
                                              void* stream) {
    if (!ix) return fail(SKNNR_ERR_INVALID, "index is NULL");
    int rc = boot_shape_check(ix, kw, k, weight_mode, weight_law);
    if (rc) return rc;
    BootPlan bp;
    if ((rc = boot_plan_check(ix, cols, stat, n_out, bp))) return rc;
    if (nq < 0 || !idx || !out) return fail(SKNNR_ERR_INVALID, "bad argument");
    if (weight_mode != SKNNR_WEIGHTS_UNIFORM && !dist) return fail(SKNNR_ERR_INVALID, "these weights need dist");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (ix->boot_B < 1) return fail(SKNNR_ERR_INVALID, "the handle has no bootstrap table (sknnr_index_set_bootstrap)");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr;
    const size_t n_el = (size_t)nq * kw;
    Staged<long> di;
    Staged<double> dd, dout;
    Staged<unsigned long long> dt;
    // (uniform weights read no distances)
    if ((rc = di.stage(idx, n_el, mem, kStageIn)) || (rc = dout.stage(out, (size_t)nq * n_out, mem, kStageOut)) ||
        (rc = dt.stage(tally, 2, mem, kStageOut)) ||
        (rc = dd.stage(weight_mode != SKNNR_WEIGHTS_UNIFORM ? dist : nullptr, n_el, mem, kStageIn)))
        return rc;
    unsigned long long* tw = dt.p;
    if (!tw) {  // (not asked for: the handle's two words, behind the workspace's last user on `st`)
        if (ix->ws_busy) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ws, 0));
        HIP_TRY(ix->boot.call.tally.ensure(2));
        tw = ix->boot.call.tally.p;
    }
    // the plan is a workspace buffer: the previous reduction may still read it
    if (ix->ws_busy) HIP_TRY(hipEventSynchronize(ix->ev_ws));
    Reduction red;
    if ((rc = boot_upload(ix->boot.call.plan, bp, k, red))) return rc;
    red.boot_tally = tw;
    HIP_TRY(hipMemsetAsync(tw, 0, 2 * sizeof(unsigned long long), st));
    if ((rc = launch_bootstrap(ix, red, dd.p, di.p, nq, kw, weight_mode, weight_law, dout.p, nullptr, st))) return rc;
    if ((rc = dout.download())) return rc;
    return dt.download();
}

extern "C" int sknnr_stream_set_bootstrap(sknnr_stream* s, int32_t k, const int32_t* cols, const int32_t* stat, int32_t n_out) {
    if (!s) return fail(SKNNR_ERR_INVALID, "stream is NULL");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    if (!p.lane[kLanePred].want) return fail(SKNNR_ERR_INVALID, "the stream was opened without predictions");
    int rc = boot_shape_check(ix, p.k, k, p.o.weight_mode & SKNNR_WEIGHTS_BASE_MASK, p.o.weight_law);
    if (rc) return rc;
    BootPlan bp;
    if ((rc = boot_plan_check(ix, cols, stat, n_out, bp))) return rc;
    std::unique_lock<std::mutex> lock;
    if ((rc = setter_begin(s, lock, "sknnr_stream_set_bootstrap", kReduceBoot, "bootstrap"))) return rc;
    if (p.prod.tally) return fail(SKNNR_ERR_INVALID, "the stream tallies neighbour usage (sknnr_stream_set_tally): it takes no bootstrap");
    if (p.prod.domain) return fail(SKNNR_ERR_INVALID, "the stream has a distance domain (sknnr_stream_set_domain): it takes no bootstrap");
    if (p.prod.zonal) return fail(SKNNR_ERR_INVALID, "the stream has zonal statistics (sknnr_stream_set_zonal): it takes no bootstrap");
    if (p.lane[kLanePred].scale)
        return fail(SKNNR_ERR_INVALID, "sknnr_stream_set_bootstrap comes before sknnr_stream_set_output: the scale / offset hold one value per output plane");
    Reduction red;
    auto& bs = ix->boot.stream;
    if ((rc = boot_upload(bs.plan, bp, k, red))) return rc;
    HIP_TRY(bs.tally.ensure(2));
    HIP_TRY(hipMemsetAsync(bs.tally.p, 0, 2 * sizeof(unsigned long long), ix->st_run));  // (in front of the first tile)
    red.boot_tally = bs.tally.p;
    p.red = red;
    p.lane[kLanePred].cols = n_out;  // from now on the prediction lane is n_out wide
    return SKNNR_OK;
}

extern "C" int sknnr_stream_get_bootstrap(sknnr_stream* s, int64_t tally[2]) {
    if (!s || !tally) return fail(SKNNR_ERR_INVALID, "sknnr_stream_get_bootstrap: NULL argument");
    HostPipe& p = s->pipe;
    sknnr_index* ix = p.ix;
    if (p.red.kind != kReduceBoot) return fail(SKNNR_ERR_INVALID, "the stream has no bootstrap stage: sknnr_stream_set_bootstrap was not called");
    std::unique_lock<std::mutex> lock;
    if (const int rc = collect_begin(p, lock)) return rc;
    HIP_TRY(hipMemcpy(tally, ix->boot.stream.tally.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_bootstrap(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "sknnr_debug_last_bootstrap: NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    std::copy(ix->last_boot, ix->last_boot + 8, out);
    return SKNNR_OK;
}

// ----------------------------------------------------------------------------------------
// crosswalk
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_crosswalk(const int64_t* table, int64_t n_table, const int64_t* idx, int64_t n, int64_t* out,
                               int32_t device, int32_t mem, void* stream) {
    if (!table || !idx || !out || n < 0 || n_table < 1) return fail(SKNNR_ERR_INVALID, "bad argument");
    if (mem != SKNNR_MEM_DEVICE && mem != SKNNR_MEM_HOST) return fail(SKNNR_ERR_INVALID, "unknown memspace %d", mem);
    if (n == 0) return SKNNR_OK;
    HIP_TRY(hipSetDevice(device));
    Staged<long> dt, di, dout;
    int rc;
    if ((rc = dt.stage(table, (size_t)n_table, mem, kStageIn)) || (rc = di.stage(idx, (size_t)n, mem, kStageIn)) ||
        (rc = dout.stage(out, (size_t)n, mem, kStageOut)))
        return rc;
    HIP_TRY(launch::crosswalk(dt.p, di.p, n, dout.p, mem == SKNNR_MEM_DEVICE ? (hipStream_t)stream : nullptr));
    return dout.download();
}

// ----------------------------------------------------------------------------------------
// diagnostics
// ----------------------------------------------------------------------------------------
extern "C" int sknnr_debug_coarse_matrix(sknnr_index* ix, const double* q, int64_t nq, float* out, double* out_qnorm,
                                         double* out_scale, double* out_eps) {
    if (!ix || !q || !out || nq < 1) return fail(SKNNR_ERR_INVALID, "bad argument");
    if (ix->ks == 0) return fail(SKNNR_ERR_UNSUPPORTED, "no coarse image (d > 128)");
    if ((double)nq * (double)ix->n_ref > 16777216.0) return fail(SKNNR_ERR_INVALID, "nq * n_ref must be <= 2^24");
    std::lock_guard<std::mutex> lock(ix->mtx);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // default stream below; the workspace may still be in use on another one
    const long n_pad = pad_rows(nq);
    HIP_TRY(ix->xstage.ensure((size_t)nq * ix->d));
    HIP_TRY(hipMemcpy(ix->xstage.p, q, (size_t)nq * ix->d * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ix->qimg.ensure((size_t)(n_pad / 32) * 2 * ix->ks * 64));
    HIP_TRY(ix->qnc.ensure(n_pad));
    int rc = launch_prep(ix, SearchPlan{}, ix->xstage.p, nq, n_pad, nullptr, nullptr);
    if (rc) return rc;
    DevBuf<float> dout;
    HIP_TRY(dout.ensure((size_t)nq * ix->n_ref));
    const long n_tiles = (ix->n_ref + 31) / 32, nqb = (nq + 31) / 32;
    hipError_t e = launch::coarse_matrix(ix->ks, ix->rimg.p, ix->perm.p, ix->qimg.p, (int)ix->n_ref, nq, n_tiles, nqb, dout.p);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)nq * ix->n_ref * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_qnorm) e = hipMemcpy(out_qnorm, ix->qnc.p, nq * sizeof(double), hipMemcpyDeviceToHost);
    dout.release();
    if (e != hipSuccess) return fail(SKNNR_ERR_HIP, "debug matrix failed: %s", hipGetErrorString(e));
    if (out_scale) *out_scale = ix->s;
    if (out_eps) *out_eps = eps_units(ix->ks) * std::ldexp(1.0, -24);
    return SKNNR_OK;
}

// the debug records that are host words only: copied under the handle's lock
template <class Rec>
static int copy_record(const sknnr_index* cix, int64_t out[8], Rec rec) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "index / out is NULL");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    const int64_t* r = rec(ix);
    std::copy(r, r + 8, out);
    return SKNNR_OK;
}
extern "C" int sknnr_debug_last_prefilter(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last.prefilter; }); }
extern "C" int sknnr_debug_last_mask(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last.mask; }); }
extern "C" int sknnr_debug_last_prep(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last.prep; }); }
extern "C" int sknnr_debug_last_narrow(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last_narrow; }); }
extern "C" int sknnr_debug_last_summary(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last_summary; }); }
extern "C" int sknnr_debug_last_plan(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last_plan; }); }
extern "C" int sknnr_debug_last_planes(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last_planes; }); }
extern "C" int sknnr_debug_last_weight_law(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last_law; }); }
extern "C" int sknnr_debug_last_grouped(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last.grouped; }); }
extern "C" int sknnr_debug_last_buffer(const sknnr_index* ix, int64_t out[8]) { return copy_record(ix, out, [](sknnr_index* i) { return i->last.buffer; }); }

// The mask, the scan and the compaction alone, on the caller's device pointers (run_device_masked's sequence without the
// search): the block offsets and the ranks, which no search result shows, come back to the host.
extern "C" int sknnr_debug_mask_compact(const void* q, int64_t nq, int32_t d_in, int32_t query_dtype, const double* nodata,
                                        int32_t device, void* stream, uint8_t* out_valid, int32_t* out_blk_off,
                                        int32_t* out_rank, void* out_packed, int32_t* out_unit, int64_t* out_n_valid) {
    if (query_dtype < 0 || query_dtype >= kDtypeCount) return fail(SKNNR_ERR_INVALID, "unknown query_dtype %d", query_dtype);
    if (nq < 0) return fail(SKNNR_ERR_INVALID, "nq must be >= 0");
    if (d_in < 1 || d_in > kMaskMaxCols) return fail(SKNNR_ERR_INVALID, "d_in = %d outside [1, %d]", d_in, kMaskMaxCols);
    if (nq > 0x7fffffffL) return fail(SKNNR_ERR_UNSUPPORTED, "more than 2^31 - 1 rows in one call");
    if (!nodata) return fail(SKNNR_ERR_INVALID, "nodata is NULL");
    const size_t row_bytes = (size_t)d_in * dtype_bytes(query_dtype);
    if (out_unit) *out_unit = launch::compact_unit(q, out_packed, row_bytes);
    if (out_n_valid) *out_n_valid = 0;
    if (nq == 0) return SKNNR_OK;
    if (!q || !out_packed) return fail(SKNNR_ERR_INVALID, "q / out_packed is NULL");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const long nb = mask_blocks(nq);
    DevBuf<double> nd;
    DevBuf<int> blk, rank;
    DevBuf<long> nv;
    DevBuf<unsigned char> valid;
    HIP_TRY(nd.ensure((size_t)d_in));
    HIP_TRY(blk.ensure((size_t)nb));
    HIP_TRY(rank.ensure((size_t)nq));
    HIP_TRY(nv.ensure(1));
    HIP_TRY(valid.ensure((size_t)nq));
    HIP_TRY(hipMemcpyAsync(nd.p, nodata, (size_t)d_in * sizeof(double), hipMemcpyHostToDevice, st));
    MaskArgs a{};
    a.x = q;
    a.x_dtype = query_dtype;
    a.nq = nq;
    a.d_in = d_in;
    a.nodata = nd.p;
    a.valid = valid.p;
    a.blk = blk.p;
    HIP_TRY(launch::row_mask(a, nv.p, st));
    CompactArgs c{};
    c.x = q;
    c.out = out_packed;
    c.nq = nq;
    c.valid = valid.p;
    c.blk_off = blk.p;
    c.rank = rank.p;
    HIP_TRY(launch::row_compact(c, row_bytes, st));
    HIP_TRY(hipStreamSynchronize(st));
    long n_valid = 0;
    HIP_TRY(hipMemcpy(&n_valid, nv.p, sizeof n_valid, hipMemcpyDeviceToHost));
    if (out_valid) HIP_TRY(hipMemcpy(out_valid, valid.p, (size_t)nq, hipMemcpyDeviceToHost));
    if (out_blk_off) HIP_TRY(hipMemcpy(out_blk_off, blk.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost));
    if (out_rank) HIP_TRY(hipMemcpy(out_rank, rank.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost));
    if (out_n_valid) *out_n_valid = n_valid;
    return SKNNR_OK;
}

// The expansion alone, on the caller's device pointers.
extern "C" int sknnr_debug_expand_rows(int64_t nq, int32_t k, int32_t t, const uint8_t* valid, const int32_t* rank,
                                       const int64_t* c_idx, const double* c_dist, const double* c_pred, int64_t* idx,
                                       double* dist, double* pred, int64_t fill_index, void* stream) {
    if (nq < 0 || nq > 0x7fffffffL) return fail(SKNNR_ERR_INVALID, "nq outside [0, 2^31 - 1]");
    if (k < 1 || t < 1) return fail(SKNNR_ERR_INVALID, "k and t must be >= 1");
    ExpandArgs e{};
    e.nq = nq;
    e.k = k;
    e.t = t;
    e.valid = valid;
    e.rank = rank;
    e.c_idx = (const long*)c_idx;
    e.c_dist = c_dist;
    e.c_pred = c_pred;
    e.idx = (long*)idx;
    e.dist = dist;
    e.pred = pred;
    e.fill_index = fill_index;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t err = launch::row_expand(e, st);
    if (err == hipErrorInvalidValue)
        return fail(SKNNR_ERR_INVALID, "an output is asked for without rank or without its packed results");
    HIP_TRY(err);
    HIP_TRY(hipStreamSynchronize(st));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_finalize(const sknnr_index* cix, int64_t out[4]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    out[0] = ix->last.finalize[0];
    out[1] = ix->last.finalize[1];
    out[2] = out[3] = 0;
    if (ix->last.finalize[1]) {
        // the rows the truncation rule put on the fail list, over every device chunk of the call (the workspace is the
        // handle's: no later call has touched it, or the record would be zero)
        int n_trunc = 0;
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&n_trunc, ix->fail_count.p + 3, sizeof n_trunc, hipMemcpyDeviceToHost));
        out[2] = n_trunc;
    }
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_hamming(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    std::copy(std::begin(ix->last.hamming), std::end(ix->last.hamming), out);
    out[7] = 0;
    if (ix->last.hamming[0]) {
        // the rows hamming_rescore_kernel put on the fail list, over every device chunk of the call (the workspace is the
        // handle's: no later call has touched it, or the record would be zero)
        int n_fail = 0;
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&n_fail, ix->fail_count.p, sizeof n_fail, hipMemcpyDeviceToHost));
        out[7] = n_fail;
    }
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_scan(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    const int64_t* r = ix->last.scan;
    std::copy(r, r + 8, out);
    out[7] = 0;
    if (!r[0]) return SKNNR_OK;
    if (r[5] < 0 || r[7]) {
        // the counts the kernels worked from (the workspace is the handle's: no later call has touched it, or the record
        // would be zero): rows on the fail list, rows scan_merge_kernel filed for the sequential replay
        int cnt[3] = {0, 0, 0};
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(cnt, ix->fail_count.p, sizeof cnt, hipMemcpyDeviceToHost));
        if (r[5] < 0) out[5] = cnt[0];
        if (r[5] < 0 && ix->last.rescue[0]) {  // the scan consumed the rescue's second list
            int handed = 0;
            HIP_TRY(hipMemcpy(&handed, ix->resc_state.p + kRescueHanded, sizeof handed, hipMemcpyDeviceToHost));
            out[5] = handed;
        }
        if (r[7]) out[7] = cnt[2];
    }
    if (!r[6]) out[6] = scan_slices(out[5], scan_nq((int)r[0] - 1), (int)ix->n_ref, (int)r[2], (int)r[3]);
    return SKNNR_OK;
}

extern "C" int sknnr_debug_last_rescue(const sknnr_index* cix, int64_t out[8]) {
    if (!cix || !out) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    std::fill(out, out + 8, 0);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    long long total[2] = {0, 0};
    HIP_TRY(hipMemcpy(total, ix->fail_total.p, sizeof total, hipMemcpyDeviceToHost));
    out[7] = total[1];
    if (!ix->last.rescue[0]) return SKNNR_OK;
    // (the workspace is the handle's: no later call has touched it, or the record would be zero)
    int w[kRescueWords];
    HIP_TRY(hipMemcpy(w, ix->resc_state.p, sizeof w, hipMemcpyDeviceToHost));
    out[0] = 1;
    out[1] = ix->last.rescue[1];
    out[2] = w[kRescueOffered];
    out[3] = w[kRescueNoThr];
    out[4] = w[kRescueOverflow];
    out[5] = w[kRescueOffered] - w[kRescueHanded];
    out[6] = w[kRescueHanded];
    return SKNNR_OK;
}

extern "C" int sknnr_debug_hamming_candidates(const sknnr_index* cix, int32_t* cnt, int32_t* ids, int64_t n) {
    if (!cix || !cnt || !ids) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (!ix->last.hamming[0]) return fail(SKNNR_ERR_INVALID, "the last call did not run the integer Hamming pre-filter");
    if (n < 0 || n > ix->last.hamming_rows)
        return fail(SKNNR_ERR_INVALID, "n = %ld rows, the last device chunk has %ld", (long)n, ix->last.hamming_rows);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cnt, ix->h_cand_cnt.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ids, ix->h_cand_id.p, (size_t)n * kHamCand * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_coarse_candidates(const sknnr_index* cix, int64_t n, float* val, int32_t* pos, int32_t* perm) {
    if (!cix || !val || !pos || !perm) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    const int64_t* r = ix->last.prefilter;
    if (!r[0]) return fail(SKNNR_ERR_UNSUPPORTED, "the last call ran no Euclidean pre-filter");
    if (ix->last.finalize[1]) return fail(SKNNR_ERR_UNSUPPORTED, "the last call filed merged candidate records, not lists");
    // (coarse2_kernel files its lists by position of a bucketed call and in positions of its own image: nothing reads them yet)
    if (r[0] != 1) return fail(SKNNR_ERR_UNSUPPORTED, "the last call ran the second-generation pre-filter: its lists are not served");
    // (the workspace is the handle's: no later call has touched it, or the record would be zero)
    const int64_t rows = r[5];
    if (n < 0 || n > rows)
        return fail(SKNNR_ERR_INVALID, "n = %ld rows, the last device chunk has %ld with its padding", (long)n, (long)rows);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t entries = (size_t)n * 2 * (size_t)r[2];
    if (entries) {
        HIP_TRY(hipMemcpy(val, ix->cand_val.p, entries * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pos, ix->cand_idx.p, entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(perm, ix->perm.p, (size_t)ix->n_ref * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_query_prep(const sknnr_index* cix, int64_t n, void* qimg, double* qnc, double* xt, uint8_t* cell,
                                      int32_t* perm, double* qnc_pos) {
    if (!cix) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    const int64_t* r = ix->last.prep;
    if (!r[0]) return fail(SKNNR_ERR_INVALID, "the last call ran no query preparation kernel");
    if (n < 0 || n > r[4]) return fail(SKNNR_ERR_INVALID, "n = %ld rows, the last device chunk has %ld with its padding", (long)n, (long)r[4]);
    if (xt && !ix->last.prep_xt) return fail(SKNNR_ERR_INVALID, "the last call wrote no transformed rows");
    if ((cell || perm) && !ix->last.prep_bucketed) return fail(SKNNR_ERR_INVALID, "the last call was not bucketed");
    if (qnc_pos && !ix->last.prep_qnc_pos) return fail(SKNNR_ERR_INVALID, "the last call filed no |q'|^2 by position");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t rows = (size_t)n;
    if (qimg) HIP_TRY(hipMemcpy(qimg, ix->qimg.p, rows * 64 * ix->ks, hipMemcpyDeviceToHost));
    if (qnc) HIP_TRY(hipMemcpy(qnc, ix->qnc.p, rows * sizeof(double), hipMemcpyDeviceToHost));
    if (xt) HIP_TRY(hipMemcpy(xt, ix->last.prep_xt, (size_t)std::min<int64_t>(n, r[3]) * ix->d * sizeof(double), hipMemcpyDeviceToHost));
    if (cell) HIP_TRY(hipMemcpy(cell, ix->qcell.p, rows, hipMemcpyDeviceToHost));
    if (perm) HIP_TRY(hipMemcpy(perm, ix->qperm.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (qnc_pos) HIP_TRY(hipMemcpy(qnc_pos, ix->qnc_pos.p, rows * sizeof(double), hipMemcpyDeviceToHost));
    return SKNNR_OK;
}

extern "C" int sknnr_debug_search_plan(int64_t n_ref, int32_t d, int32_t cell_depth, int32_t kk, int64_t nq, int32_t formula,
                                       int32_t flags, int64_t out[16]) {
    const bool exclude_self = flags & 1;
    if (!out || n_ref < 1 || d < 1 || kk < (exclude_self ? 2 : 1) || nq < 0 || cell_depth < 0 || cell_depth > kCellMaxDepth ||
        formula < SKNNR_FORMULA_EXPANDED || formula > SKNNR_FORMULA_HAMMING)
        return fail(SKNNR_ERR_INVALID, "bad argument");
    // the description sknnr_index_create would leave for these shapes (no affine map)
    const int ks = (d + 15) / 16 <= kMaxKs ? (d + 15) / 16 : 0;
    const IndexDesc ix{n_ref, d, ks, d, image_stages2(n_ref, ks), cell_depth, (flags & 8) != 0, (flags & 4) != 0};
    sknnr_query_opts o{};
    o.n_neighbors = kk - (exclude_self ? 1 : 0);
    o.exclude_self = exclude_self;
    o.formula = formula;
    const SearchPlan p = plan_search(ix, &o, nq, true, (flags & 2) ? 1 : 0);
    const int64_t words[16] = {p.coarse ? (p.v2 ? 2 : 1) : 0, p.coarse ? ks : 0, p.coarse ? p.m_list : 0, p.coarse ? p.rank_extra : 0,
                               p.bucketed ? cell_depth : 0, p.record, p.rescue, p.ham_int, p.kk, p.chunk, p.cap_pad, p.to_xt,
                               p.d_x, p.check_finite, p.x_dtype, (p.affine ? 1 : 0) | (p.self_rows ? 2 : 0)};
    std::copy(std::begin(words), std::end(words), out);
    return SKNNR_OK;
}

extern "C" int sknnr_debug_image_constants(const sknnr_index* cix, double* mu, double* s, int32_t* cell_depth, float* axes,
                                           float* centre, float* thr) {
    if (!cix) return fail(SKNNR_ERR_INVALID, "NULL argument");
    sknnr_index* ix = const_cast<sknnr_index*>(cix);
    std::lock_guard<std::mutex> lock(ix->mtx);
    if (ix->ks == 0) return fail(SKNNR_ERR_UNSUPPORTED, "no coarse image (d > 128)");
    if (mu) std::copy(ix->mu.begin(), ix->mu.begin() + 16 * ix->ks, mu);
    if (s) *s = ix->s;
    if (cell_depth) *cell_depth = ix->cell_depth;
    if ((axes || centre || thr) && ix->cell_depth > 0) {
        HIP_TRY(hipSetDevice(ix->device));
        if (axes) HIP_TRY(hipMemcpy(axes, ix->cell_axes.p, (size_t)ix->cell_depth * ix->d * sizeof(float), hipMemcpyDeviceToHost));
        if (centre) HIP_TRY(hipMemcpy(centre, ix->cell_centre.p, (size_t)ix->d * sizeof(float), hipMemcpyDeviceToHost));
        if (thr) HIP_TRY(hipMemcpy(thr, ix->cell_thr.p, (((size_t)1 << ix->cell_depth) - 1) * sizeof(float), hipMemcpyDeviceToHost));
    }
    return SKNNR_OK;
}

#endif  // SKNNR_LANE_ARITHMETIC_ONLY
