// host_stage.h -- the pure host arithmetic of the host pipeline (sknnr_hip.hip): the byte layout of its output lanes, the
// staging copies into and out of the pinned slots, the cuts of a push into tiles, and the description of a push.
// Nothing of HIP is included or named here: element sizes and the row quantum arrive as plain integers, so that
// tests/cpp/host_stage_main.cpp and scripts/lane_arithmetic_check.cpp compile this alone on the CPU, under the sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

// ----------------------------------------------------------------------------------------
// the outputs of the host pipeline: one lane each
// ----------------------------------------------------------------------------------------
// What the host pipeline hands to the caller, in the order the debug records use (bit `1 << lane` of last_narrow's wide mask).
enum { kLaneIdx = 0, kLaneDist = 1, kLanePred = 2, kLanes = 3 };

// The byte arithmetic of a lane: `cols` columns (k, k, t) of `esz` bytes per element (8 unless the output is typed).
inline size_t lane_bytes(long n, int cols, size_t esz) { return (size_t)n * cols * esz; }               // a tile of n rows
inline size_t lane_units(long n, int cols, size_t esz) { return (lane_bytes(n, cols, esz) + 7) / 8; }  // ... in 8-byte words
// Where tile [c0, ...) starts in the caller's array: packed (N, cols) rows, or planes -- there the tile is a segment of
// every plane, and the address is that of the first plane's.
inline size_t lane_tile_offset(long c0, int cols, size_t esz, bool planes) { return (size_t)c0 * (planes ? 1 : cols) * esz; }

// ----------------------------------------------------------------------------------------
// staging copies
// ----------------------------------------------------------------------------------------
// piece(a, b) over the byte range [0, bytes): one call below 16 MiB, else shared out over at most 8 threads in pieces
// rounded up to 4 KiB.  A single core copies ~10 GB/s, PCIe Gen5 x16 moves ~50.
template <typename Piece>
inline void fan_out(size_t bytes, Piece piece) {
    const size_t kMin = 8u << 20;
    unsigned n = std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
    if (bytes < 2 * kMin) n = 1;
    if (n == 1) {
        piece((size_t)0, bytes);
        return;
    }
    std::vector<std::thread> th;
    // (the share rounded UP before the 4 KiB rounding: a share that is a whole number of pages would leave bytes % n behind)
    const size_t per = (((bytes + n - 1) / n) + 4095) & ~(size_t)4095;
    for (unsigned i = 0; i < n; ++i) {
        const size_t a = (size_t)i * per;
        if (a >= bytes) break;
        th.emplace_back(piece, a, std::min(a + per, bytes));
    }
    for (auto& t : th) t.join();
}

inline void parallel_copy(void* dst, const void* src, size_t bytes) {
    fan_out(bytes, [=](size_t a, size_t b) { std::memcpy((char*)dst + a, (const char*)src + a, b - a); });
}

// Staging copy of a band-first tile: elements [off, off + n) of each of `c` separately held planes, packed (c, n) into
// dst.  Plain copies, one per band (nothing is transposed on the host); a large tile's bands are shared out by the bytes
// of the packed destination, as parallel_copy does for rows.
inline void stage_planes(void* dst, const void* const* planes, int c, size_t esz, long off, long n) {
    const size_t seg = (size_t)n * esz;
    fan_out(seg * c, [=](size_t a, size_t b) {  // bytes [a, b) of the packed destination
        while (a < b) {
            const size_t j = a / seg, within = a - j * seg, len = std::min(seg - within, b - a);
            std::memcpy((char*)dst + a, (const char*)planes[j] + (size_t)off * esz + within, len);
            a += len;
        }
    });
}
// The copy-out counterpart: `c` segments of n elements of esz bytes, packed in src, to dst + j * stride.
inline void unstage_planes(void* dst, const void* src, int c, long n, long stride, size_t esz) {
    for (int j = 0; j < c; ++j)
        parallel_copy((char*)dst + (size_t)j * stride * esz, (const char*)src + (size_t)j * n * esz, (size_t)n * esz);
}

// ---- neighbour replay: what a tile holds instead of feature rows -----------------------------------------------------------
// the stored columns and the bytes of a stored index (4 / 8) and of a stored distance (4 / 8; 0: none are stored)
struct ReplayLayout {
    int ks = 0;
    int idx_bytes = 8;
    int dist_bytes = 0;
};
// the stored arrays of one push: rows (n, ks), or planes `stride` elements apart; dist null without distances
struct ReplaySrc {
    const char* idx = nullptr;
    const char* dist = nullptr;
    long stride = 0;
};
// A tile of n pixels as it is staged and uploaded: the index block -- rows (n, ks) or planes (ks, n), packed -- and,
// 16-byte aligned behind it, the distance block in the same layout.
inline size_t replay_dist_offset(const ReplayLayout& r, long n) { return ((size_t)n * r.ks * r.idx_bytes + 15) & ~(size_t)15; }
inline size_t replay_tile_bytes(const ReplayLayout& r, long n) { return replay_dist_offset(r, n) + (size_t)n * r.ks * r.dist_bytes; }
// Staging copy of pixels [off, off + n) of a push: plain copies, one per block of a row tile, one per plane otherwise.
inline void stage_replay(void* dst, const ReplayLayout& r, const ReplaySrc& s, bool planes, long off, long n) {
    const auto block = [&](char* to, const char* from, size_t esz) {
        if (!planes) {
            parallel_copy(to, from + (size_t)off * r.ks * esz, (size_t)n * r.ks * esz);
            return;
        }
        for (int j = 0; j < r.ks; ++j)
            parallel_copy(to + (size_t)j * n * esz, from + ((size_t)j * s.stride + off) * esz, (size_t)n * esz);
    };
    block((char*)dst, s.idx, (size_t)r.idx_bytes);
    if (r.dist_bytes) block((char*)dst + replay_dist_offset(r, n), s.dist, (size_t)r.dist_bytes);
}

// ----------------------------------------------------------------------------------------
// a push and its tiles
// ----------------------------------------------------------------------------------------
// The boundaries of the tiles of a push of nq pixels: at most `cap` each.  A pipeline that starts empty (`idle`) ramps up
// (`ramp`): the device waits for the first tile's staging copy and host-to-device transfer (7 ms for a 1M-row tile) with
// nothing to do, so the first tiles are an eighth, a quarter and a half of the regular size, in multiples of `quantum`
// (the search's row quantum).
inline std::vector<long> tile_cuts(long nq, long cap, bool idle, bool ramp, long quantum) {
    std::vector<long> cuts;
    long c = 0;
    if (idle && ramp && nq > cap / 2)
        for (long part : {cap / 8, cap / 4, cap / 2}) {
            part = std::max<long>(part / quantum * quantum, quantum);
            if (c + part >= nq) break;
            c += part;
            cuts.push_back(c);
        }
    while (c < nq) {
        c = std::min(nq, c + cap);
        cuts.push_back(c);
    }
    return cuts;
}

// One push as its entry point describes it, once: where its pixels come from, where its results go.  A tile is
// (push, off, n): pixels [off, off + n) of it.  The arrays it names are the caller's and stay valid until the last tile
// has been submitted (the inputs) or has left the pipeline (the outputs).
struct Push {
    // the input, in exactly one form: (nq, cols) rows at `rows`; `cols` separately held bands; stored neighbours
    enum Source { kRows, kBands, kStored } source = kRows;
    const void* rows = nullptr;
    const void* const* bands = nullptr;
    ReplaySrc stored{};
    int cols = 0;           // kRows / kBands: the input columns, of
    size_t esz = 0;         // ... this many bytes per element
    ReplayLayout layout{};  // kStored
    // The layout the results leave in -- planes out_stride elements apart, or rows -- and, replayed, that of the stored arrays.
    bool band_first = false;
    void* out[kLanes] = {};  // per lane, in the lane's own element type (null: not asked for in this push)
    long out_stride = 0;
    const int32_t* zones = nullptr;  // one zone code per pixel (null unless the pipeline is zonal)
    uint8_t* domain_out = nullptr;   // where the code plane goes, one byte per pixel (null: not asked for)
    long push_no = 0;                // which push of its pipeline this is, counting from 0

    Push() = default;
    // what an entry point knows before it has looked at the pipeline; it names the source's arrays itself
    Push(Source source_, bool band_first_, void* out_idx, void* out_dist, void* out_pred, long out_stride_)
        : source(source_), band_first(band_first_), out{out_idx, out_dist, out_pred} /* (lane order) */, out_stride(out_stride_) {}

    // the bytes a tile of n pixels takes in a pinned slot, and on the device
    size_t staged_bytes(long n) const { return source == kStored ? replay_tile_bytes(layout, n) : (size_t)n * cols * esz; }
    // pixels [off, off + n) into a pinned slot
    void stage(void* dst, long off, long n) const {
        if (source == kStored) stage_replay(dst, layout, stored, band_first, off, n);
        else if (source == kBands) stage_planes(dst, bands, cols, esz, off, n);
        else parallel_copy(dst, (const char*)rows + (size_t)off * cols * esz, (size_t)n * cols * esz);
    }
    // where the results of the tile at pixel c0 go: lane l (of lane_cols columns of lane_esz bytes), and the code plane
    void* out_at(int l, long c0, int lane_cols, size_t lane_esz) const {
        return out[l] ? (char*)out[l] + lane_tile_offset(c0, lane_cols, lane_esz, band_first) : nullptr;
    }
    uint8_t* domain_at(long c0) const { return domain_out ? domain_out + c0 : nullptr; }
};
