// The host pipeline's pure arithmetic (sknnr_amd/csrc/host_stage.h) alone on the CPU, under the sanitizers:
// tests/test_host_stage_cpu.py compiles this with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -I sknnr_amd/csrc tests/cpp/host_stage_main.cpp
// and runs it.  Every source and destination is a heap block of exactly the bytes that may be touched, so a size or an
// offset that is off runs into the sanitizer; the staged bytes are compared with plain loops written here, and the bytes
// around a destination (and between the planes of a caller's array) must keep their fill.
#include "host_stage.h"

#include <cstdio>
#include <cstdlib>
#include <numeric>

namespace {

int failures = 0;

void check(bool ok, const char* what, long a = 0, long b = 0) {
    if (ok) return;
    std::fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
    ++failures;
}

// ---- cuts -----------------------------------------------------------------------------------------------------------------
constexpr long kQuantum = 6144;  // the search's row quantum (kRowQuantum, coarse.hip.h)
constexpr long kMi = 1L << 20;

struct CutCase {
    long nq, cap;
    std::vector<long> ramped, plain;  // idle with the ramp on; every other combination
};
// What the loop in pipe_submit_rows gave before it became tile_cuts, written out.
const CutCase kCuts[] = {
    {1, 1024, {1}, {1}},
    {1023, 1024, {1023}, {1023}},
    {1024, 1024, {1024}, {1024}},
    {1025, 1024, {1024, 1025}, {1024, 1025}},
    {7000, 1024, {6144, 7000}, {1024, 2048, 3072, 4096, 5120, 6144, 7000}},
    {20000, 1024, {6144, 12288, 18432, 19456, 20000},
     {1024, 2048, 3072, 4096, 5120, 6144, 7168, 8192, 9216, 10240, 11264, 12288, 13312, 14336, 15360, 16384, 17408, 18432, 19456, 20000}},
    {kMi + 1, kMi, {129024, 387072, 909312, 1048577}, {1048576, 1048577}},
    {3 * kMi, kMi, {129024, 387072, 909312, 1957888, 3006464, 3145728}, {1048576, 2097152, 3145728}},
};

void cuts() {
    for (const CutCase& c : kCuts)
        for (int idle = 0; idle < 2; ++idle)
            for (int ramp = 0; ramp < 2; ++ramp) {
                const std::vector<long> got = tile_cuts(c.nq, c.cap, idle, ramp, kQuantum);
                check(got == (idle && ramp ? c.ramped : c.plain), "tile_cuts differs from the table", c.nq, 2 * idle + ramp);
                check(!got.empty() && got.back() == c.nq, "the cuts do not end at nq", c.nq);
                long prev = 0;
                for (long cut : got) {
                    check(cut > prev, "the cuts are not strictly increasing", c.nq, cut);
                    check(cut - prev <= std::max(c.cap, kQuantum), "a tile above max(cap, quantum)", c.nq, cut);
                    prev = cut;
                }
            }
}

// ---- guarded blocks ---------------------------------------------------------------------------------------------------------
constexpr size_t kGuard = 64;
constexpr unsigned char kGuardFill = 0xA5, kFill = 0x5A;

// `bytes` of kFill between two guards; body() is the destination
struct Guarded {
    std::vector<unsigned char> mem;
    explicit Guarded(size_t bytes) : mem(bytes + 2 * kGuard, kGuardFill) { std::fill(body(), body() + bytes, kFill); }
    unsigned char* body() { return mem.data() + kGuard; }
    size_t bytes() const { return mem.size() - 2 * kGuard; }
    bool guards_intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (mem[i] != kGuardFill || mem[mem.size() - 1 - i] != kGuardFill) return false;
        return true;
    }
};

// a heap block of exactly n bytes holding a byte pattern that depends on `seed`
std::vector<unsigned char> pattern(size_t n, unsigned seed) {
    std::vector<unsigned char> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (unsigned char)((i * 131u + seed * 29u + (i >> 8)) & 0xff);
    return v;
}

struct Tile {
    long off, n;
};
// a push of N pixels: the whole of it, all but the first pixel, and the last pixel alone (offsets 0, 1 and N - 1)
std::vector<Tile> tiles_of(long N) { return {{0, N}, {1, N - 1}, {N - 1, 1}}; }

// ---- rows -------------------------------------------------------------------------------------------------------------------
void rows() {
    const long N = 37;
    const int cols = 5, k = 3;
    const size_t esz = 8, out_esz = 4;
    const std::vector<unsigned char> src = pattern((size_t)N * cols * esz, 1);
    std::vector<unsigned char> out((size_t)N * k * out_esz, kFill);  // the caller's (N, k) rows of one lane
    Push u;
    u.rows = src.data();
    u.cols = cols;
    u.esz = esz;
    u.out[kLaneIdx] = out.data();
    for (const Tile& t : tiles_of(N)) {
        check(u.staged_bytes(t.n) == (size_t)t.n * cols * esz, "rows: staged_bytes", t.off, t.n);
        Guarded pin(u.staged_bytes(t.n));
        u.stage(pin.body(), t.off, t.n);
        check(pin.guards_intact(), "rows: stage wrote outside its tile", t.off, t.n);
        check(std::memcmp(pin.body(), src.data() + (size_t)t.off * cols * esz, pin.bytes()) == 0, "rows: staged bytes", t.off, t.n);
        // the way out: a tile of the lane's results to where out_at says
        const std::vector<unsigned char> res = pattern(lane_bytes(t.n, k, out_esz), 2);
        std::fill(out.begin(), out.end(), kFill);
        unsigned char* at = (unsigned char*)u.out_at(kLaneIdx, t.off, k, out_esz);
        check(at == out.data() + (size_t)t.off * k * out_esz, "rows: out_at", t.off, t.n);
        parallel_copy(at, res.data(), res.size());
        for (size_t i = 0; i < out.size(); ++i) {
            const size_t lo = (size_t)t.off * k * out_esz;
            const unsigned char want = i >= lo && i < lo + res.size() ? res[i - lo] : kFill;
            if (out[i] != want) {
                check(false, "rows: copy-out", t.off, (long)i);
                break;
            }
        }
        check(u.out_at(kLaneDist, t.off, k, out_esz) == nullptr && u.domain_at(t.off) == nullptr, "a lane nobody asked for", t.off);
    }
}

// ---- bands: 3 separately held bands of 2-byte elements ---------------------------------------------------------------------
void bands() {
    const long N = 41, stride = N + 6;  // (the caller's output planes are `stride` elements apart)
    const int c = 3, k = 2;
    const size_t esz = 2, out_esz = 8;
    std::vector<std::vector<unsigned char>> band;
    const void* ptrs[c];
    for (int j = 0; j < c; ++j) {
        band.push_back(pattern((size_t)N * esz, 10 + j));
        ptrs[j] = band[j].data();
    }
    std::vector<unsigned char> out(((size_t)(k - 1) * stride + N) * out_esz, kFill);  // (k, N) windows of a (k, stride) array
    Push u;
    u.source = Push::kBands;
    u.bands = ptrs;
    u.cols = c;
    u.esz = esz;
    u.band_first = true;
    u.out[kLanePred] = out.data();
    u.out_stride = stride;
    for (const Tile& t : tiles_of(N)) {
        check(u.staged_bytes(t.n) == (size_t)t.n * c * esz, "bands: staged_bytes", t.off, t.n);
        Guarded pin(u.staged_bytes(t.n));
        u.stage(pin.body(), t.off, t.n);
        check(pin.guards_intact(), "bands: stage wrote outside its tile", t.off, t.n);
        for (int j = 0; j < c; ++j)
            check(std::memcmp(pin.body() + (size_t)j * t.n * esz, band[j].data() + (size_t)t.off * esz, (size_t)t.n * esz) == 0,
                  "bands: staged plane", t.off, j);
        // the way out: packed (k, n) results to the caller's planes
        const std::vector<unsigned char> res = pattern(lane_bytes(t.n, k, out_esz), 3);
        std::fill(out.begin(), out.end(), kFill);
        unsigned char* at = (unsigned char*)u.out_at(kLanePred, t.off, k, out_esz);
        check(at == out.data() + (size_t)t.off * out_esz, "bands: out_at", t.off, t.n);
        unstage_planes(at, res.data(), k, t.n, u.out_stride, out_esz);
        for (size_t i = 0; i < out.size(); ++i) {
            const size_t plane = i / ((size_t)stride * out_esz), within = i % ((size_t)stride * out_esz);
            const size_t lo = (size_t)t.off * out_esz, len = (size_t)t.n * out_esz;
            const unsigned char want = within >= lo && within < lo + len ? res[plane * len + within - lo] : kFill;
            if (out[i] != want) {
                check(false, "bands: copy-out", t.off, (long)i);
                break;
            }
        }
    }
}

// ---- stored neighbours: 4-byte indices and 4-byte distances, rows and planes ---------------------------------------------------
void stored(bool planes) {
    const long N = 29, stride = planes ? N + 5 : 0;
    const ReplayLayout lay{5, 4, 4};
    const size_t elems = planes ? (size_t)(lay.ks - 1) * stride + N : (size_t)N * lay.ks;  // (ks, N) windows of (ks, stride)
    const std::vector<unsigned char> idx = pattern(elems * 4, 20), dist = pattern(elems * 4, 21);
    Push u;
    u.source = Push::kStored;
    u.stored = {(const char*)idx.data(), (const char*)dist.data(), stride};
    u.layout = lay;
    u.band_first = planes;
    for (const Tile& t : tiles_of(N)) {
        const size_t block = (size_t)t.n * lay.ks * 4, d0 = (block + 15) / 16 * 16;
        check(replay_dist_offset(lay, t.n) == d0 && u.staged_bytes(t.n) == d0 + block, "stored: layout of a tile", t.off, t.n);
        Guarded pin(u.staged_bytes(t.n));
        u.stage(pin.body(), t.off, t.n);
        check(pin.guards_intact(), "stored: stage wrote outside its tile", t.off, t.n);
        const unsigned char* src[2] = {idx.data(), dist.data()};
        for (int which = 0; which < 2; ++which)
            for (long i = 0; i < t.n; ++i)
                for (int j = 0; j < lay.ks; ++j) {
                    const size_t to = (which ? d0 : 0) + (planes ? (size_t)j * t.n + i : (size_t)i * lay.ks + j) * 4;
                    const size_t from = (planes ? (size_t)j * stride + t.off + i : (size_t)(t.off + i) * lay.ks + j) * 4;
                    if (std::memcmp(pin.body() + to, src[which] + from, 4) != 0) {
                        check(false, planes ? "stored planes: staged element" : "stored rows: staged element", t.off, i);
                        i = t.n;
                        break;
                    }
                }
        for (size_t i = block; i < d0; ++i) check(pin.body()[i] == kFill, "stored: the padding between the blocks was written", t.off, (long)i);
    }
    const ReplayLayout none{5, 8, 0};  // (no stored distances: the tile ends with its aligned index block)
    check(replay_tile_bytes(none, 3) == 128 && replay_dist_offset(none, 3) == 128, "stored: layout without distances");
}

// ---- the fan-out: 33 MiB and an odd count, so that the threads and their 4 KiB rounding run -----------------------------------
void fan_out_once() {
    const size_t bytes = 33 * (size_t)kMi + 7;
    const std::vector<unsigned char> src = pattern(bytes, 30);
    {
        Guarded dst(bytes);
        parallel_copy(dst.body(), src.data(), bytes);
        check(dst.guards_intact() && std::memcmp(dst.body(), src.data(), bytes) == 0, "fan-out: parallel_copy");
    }
    {
        // three bands of a third each (the pieces then cross band boundaries), out of the middle of the block
        const long n = (long)(bytes / 3) - 2;
        const void* ptrs[3] = {src.data(), src.data() + bytes / 3, src.data() + 2 * (bytes / 3)};
        Guarded dst((size_t)n * 3);
        stage_planes(dst.body(), ptrs, 3, 1, 2, n);
        bool same = dst.guards_intact();
        for (int j = 0; j < 3 && same; ++j)
            same = std::memcmp(dst.body() + (size_t)j * n, (const unsigned char*)ptrs[j] + 2, (size_t)n) == 0;
        check(same, "fan-out: stage_planes");
    }
    // the pieces themselves tile [0, bytes) at 4 KiB boundaries.  (33 MiB over 8, 4 or 2 threads is a whole number of pages
    // each: the 7 odd bytes are the last piece's, and a share rounded down would drop them.)
    size_t total = 0;
    std::vector<std::pair<size_t, size_t>> pieces(64, {0, 0});
    fan_out(bytes, [&](size_t a, size_t b) { pieces[a >> 22] = {a, b}; });  // (pieces are above 4 MiB: distinct elements)
    for (const auto& pc : pieces) {
        if (pc.second == 0) continue;
        check(pc.first % 4096 == 0 && (pc.second % 4096 == 0 || pc.second == bytes), "fan-out: a piece off its 4 KiB boundary");
        total += pc.second - pc.first;
    }
    check(total == bytes, "fan-out: the pieces do not add up to the bytes");
}

}  // namespace

int main() {
    cuts();
    rows();
    bands();
    stored(false);
    stored(true);
    fan_out_once();
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::puts("host stage ok");
    return 0;
}
