// The byte arithmetic of the host pipeline's output lanes (sknnr_amd/csrc/host_stage.h, as sknnr_hip.hip includes it), alone
// on the CPU and under the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/lane_arithmetic_check.cpp -o /tmp/lane_check
//   /tmp/lane_check
//
// Three lanes (indices and distances of k = 5 columns, predictions of t = 3) at 4 / 4 / 1, 4 / 4 / 2 and 8 / 8 / 8 bytes per
// element, tiles of 1, 300 and 1024 rows.  The sizes and offsets are compared with values worked out by hand; then the
// tiles are written into heap arrays of exactly the caller's size, as rows and as planes, and every byte must have been
// written once -- an offset or a size that is off runs into the sanitizer or leaves a count that is not 1.
#define SKNNR_LANE_ARITHMETIC_ONLY
#include "../sknnr_amd/csrc/sknnr_hip.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int failures = 0;

void expect(size_t got, size_t want, const char* what, long n, int cols, size_t esz) {
    if (got == want) return;
    std::fprintf(stderr, "%s(n or c0 = %ld, cols = %d, esz = %zu) = %zu, expected %zu\n", what, n, cols, esz, got, want);
    ++failures;
}

constexpr int K = 5, T = 3;
constexpr long kTiles[] = {1, 300, 1024};
constexpr long kStarts[] = {0, 1, 301, 1325};  // where those tiles start in the caller's arrays, and where they end

struct Shape {
    int cols;
    size_t esz;
    size_t bytes[3], units[3];  // per tile
    size_t row_off[4], plane_off[4];  // per start
};
// (by hand: bytes = n * cols * esz; units = bytes / 8 rounded up; row_off = c0 * cols * esz; plane_off = c0 * esz)
const Shape kShapes[] = {
    {K, 4, {20, 6000, 20480}, {3, 750, 2560}, {0, 20, 6020, 26500}, {0, 4, 1204, 5300}},
    {K, 8, {40, 12000, 40960}, {5, 1500, 5120}, {0, 40, 12040, 53000}, {0, 8, 2408, 10600}},
    {T, 1, {3, 900, 3072}, {1, 113, 384}, {0, 3, 903, 3975}, {0, 1, 301, 1325}},
    {T, 2, {6, 1800, 6144}, {1, 225, 768}, {0, 6, 1806, 7950}, {0, 2, 602, 2650}},
    {T, 8, {24, 7200, 24576}, {3, 900, 3072}, {0, 24, 7224, 31800}, {0, 8, 2408, 10600}},
};

// Every tile of a lane into an array of the caller's exact size, one count per byte written.
void walk(const Shape& s, bool planes) {
    const long total = kStarts[3];
    std::vector<unsigned char> hits((size_t)total * s.cols * s.esz, 0);
    for (int i = 0; i < 3; ++i) {
        const long n = kTiles[i];
        unsigned char* at = hits.data() + lane_tile_offset(kStarts[i], s.cols, s.esz, planes);
        if (!planes) {
            for (size_t b = 0; b < lane_bytes(n, s.cols, s.esz); ++b) ++at[b];
            continue;
        }
        for (int j = 0; j < s.cols; ++j)  // (plane j of the tile: n elements, `total` elements after plane j - 1)
            for (size_t b = 0; b < (size_t)n * s.esz; ++b) ++at[(size_t)j * total * s.esz + b];
    }
    for (size_t b = 0; b < hits.size(); ++b)
        if (hits[b] != 1) {
            std::fprintf(stderr, "cols = %d, esz = %zu, %s: byte %zu written %d times\n", s.cols, s.esz,
                         planes ? "planes" : "rows", b, hits[b]);
            ++failures;
            return;
        }
}

}  // namespace

int main() {
    static_assert(kLaneIdx == 0 && kLaneDist == 1 && kLanePred == 2 && kLanes == 3, "the debug records' bit order");
    for (const Shape& s : kShapes) {
        for (int i = 0; i < 3; ++i) {
            expect(lane_bytes(kTiles[i], s.cols, s.esz), s.bytes[i], "lane_bytes", kTiles[i], s.cols, s.esz);
            expect(lane_units(kTiles[i], s.cols, s.esz), s.units[i], "lane_units", kTiles[i], s.cols, s.esz);
            // (the pinned and narrow buffers hold `units` 8-byte words: never fewer bytes than the copy moves, never 8 more)
            const size_t room = 8 * lane_units(kTiles[i], s.cols, s.esz);
            if (room < s.bytes[i] || room >= s.bytes[i] + 8) {
                std::fprintf(stderr, "units of n = %ld, cols = %d, esz = %zu do not fit its bytes\n", kTiles[i], s.cols, s.esz);
                ++failures;
            }
        }
        for (int i = 0; i < 4; ++i) {
            expect(lane_tile_offset(kStarts[i], s.cols, s.esz, false), s.row_off[i], "lane_tile_offset rows", kStarts[i], s.cols, s.esz);
            expect(lane_tile_offset(kStarts[i], s.cols, s.esz, true), s.plane_off[i], "lane_tile_offset planes", kStarts[i], s.cols, s.esz);
        }
        walk(s, false);
        walk(s, true);
    }
    // beyond 32 bits: a 10^9-row call's last tile, 40 targets of 8 bytes
    expect(lane_tile_offset(999000000L, 40, 8, false), 319680000000ULL, "lane_tile_offset rows", 999000000L, 40, 8);
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::puts("lane arithmetic ok: 5 shapes x 3 tiles, rows and planes");
    return 0;
}
