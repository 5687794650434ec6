// The four distance-weight laws as the device evaluates them (weight_law_value of sknnr_amd/csrc/weights.hip.h, which is
// host-callable), alone on the CPU and under the sanitizers, against values numpy wrote:
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all scripts/weight_law_check.cpp -o /tmp/weight_law_check
//   /tmp/weight_law_check tests/golden/weight_laws.txt
//
// (-O3 and -ffp-contract=off are the library's own flags: the point is that these expressions, so compiled, round as
// numpy's do.)  Every line of the fixture is "law p0 d w": the sknnr_weight_law code, then three float64 bit patterns
// in hex; tests/test_weight_laws_cpu.py checks that the lines are what sknnr_amd.weights gives.  The program also
// evaluates a plain C++ restatement of its own, written without the header's helper, and expects the same bits.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sknnr_amd/csrc/weights.hip.h"

namespace {

double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

uint64_t to_bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// the table of sknnr_amd/weights.py, operation by operation (volatile: nothing is folded or fused across statements)
double restated(int law, double p, double d) {
    volatile double a, b;
    switch (law) {
        case 1:
            a = p + d;
            return 1.0 / a;
        case 2:
            a = d * d;
            b = p + a;
            return 1.0 / b;
        case 3:
            a = d / p;
            b = 1.0 - a;
            return b > 0.0 ? b : 0.0;
        default:
            a = d / p;
            b = a * a;
            a = 1.0 - b;
            return a > 0.0 ? a : 0.0;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s tests/golden/weight_laws.txt\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    struct Row {
        int law;
        uint64_t p0, d, w;
    };
    std::vector<Row> rows;
    char line[256];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        Row r{};
        if (std::sscanf(line, "%d %" SCNx64 " %" SCNx64 " %" SCNx64, &r.law, &r.p0, &r.d, &r.w) != 4) {
            std::fprintf(stderr, "bad line: %s", line);
            std::fclose(f);
            return 2;
        }
        rows.push_back(r);
    }
    std::fclose(f);
    int failures = 0, seen[sknnr::kLawCount] = {};
    for (const Row& r : rows) {
        if (r.law <= sknnr::kLawNone || r.law >= sknnr::kLawCount) {
            std::fprintf(stderr, "law %d is no law\n", r.law);
            return 2;
        }
        ++seen[r.law];
        const double p0 = from_bits(r.p0), d = from_bits(r.d);
        const uint64_t got = to_bits(sknnr::weight_law_value(r.law, p0, 0.0, d)), mine = to_bits(restated(r.law, p0, d));
        if (got != r.w || mine != r.w) {
            std::fprintf(stderr, "law %d p0 %a d %a: header %016" PRIx64 ", restated %016" PRIx64 ", numpy %016" PRIx64 "\n",
                         r.law, p0, d, got, mine, r.w);
            ++failures;
        }
    }
    for (int law = 1; law < sknnr::kLawCount; ++law)
        if (!seen[law]) {
            std::fprintf(stderr, "no line for law %d\n", law);
            ++failures;
        }
    std::printf("%zu values, %d failures\n", rows.size(), failures);
    return failures ? 1 : 0;
}
