// TEST INFRASTRUCTURE: sentinel_amd/csrc/java_num.h on the CPU (no HIP, no GPU), built by java_num_host.mk with the
// address and undefined-behaviour sanitizers.
//   no arguments        the known answers of Math.round(double), (int) double and (long) double from their Java
//                       definitions; prints "java num host ok"
//   MASK X1 X2 ...      one line "X mix64(X) mix64_final(X) table_home(X, MASK)" per X (decimal or 0x… in, hex out),
//                       for tests/test_java_num_host.py to compare with the Python mirrors
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../sentinel_amd/csrc/java_num.h"

static int failures = 0;

static void expect(const char* what, double in, int64_t got, int64_t want) {
    if (got == want) return;
    std::printf("FAIL %s(%.17g) = %" PRId64 ", want %" PRId64 "\n", what, in, got, want);
    ++failures;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        const uint64_t mask = std::strtoull(argv[1], nullptr, 0);
        for (int i = 2; i < argc; ++i) {
            const uint64_t x = std::strtoull(argv[i], nullptr, 0);
            std::printf("0x%" PRIx64 " 0x%" PRIx64 " 0x%" PRIx64 " 0x%" PRIx64 "\n", x, sg::mix64(x), sg::mix64_final(x),
                        sg::table_home(x, mask));
        }
        return 0;
    }
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double p52 = 4503599627370496.0;  // 2^52
    const double p53 = 9007199254740992.0;  // 2^53

    // Math.round(double): floor(a + 1/2), saturating, NaN → 0
    struct { double in; int64_t want; } round_kat[] = {
        {0.5, 1}, {-0.5, 0}, {1.5, 2}, {2.5, 3}, {-1.5, -1}, {-2.5, -2},
        {0.49999999999999994, 0},
        {p52 + 1, 4503599627370497LL}, {-(p52 + 1), -4503599627370497LL}, {p53, 9007199254740992LL},
        {nan, 0},
        {inf, INT64_MAX}, {1e300, INT64_MAX}, {-inf, INT64_MIN}, {-1e300, INT64_MIN},
        {0.0, 0}, {-0.0, 0}, {1.0, 1}, {-1.0, -1}, {1e-320, 0}, {-0.49999999999999994, 0},
    };
    for (const auto& k : round_kat) expect("java_round", k.in, sg::java_round(k.in), k.want);

    // (int) double: NaN → 0, saturate, truncate toward zero
    struct { double in; int32_t want; } d2i_kat[] = {
        {nan, 0}, {inf, INT32_MAX}, {-inf, INT32_MIN}, {2147483647.5, INT32_MAX}, {-2147483648.9, INT32_MIN},
        {-0.9, 0}, {0.9, 0}, {-1.9, -1}, {1e19, INT32_MAX}, {2147483646.9, 2147483646}, {-2147483647.9, -2147483647},
    };
    for (const auto& k : d2i_kat) expect("java_d2i", k.in, sg::java_d2i(k.in), k.want);

    // (long) double
    struct { double in; int64_t want; } d2l_kat[] = {
        {nan, 0}, {inf, INT64_MAX}, {-inf, INT64_MIN}, {1e19, INT64_MAX}, {-1e19, INT64_MIN}, {-0.9, 0},
        {2147483647.5, 2147483647LL}, {-2147483648.9, -2147483648LL}, {p53, 9007199254740992LL},
        {9223372036854774784.0, 9223372036854774784LL},  // the largest double below 2^63
    };
    for (const auto& k : d2l_kat) expect("java_d2l", k.in, sg::java_d2l(k.in), k.want);

    if (failures) return 1;
    std::printf("java num host ok\n");
    return 0;
}
