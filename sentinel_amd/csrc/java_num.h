// java_num.h — the Java numeric conversions and the 64-bit mixing hash that bit-exact parity with the reference rests
// on, one copy for the kernels and the host side. Plain inline C++: __host__ __device__ under hipcc, and a host
// compiler without HIP takes it as it is (tests/cpp/test_java_num_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_HD __host__ __device__ __forceinline__
#else
#define SG_HD inline
#endif

namespace sg {

// (int) double, JLS §5.1.3: NaN → 0, saturate, truncate toward zero.
SG_HD int32_t java_d2i(double x) {
    if (x != x) return 0;
    if (x >= 2147483647.0) return INT32_MAX;
    if (x <= -2147483648.0) return INT32_MIN;
    return (int32_t)x;
}

// (long) double, JLS §5.1.3
SG_HD int64_t java_d2l(double x) {
    if (x != x) return 0;
    if (x >= 9223372036854775807.0) return INT64_MAX;
    if (x <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)x;
}

// java.lang.Math.round(double) (JDK 7u+): floor(a + 1/2) computed exactly on the bits; saturating.
SG_HD int64_t java_round(double a) {
    int64_t bits;
    __builtin_memcpy(&bits, &a, 8);
    const int64_t biased_exp = (bits & 0x7FF0000000000000LL) >> 52;
    const int64_t shift = (52 - 1 + 1023) - biased_exp;
    if ((shift & -64) == 0) {
        int64_t r = (bits & 0x000FFFFFFFFFFFFFLL) | 0x0010000000000000LL;
        if (bits < 0) r = -r;
        return ((r >> shift) + 1) >> 1;
    }
    return java_d2l(a);
}

// splitmix64's finaliser alone (a key that is already spread, or offset by the caller)
SG_HD uint64_t mix64_final(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint64_t kGoldenGamma = 0x9E3779B97F4A7C15ull;

// splitmix64 of z: the finaliser of z + golden gamma (sentinel_amd/cluster.py splitmix64 and
// sentinel_amd/param_wire.py _mix64 are the mirrors)
SG_HD uint64_t mix64(uint64_t z) { return mix64_final(z + kGoldenGamma); }

// The home slot of a value in an exact open-addressing table of mask + 1 slots: where its probe sequence starts.
SG_HD uint64_t table_home(uint64_t v, uint64_t mask) { return mix64(v) & mask; }

}  // namespace sg
