// TEST INFRASTRUCTURE: the host-only size arithmetic and refusal order of the in-place table growth
// (sentinel_amd/csrc/table_grow.h) on the CPU, with its own main: no GPU, no HIP. Built by table_grow_host.mk with the
// address and undefined-behaviour sanitizers; run by tests/test_table_grow_abi.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sentinel_amd/csrc/table_grow.h"

using namespace sg;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static std::vector<uint64_t> masks(std::initializer_list<int> lg) {
    std::vector<uint64_t> m;
    for (int x : lg) m.push_back((1ull << x) - 1);
    return m;
}

static void param_plans() {
    const auto cur = masks({1, 4, 2});
    const uint64_t mb = 1 << 15;
    {  // sizes kept, grown and mixed: bases are running sums of 2^lg + 1
        const int32_t want[3] = {0, 5, 0};
        const GrowPlan p = grow_plan_param(cur, want, 3, mb, true);
        CHECK(p.code == SG_OK);
        CHECK(p.mask[0] == 1 && p.mask[1] == 31 && p.mask[2] == 3);
        CHECK(p.base[0] == 0 && p.base[1] == 3 && p.base[2] == 36);
        CHECK(p.total == 3 + 33 + 5);
    }
    {  // a call of zeros is a plan too (compaction): the layout in force
        const int32_t want[3] = {0, 0, 0};
        const GrowPlan p = grow_plan_param(cur, want, 3, mb, false);
        CHECK(p.code == SG_OK && p.total == 3 + 17 + 5 && p.base[2] == 20);
    }
    {  // the same size named outright
        const int32_t want[3] = {1, 4, 2};
        CHECK(grow_plan_param(cur, want, 3, mb, false).code == SG_OK);
    }
    const int32_t one[3] = {2, 0, 0};
    CHECK(grow_plan_param({}, one, 3, mb, false).code == SG_E_INVAL);      // before a load
    CHECK(grow_plan_param({}, nullptr, 0, mb, false).code == SG_E_INVAL);
    CHECK(grow_plan_param(cur, one, 2, mb, false).code == SG_E_INVAL);     // a wrong n
    CHECK(grow_plan_param(cur, one, 4, mb, false).code == SG_E_INVAL);
    CHECK(grow_plan_param(cur, nullptr, 3, mb, false).code == SG_E_INVAL);
    {
        const int32_t shrink[3] = {0, 3, 0}, low[3] = {-1, 0, 0}, high[3] = {0, 0, 31};
        CHECK(grow_plan_param(cur, shrink, 3, mb, false).code == SG_E_INVAL);
        CHECK(grow_plan_param(cur, low, 3, mb, false).code == SG_E_INVAL);
        CHECK(grow_plan_param(cur, high, 3, mb, false).code == SG_E_INVAL);
    }
    {  // 2^32 slots or more; the arguments are judged first
        const auto four = masks({1, 1, 1, 1});
        const int32_t big[4] = {30, 30, 30, 30}, bad[4] = {30, 30, 30, 31};
        CHECK(grow_plan_param(four, big, 4, mb, false).code == SG_E_UNSUPPORTED);
        CHECK(grow_plan_param(four, bad, 4, mb, false).code == SG_E_INVAL);
        const int32_t three[4] = {30, 30, 30, 0};  // 3 * 2^30 + 6 slots: 32 slot bits
        CHECK(grow_plan_param(four, three, 4, 1 << 16, false).code == SG_OK);               // 16 + 8 + 32
        CHECK(grow_plan_param(four, three, 4, 1ull << 24, false).code == SG_OK);            // 24 + 8 + 32 = 64
        CHECK(grow_plan_param(four, three, 4, (1ull << 24) + 2, false).code == SG_E_UNSUPPORTED);  // 25 index bits
        CHECK(grow_plan_param(four, three, 4, 1 << 16, true).code == SG_OK);                // below 0xFFFFFFFC
        const int32_t most[4] = {30, 30, 30, 29};  // 3.5 * 2^30 + 4: still 32 bits, still below the codes
        CHECK(grow_plan_param(four, most, 4, 1 << 16, true).code == SG_OK);
    }
}

static void cparam_plans() {
    const uint64_t mb = 1 << 15;
    {
        const GrowPlan p = grow_plan_cparam(3, 3, 3, mb);
        CHECK(p.code == SG_OK && p.total == 27 && p.base[1] == 9 && p.base[2] == 18 && p.mask[2] == 7);
    }
    CHECK(grow_plan_cparam(3, 3, 2, mb).code == SG_OK);              // the same size: a compaction
    CHECK(grow_plan_cparam(0, 0, 4, mb).code == SG_E_INVAL);         // before a load
    CHECK(grow_plan_cparam(3, 3, 1, mb).code == SG_E_INVAL);         // a shrink
    CHECK(grow_plan_cparam(3, 3, 0, mb).code == SG_E_INVAL);
    CHECK(grow_plan_cparam(3, 3, 29, mb).code == SG_E_INVAL);
    CHECK(grow_plan_cparam(3, 3, -7, mb).code == SG_E_INVAL);
    CHECK(grow_plan_cparam(16, 3, 28, mb).code == SG_E_UNSUPPORTED); // 16 * (2^28 + 1) >= 2^32
    CHECK(grow_plan_cparam(15, 3, 28, mb).code == SG_OK);            // 32 slot bits, 24 id bits, 16 needed
    CHECK(grow_plan_cparam(15, 3, 28, (1ull << 24) - 1).code == SG_OK);
    CHECK(grow_plan_cparam(15, 3, 28, 1ull << 24).code == SG_E_UNSUPPORTED);  // 25 id bits do not fit
}

static void vdict_plans() {
    CHECK(grow_plan_vdict(false, 0, 0, 8, 0).code == SG_E_INVAL);
    CHECK(grow_plan_vdict(true, 64, 100, 6, 100).code == SG_OK);     // both as they are
    CHECK(grow_plan_vdict(true, 64, 100, 6, 200).code == SG_OK);     // the arena alone
    CHECK(grow_plan_vdict(true, 64, 100, 8, 100).total == 256);
    CHECK(grow_plan_vdict(true, 64, 100, 5, 100).code == SG_E_INVAL);
    CHECK(grow_plan_vdict(true, 64, 100, 6, 99).code == SG_E_INVAL);
    CHECK(grow_plan_vdict(true, 64, 100, 29, 100).code == SG_E_INVAL);
    CHECK(grow_plan_vdict(true, 64, 100, 0, 100).code == SG_E_INVAL);
    CHECK(grow_plan_vdict(true, 1ull << 28, 0, 28, 0).code == SG_OK);
}

int main() {
    param_plans();
    cparam_plans();
    vdict_plans();
    std::printf("table grow host ok\n");
    return 0;
}
