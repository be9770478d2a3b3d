// TEST INFRASTRUCTURE: the host-only per-resource limitApp table of LogSlot's rollup
// (sentinel_amd/csrc/blocklog_rules.h) on the CPU, under the address and undefined-behaviour sanitizers. No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sentinel_amd/csrc/blocklog_rules.h"

using namespace sg;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static sg_local_flow_rule rule(uint32_t res, int32_t app, int32_t cluster_mode = SG_CLUSTER_MODE_OFF) {
    sg_local_flow_rule r{};
    r.resource = res;
    r.grade = 1;
    r.count = 10.0;
    r.limit_app = app;
    r.ref_resource = -1;
    r.cluster_mode = cluster_mode;
    return r;
}

// The kept rule lists as the library hands them to blocklog_limit_apps, reduced to what these cases vary: a rule of a
// resource index >= K or with cluster_mode SG_CLUSTER_MODE_INVALID is dropped at load (sg_local_load_flow_rules also
// drops the other invalid rules and duplicates; a duplicate shares its limitApp, so it cannot change the table).
static void group_rules(const sg_local_flow_rule* rules, uint32_t n, uint32_t K,
                        std::vector<std::vector<uint32_t>>& kept) {
    kept.assign(K, {});
    for (uint32_t i = 0; i < n; ++i) {
        if (rules[i].resource >= K || rules[i].cluster_mode == SG_CLUSTER_MODE_INVALID) continue;
        kept[rules[i].resource].push_back(i);
    }
}

static std::vector<int32_t> table(const std::vector<sg_local_flow_rule>& rules, uint32_t K) {
    std::vector<std::vector<uint32_t>> kept;
    group_rules(rules.data(), (uint32_t)rules.size(), K, kept);
    CHECK(kept.size() == K);
    std::vector<int32_t> app;
    blocklog_limit_apps(rules.data(), kept, app);
    CHECK(app.size() == K);
    return app;
}

int main() {
    const int32_t D = SG_LIMIT_APP_DEFAULT, O = SG_LIMIT_APP_OTHER;
    {  // no rules at all, and no resources
        CHECK(table({}, 0).empty());
        const std::vector<int32_t> a = table({}, 3);
        CHECK(a[0] == D && a[1] == D && a[2] == D);
    }
    {  // one rule: its limitApp, whatever it is
        CHECK(table({rule(0, D)}, 1)[0] == D);
        CHECK(table({rule(0, O)}, 1)[0] == O);
        CHECK(table({rule(0, 7)}, 1)[0] == 7);
    }
    {  // equal limitApps are uniform, different ones are mixed — per resource
        const std::vector<int32_t> a =
            table({rule(0, D), rule(0, D), rule(1, 3), rule(1, 3), rule(2, D), rule(2, 3), rule(3, O), rule(3, D),
                   rule(4, 1), rule(4, 2)}, 6);
        CHECK(a[0] == D && a[1] == 3);
        CHECK(a[2] == kBlogMixed && a[3] == kBlogMixed && a[4] == kBlogMixed);
        CHECK(a[5] == D);  // a resource without rules
    }
    {  // order does not matter (FlowRuleComparator only reorders)
        CHECK(table({rule(0, 3), rule(0, D), rule(0, 3)}, 1)[0] == kBlogMixed);
        CHECK(table({rule(0, D), rule(0, 3), rule(0, 3)}, 1)[0] == kBlogMixed);
    }
    {  // rules dropped at load do not count: the resource stays uniform
        const std::vector<int32_t> a =
            table({rule(0, D), rule(0, 5, SG_CLUSTER_MODE_INVALID), rule(1, 5, SG_CLUSTER_MODE_INVALID), rule(9, 5)}, 2);
        CHECK(a[0] == D);
        CHECK(a[1] == D);  // its only rule was dropped: no rule
    }
    {  // cluster-mode rules count like local ones (BLOCKED and the fallback throw with the rule's limitApp)
        const std::vector<int32_t> a = table({rule(0, D), rule(0, 2, SG_CLUSTER_MODE_FALLBACK), rule(1, 2),
                                              rule(1, 2, SG_CLUSTER_MODE_NO_FALLBACK)}, 2);
        CHECK(a[0] == kBlogMixed && a[1] == 2);
    }
    {  // a resource index at K - 1, and one at K (dropped)
        const uint32_t K = 1000;
        const std::vector<int32_t> a = table({rule(K - 1, O), rule(K - 1, 4), rule(K, 4)}, K);
        CHECK(a[K - 1] == kBlogMixed && a[K - 2] == D && a[0] == D);
    }
    {  // kBlogMixed is no limit_app value
        CHECK(kBlogMixed != D && kBlogMixed != O && kBlogMixed < 0);
    }
    std::printf("blocklog host ok\n");
    return 0;
}
