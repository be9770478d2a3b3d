// blocklog_rules.h — LogSlot's per-resource limitApp table and its host-side compiler. No HIP in here: the device
// reads the int32 table (engine.h includes this file), sg_local_load_flow_rules computes it, and
// tests/cpp/test_blocklog_host.cpp runs it on the CPU.
//
// LogSlot.entry (core/slots/logger/LogSlot.java:35-47) logs e.getRuleLimitApp() of every BlockException. For a
// FlowException that is rule.getLimitApp() of the rule that failed (FlowRuleChecker.java:53). When every flow rule the
// device checks for a resource carries one limitApp, that value is the answer whichever rule failed, and the walkers
// have nothing to report; only a resource whose rules name several limitApps (kBlogMixed) needs the failing rule from
// cx_entry. The resources of the lane walkers (one "default" DIRECT rule, LRule::fr_n == 0) and resources with no flow
// rule at all are uniform "default".
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/sentinel_gpu.h"

namespace sg {

constexpr int32_t kBlogMixed = INT32_MIN;  // the resource's rules name several limitApps (never a limit_app value)

// The table over the rules the device checks: kept[r] lists resource r's rule indices after the load-time drops
// (invalid rules, SG_CLUSTER_MODE_INVALID, duplicates), in any order — FlowRuleComparator reorders a resource's rules
// but never changes their set. Cluster-mode rules count like any other: the embedded server's BLOCKED answer and the
// local fallback both throw with the rule's own limitApp. app[K] = the one limitApp, SG_LIMIT_APP_DEFAULT for a
// resource without rules, or kBlogMixed.
inline void blocklog_limit_apps(const sg_local_flow_rule* rules, const std::vector<std::vector<uint32_t>>& kept,
                                std::vector<int32_t>& app) {
    app.assign(kept.size(), SG_LIMIT_APP_DEFAULT);
    for (size_t k = 0; k < kept.size(); ++k) {
        const std::vector<uint32_t>& v = kept[k];
        if (v.empty()) continue;
        int32_t one = rules[v[0]].limit_app;
        for (uint32_t i : v)
            if (rules[i].limit_app != one) one = kBlogMixed;
        app[k] = one;
    }
}

}  // namespace sg
