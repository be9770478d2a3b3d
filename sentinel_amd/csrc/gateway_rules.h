// gateway_rules.h — GatewayFlowSlot's host side and the one function host and device share: which gateway rules are
// kept (GatewayRuleManager.isValidRule), how they become ParamFlowRules and the parser's per-resource tables
// (GatewayRuleManager.applyGatewayRuleInternal, GatewayRuleConverter), and gw_match (GatewayParamParser
// .parseWithMatchStrategyInternal). No HIP in here beyond the host/device marker: engine.h's users include it,
// gateway.hip calls gw_match per item, the C ABI runs the conversion, and tests/cpp/test_gateway_host.cpp runs all
// of it on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/sentinel_gpu.h"

#if defined(__HIPCC__)
#define SG_GW_HD __host__ __device__
#else
#define SG_GW_HD
#endif

namespace sg {

struct GwRes {               // the parser's view of one resource
    uint32_t rule_begin;     // its item rules: GwItemRule[rule_begin, rule_begin + n_items), by paramIdx
    uint32_t n_items;
    uint32_t has_item_less;  // → a last "$D" arg
    uint32_t reserved;
};

struct GwItemRule {          // what parseParameterFor reads of an item rule
    int32_t resource_mode;
    int32_t parse_strategy;
    int32_t match_strategy;
    uint32_t pat_off;        // into the pattern blob; pat_len 0 = null or empty: the value is kept
    uint32_t pat_len;
};

// isValidRule / isValidParamItem. The resource name is the caller's index, so "blank resource" cannot occur.
inline bool gw_valid_rule(const sg_gateway_rule& r) {
    if (r.resource_mode < 0 || r.grade < 0 || r.count < 0 || r.burst < 0 || r.control_behavior < 0) return false;
    if (r.control_behavior == 2 && r.max_queueing_timeout_ms < 0) return false;  // CONTROL_BEHAVIOR_RATE_LIMITER
    if (r.interval_sec <= 0) return false;
    if (!r.has_item) return true;
    if (r.parse_strategy < 0) return false;
    const bool field_required = r.parse_strategy == SG_GW_PARSE_HEADER || r.parse_strategy == SG_GW_PARSE_URL_PARAM ||
                                r.parse_strategy == SG_GW_PARSE_COOKIE;
    if (field_required && r.field_blank) return false;
    const bool pattern_empty = r.pattern_null || r.pattern_len == 0;  // StringUtil.isEmpty
    return pattern_empty || r.match_strategy >= 0;
}

// parseWithMatchStrategyInternal for a non-null value: true keeps the value, false makes it "$NM". regex_flag is the
// caller's java.util.regex verdict (true also for a pattern that did not compile). PREFIX has no case in the
// reference's switch: it and every unknown strategy fall to `default: return value`.
SG_GW_HD inline bool gw_match(int32_t match_strategy, const uint8_t* value, uint32_t len, const uint8_t* pattern,
                              uint32_t plen, bool regex_flag) {
    if (plen == 0) return true;  // StringUtil.isEmpty(pattern): the strategy is not consulted
    switch (match_strategy) {
        case SG_GW_MATCH_EXACT: {
            if (len != plen) return false;
            for (uint32_t k = 0; k < len; ++k)
                if (value[k] != pattern[k]) return false;
            return true;
        }
        case SG_GW_MATCH_CONTAINS: {
            if (plen > len) return false;
            for (uint32_t s = 0; s + plen <= len; ++s) {
                uint32_t k = 0;
                while (k < plen && value[s + k] == pattern[k]) ++k;
                if (k == plen) return true;
            }
            return false;
        }
        case SG_GW_MATCH_REGEX: return regex_flag;
        default: return true;
    }
}

// ParamFlowRule.equals over what a converted item-less rule can differ in (Double.compare for the count).
inline bool gw_same_converted(const sg_gateway_rule& a, const sg_gateway_rule& b) {
    const bool same_count = (std::isnan(a.count) && std::isnan(b.count)) ||
                            (a.count == b.count && std::signbit(a.count) == std::signbit(b.count));
    return same_count && a.grade == b.grade && a.interval_sec == b.interval_sec && a.burst == b.burst &&
           a.control_behavior == b.control_behavior && a.max_queueing_timeout_ms == b.max_queueing_timeout_ms;
}

struct GwConverted {
    std::vector<sg_pslot_rule> rules;     // sorted by (resource, paramIdx, caller order)
    std::vector<sg_param_hot_item> hot;
    std::vector<uint32_t> source;         // rules[i] came from gateway rule source[i]
    std::vector<GwRes> res;               // [n_resources]
    std::vector<GwItemRule> items;
};

// A pattern range outside the blob or a resource >= n_resources: false (nothing else can fail).
inline bool gw_ranges_ok(const sg_gateway_rule* rules, uint32_t n, uint64_t n_pattern_bytes, uint32_t n_resources) {
    for (uint32_t i = 0; i < n; ++i) {
        const sg_gateway_rule& r = rules[i];
        if (r.resource >= n_resources) return false;
        if (r.has_item && !r.pattern_null && (uint64_t)r.pattern_off + r.pattern_len > n_pattern_bytes) return false;
    }
    return true;
}

inline sg_pslot_rule gw_to_param_rule(const sg_gateway_rule& g, int32_t idx) {  // applyToParamRule without the item
    sg_pslot_rule p{};
    p.rule.count = g.count;
    p.rule.duration_sec = g.interval_sec;
    p.rule.burst = g.burst;
    p.rule.behavior = g.control_behavior;
    p.rule.max_queueing_ms = g.max_queueing_timeout_ms;
    p.rule.capacity_log2 = g.capacity_log2;
    p.resource = g.resource;
    p.param_idx = idx;
    p.grade = g.grade;
    return p;
}

// applyGatewayRuleInternal over rules that passed gw_ranges_ok; nm_id = the value id of "$NM".
inline GwConverted gw_convert(const sg_gateway_rule* rules, uint32_t n, uint32_t n_resources, uint64_t nm_id) {
    GwConverted c;
    c.res.assign(n_resources, GwRes{0, 0, 0, 0});
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return rules[a].resource < rules[b].resource; });
    size_t at = 0;
    while (at < order.size()) {
        const uint32_t resource = rules[order[at]].resource;
        size_t end = at;
        while (end < order.size() && rules[order[end]].resource == resource) ++end;
        GwRes& gr = c.res[resource];
        gr.rule_begin = (uint32_t)c.items.size();
        for (size_t k = at; k < end; ++k) {  // applyToParamRule: 0, 1, 2, … in the caller's order
            const sg_gateway_rule& g = rules[order[k]];
            if (!gw_valid_rule(g) || !g.has_item) continue;
            sg_pslot_rule p = gw_to_param_rule(g, (int32_t)gr.n_items);
            if (!g.pattern_null) {  // generateNonMatchPassParamItem, for an empty pattern too
                p.rule.hot_begin = (uint32_t)c.hot.size();
                p.rule.hot_count = 1;
                c.hot.push_back(sg_param_hot_item{nm_id, SG_GW_NM_THRESHOLD, 0});
            }
            const bool keep_value = g.pattern_null || g.pattern_len == 0;
            c.items.push_back(GwItemRule{g.resource_mode, g.parse_strategy, g.match_strategy,
                                         keep_value ? 0u : g.pattern_off, keep_value ? 0u : g.pattern_len});
            c.rules.push_back(p);
            c.source.push_back(order[k]);
            ++gr.n_items;
        }
        const size_t first_item_less = c.rules.size();
        for (size_t k = at; k < end; ++k) {  // applyNonParamToParamRule: all on the last index, equal ones once
            const sg_gateway_rule& g = rules[order[k]];
            if (!gw_valid_rule(g) || g.has_item) continue;
            gr.has_item_less = 1;
            bool seen = false;
            for (size_t j = first_item_less; j < c.rules.size() && !seen; ++j)
                seen = gw_same_converted(rules[c.source[j]], g);
            if (seen) continue;
            c.rules.push_back(gw_to_param_rule(g, (int32_t)gr.n_items));
            c.source.push_back(order[k]);
        }
        at = end;
    }
    return c;
}

}  // namespace sg
