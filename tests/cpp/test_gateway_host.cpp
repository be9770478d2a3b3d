// TEST INFRASTRUCTURE: GatewayFlowSlot's host side (sentinel_amd/csrc/gateway_rules.h) on the CPU, built with the
// address and undefined-behaviour sanitizers by tests/cpp/gateway_host.mk: rule validity, the conversion to
// ParamFlowRules and the parser's tables, and gw_match, through the adapter's JUnit expectations and the edges the
// device kernels rely on. `test_gateway_host convert <rules.bin> <n_resources> <nm_id> <out.bin>` runs the conversion
// over a file of sg_gateway_rule records for tests/test_gateway_abi.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../sentinel_amd/csrc/gateway_rules.h"

using namespace sg;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static std::string blob;  // the pattern blob of the rules below

static sg_gateway_rule rule(uint32_t resource, double count) {  // new GatewayFlowRule(resource).setCount(count)
    sg_gateway_rule r{};
    r.resource = resource;
    r.count = count;
    r.grade = 1;
    r.interval_sec = 1;
    r.max_queueing_timeout_ms = 500;
    r.pattern_null = 1;
    return r;
}

// .setParamItem(new GatewayParamFlowItem().setParseStrategy(..).setFieldName(..).setPattern(..).setMatchStrategy(..))
static sg_gateway_rule with_item(sg_gateway_rule r, int32_t parse, bool field_blank, const char* pattern = nullptr,
                                 int32_t match = SG_GW_MATCH_EXACT) {
    r.has_item = 1;
    r.parse_strategy = parse;
    r.field_blank = field_blank;
    r.match_strategy = match;
    r.pattern_null = pattern == nullptr;
    if (pattern) {
        r.pattern_off = (uint32_t)blob.size();
        r.pattern_len = (uint32_t)std::strlen(pattern);
        blob += pattern;
    }
    return r;
}

static bool match(int32_t strategy, const std::string& value, const std::string& pattern, bool verdict = false) {
    // copies of exactly the string's size: a read past either end is the sanitizer's to report
    std::vector<uint8_t> v(value.begin(), value.end()), p(pattern.begin(), pattern.end());
    return gw_match(strategy, v.data(), (uint32_t)v.size(), p.data(), (uint32_t)p.size(), verdict);
}

// parseParameterFor over the converted tables, as the kernels read them: "" stands for an emptied array, else one
// string per arg ("<null>" for a null arg)
struct RawItem {
    const char* value;  // nullptr: the RequestItemParser returned null
    bool verdict;
};
static std::vector<std::string> parse(const GwConverted& c, uint32_t resource, int32_t mode,
                                      const std::vector<RawItem>& raw) {
    std::vector<std::string> out;
    const GwRes gr = resource < c.res.size() ? c.res[resource] : GwRes{0, 0, 0, 0};
    CHECK(raw.size() == gr.n_items);
    for (uint32_t k = 0; k < gr.n_items; ++k)
        if (c.items[gr.rule_begin + k].resource_mode != mode) return out;
    for (uint32_t k = 0; k < gr.n_items; ++k) {
        const GwItemRule& ir = c.items[gr.rule_begin + k];
        if (!raw[k].value || (uint32_t)ir.parse_strategy > SG_GW_PARSE_COOKIE) {
            out.push_back("<null>");
            continue;
        }
        const std::string v = raw[k].value;
        const bool keep = gw_match(ir.match_strategy, (const uint8_t*)v.data(), (uint32_t)v.size(),
                                   (const uint8_t*)blob.data() + ir.pat_off, ir.pat_len, raw[k].verdict);
        out.push_back(keep ? v : "$NM");
    }
    if (gr.has_item_less) out.push_back("$D");
    return out;
}

static int convert_file(const char* in, uint32_t n_resources, uint64_t nm_id, const char* outp) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<sg_gateway_rule> rules;
    sg_gateway_rule r;
    while (std::fread(&r, sizeof r, 1, f) == 1) rules.push_back(r);
    std::fclose(f);
    if (!gw_ranges_ok(rules.data(), (uint32_t)rules.size(), 1ull << 31, n_resources)) return 3;
    const GwConverted c = gw_convert(rules.data(), (uint32_t)rules.size(), n_resources, nm_id);
    std::FILE* o = std::fopen(outp, "wb");
    if (!o) return 2;
    const uint32_t head[4] = {(uint32_t)c.rules.size(), (uint32_t)c.hot.size(), (uint32_t)c.res.size(),
                              (uint32_t)c.items.size()};
    auto put = [&](const void* p, size_t size, size_t n) {  // an empty vector's data() may be null
        if (n) std::fwrite(p, size, n, o);
    };
    put(head, sizeof head, 1);
    put(c.rules.data(), sizeof(sg_pslot_rule), c.rules.size());
    put(c.hot.data(), sizeof(sg_param_hot_item), c.hot.size());
    put(c.source.data(), sizeof(uint32_t), c.source.size());
    put(c.res.data(), sizeof(GwRes), c.res.size());
    put(c.items.data(), sizeof(GwItemRule), c.items.size());
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && std::strcmp(argv[1], "convert") == 0)
        return convert_file(argv[2], (uint32_t)std::strtoul(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                            argv[5]);
    static_assert(sizeof(sg_gateway_rule) == 72 && sizeof(sg_gateway_req) == 16 && sizeof(sg_gateway_item) == 16, "");
    static_assert(sizeof(GwRes) == 16 && sizeof(GwItemRule) == 20, "");

    {  // GatewayRuleManagerTest.testIsValidRule (bad1, a rule without a resource, has no counterpart: resources are indices)
        sg_gateway_rule bad2 = rule(0, 0);
        bad2.interval_sec = 0;
        const sg_gateway_rule bad3 = with_item(rule(0, 0), SG_GW_PARSE_URL_PARAM, true);
        const sg_gateway_rule bad4 = with_item(rule(0, 0), SG_GW_PARSE_URL_PARAM, false, "def", -1);
        const sg_gateway_rule good1 = rule(0, 0);
        const sg_gateway_rule good2 = with_item(rule(0, 0), 0, true);
        const sg_gateway_rule good3 = with_item(rule(0, 0), SG_GW_PARSE_CLIENT_IP, false, "def", SG_GW_PARSE_HEADER);
        CHECK(!gw_valid_rule(bad2) && !gw_valid_rule(bad3) && !gw_valid_rule(bad4));
        CHECK(gw_valid_rule(good1) && gw_valid_rule(good2) && gw_valid_rule(good3));
    }
    {  // every validity branch, one field at a time
        sg_gateway_rule r = rule(0, 1);
        CHECK(gw_valid_rule(r));
        r = rule(0, 1), r.resource_mode = -1;
        CHECK(!gw_valid_rule(r));
        r = rule(0, 1), r.grade = -1;
        CHECK(!gw_valid_rule(r));
        r = rule(0, -0.5);
        CHECK(!gw_valid_rule(r));
        r = rule(0, 1), r.burst = -1;
        CHECK(!gw_valid_rule(r));
        r = rule(0, 1), r.control_behavior = -1;
        CHECK(!gw_valid_rule(r));
        r = rule(0, 1), r.control_behavior = 2, r.max_queueing_timeout_ms = -1;
        CHECK(!gw_valid_rule(r));
        r = rule(0, 1), r.control_behavior = 0, r.max_queueing_timeout_ms = -1;  // read by the rate limiter only
        CHECK(gw_valid_rule(r));
        r = rule(0, 1), r.control_behavior = 2, r.max_queueing_timeout_ms = 0;
        CHECK(gw_valid_rule(r));
        r = rule(0, 1), r.interval_sec = -3;
        CHECK(!gw_valid_rule(r));
        r = rule(0, 1), r.grade = 7, r.resource_mode = 5;  // only negative values are refused
        CHECK(gw_valid_rule(r));
        r = rule(0, 1), r.parse_strategy = -1, r.match_strategy = -1, r.field_blank = 1;  // no item: its fields are unread
        CHECK(gw_valid_rule(r));
        CHECK(!gw_valid_rule(with_item(rule(0, 1), -1, false)));
        for (int32_t parse = 0; parse <= 9; ++parse) {
            const bool required = parse == SG_GW_PARSE_HEADER || parse == SG_GW_PARSE_URL_PARAM || parse == SG_GW_PARSE_COOKIE;
            CHECK(gw_valid_rule(with_item(rule(0, 1), parse, true)) == !required);
            CHECK(gw_valid_rule(with_item(rule(0, 1), parse, false)));
        }
        CHECK(gw_valid_rule(with_item(rule(0, 1), 0, false, nullptr, -1)));  // null pattern: the strategy is unread
        CHECK(gw_valid_rule(with_item(rule(0, 1), 0, false, "", -1)));       // empty pattern: the same
        CHECK(!gw_valid_rule(with_item(rule(0, 1), 0, false, "x", -1)));
        CHECK(gw_valid_rule(with_item(rule(0, 1), 0, false, "x", 7)));
    }
    {  // gw_match
        const int E = SG_GW_MATCH_EXACT, C = SG_GW_MATCH_CONTAINS, R = SG_GW_MATCH_REGEX, P = SG_GW_MATCH_PREFIX;
        CHECK(match(E, "Wow", "Wow") && !match(E, "Wow_foo", "Wow") && !match(E, "Wo", "Wow") && !match(E, "wow", "Wow"));
        CHECK(!match(E, "", "a") && match(E, "a", "a") && !match(E, "b", "a"));
        CHECK(!match(C, "ab", "abc"));                       // pattern longer than the value
        CHECK(match(C, "abc", "abc"));                       // equal to it
        CHECK(match(C, "abcdef", "abc"));                    // at the start
        CHECK(match(C, "defabc", "abc"));                    // at the end
        CHECK(match(C, "aaab", "aab") && !match(C, "aaac", "aab"));
        CHECK(!match(C, "", "a") && match(C, "a", "a") && !match(C, "b", "a"));
        CHECK(match(C, "warn_foo", "warn") && !match(C, "foo", "warn"));
        CHECK(match(C, "na\xC3\xAFve", "\xC3\xAF") && match(E, "\xE2\x82\xAC", "\xE2\x82\xAC") &&
              !match(E, "\xE2\x82\xAC", "\xE2\x82\xAD") && !match(C, "\xE2\x82", "\xE2\x82\xAC"));
        CHECK(match(R, "23", "\\d+", true) && !match(R, "some233", "\\d+", false));
        CHECK(match(P, "zzz", "abc") && match(7, "zzz", "abc") && match(-1, "", "abc"));  // default: the value is kept
        for (int s : {E, P, R, C, 7}) CHECK(match(s, "anything", "") && match(s, "", ""));  // an empty pattern is not consulted
    }
    {  // GatewayRuleManagerTest.testLoadAndGetGatewayRules, GatewayRuleConverterTest.testConvertAndApplyToParamRule
        blob.clear();
        sg_gateway_rule r1 = rule(0, 500);
        sg_gateway_rule r2 = with_item(rule(0, 20), SG_GW_PARSE_CLIENT_IP, true);
        r2.interval_sec = 2, r2.burst = 5, r2.capacity_log2 = 11;
        sg_gateway_rule r3 = with_item(rule(1, 10), SG_GW_PARSE_HEADER, false);
        r3.control_behavior = 2, r3.max_queueing_timeout_ms = 600;
        const sg_gateway_rule rules[] = {r1, r2, r3};
        CHECK(gw_ranges_ok(rules, 3, 0, 2) && !gw_ranges_ok(rules, 3, 0, 1));
        const GwConverted c = gw_convert(rules, 3, 2, 1);
        CHECK(c.rules.size() == 3 && c.hot.empty());
        CHECK(c.source[0] == 1 && c.source[1] == 0 && c.source[2] == 2);
        CHECK(c.rules[0].param_idx == 0 && c.rules[1].param_idx == 1 && c.rules[2].param_idx == 0);
        const sg_pslot_rule& p = c.rules[0];
        CHECK(p.resource == 0 && p.rule.count == 20 && p.rule.duration_sec == 2 && p.rule.burst == 5 && p.grade == 1 &&
              p.rule.behavior == 0 && p.rule.max_queueing_ms == 500 && p.rule.capacity_log2 == 11 && p.cluster_mode == 0 &&
              p.rule.hot_count == 0);
        CHECK(c.rules[2].rule.behavior == 2 && c.rules[2].rule.max_queueing_ms == 600);
        CHECK(c.res[0].n_items == 1 && c.res[0].has_item_less == 1 && c.res[1].n_items == 1 && c.res[1].has_item_less == 0);
    }
    {  // GatewayParamParserTest.testParseParametersNoParamItem
        blob.clear();
        sg_gateway_rule a = rule(0, 5), b = rule(0, 10);
        b.control_behavior = 2, b.max_queueing_timeout_ms = 1000;
        const sg_gateway_rule rules[] = {a, b};
        const GwConverted c = gw_convert(rules, 2, 1, 1);
        CHECK(parse(c, 0, 0, {}).size() == 1 && parse(c, 0, 0, {})[0] == "$D");
        CHECK(c.rules.size() == 2 && c.rules[0].param_idx == 0 && c.rules[1].param_idx == 0);
    }
    {  // ...WithItems
        blob.clear();
        sg_gateway_rule np = rule(0, 10);
        np.interval_sec = 10;
        const sg_gateway_rule rules[] = {with_item(rule(0, 2), SG_GW_PARSE_CLIENT_IP, true),
                                         with_item(rule(0, 10), SG_GW_PARSE_HEADER, false),
                                         with_item(rule(0, 20), SG_GW_PARSE_URL_PARAM, false),
                                         with_item(rule(0, 120), SG_GW_PARSE_HOST, true),
                                         with_item(rule(0, 50), SG_GW_PARSE_COOKIE, false),
                                         np,
                                         with_item(rule(1, 5), SG_GW_PARSE_URL_PARAM, false)};
        sg_gateway_rule all[7];
        std::memcpy(all, rules, sizeof rules);
        all[6].resource_mode = 1;
        const GwConverted c = gw_convert(all, 7, 2, 1);
        const auto params = parse(c, 0, 0, {{"66.77.88.99", false}, {"Sentinel", false}, {"17", false},
                                            {"hello.test.sentinel", false}, {"Sentinel-Foo", false}});
        CHECK(params.size() == 6 && params[0] == "66.77.88.99" && params[1] == "Sentinel" && params[2] == "17" &&
              params[3] == "hello.test.sentinel" && params[4] == "Sentinel-Foo" && params[5] == "$D");
        CHECK(parse(c, 1, 0, {{"17", false}}).empty());  // a route-id predicate over a custom-API rule
        const auto api = parse(c, 1, 1, {{"fs", false}});
        CHECK(api.size() == 1 && api[0] == "fs");
        CHECK(parse(c, 5, 0, {}).empty());               // a resource the tables do not have
    }
    {  // ...WithEmptyItemPattern, ...WithItemPatternMatching
        blob.clear();
        sg_gateway_rule api = with_item(rule(2, 5), SG_GW_PARSE_URL_PARAM, false, "\\d+", SG_GW_MATCH_REGEX);
        api.resource_mode = 1;
        const sg_gateway_rule rules[] = {with_item(rule(0, 10), SG_GW_PARSE_HEADER, false, "", SG_GW_MATCH_EXACT),
                                         with_item(rule(1, 10), SG_GW_PARSE_HEADER, false, "Wow", SG_GW_MATCH_EXACT),
                                         with_item(rule(1, 20), SG_GW_PARSE_URL_PARAM, false, "warn", SG_GW_MATCH_CONTAINS),
                                         api};
        CHECK(gw_ranges_ok(rules, 4, blob.size(), 3) && !gw_ranges_ok(rules, 4, blob.size() - 1, 3));
        const GwConverted c = gw_convert(rules, 4, 3, 9);
        CHECK(parse(c, 0, 0, {{"Sent1nel", false}}) == std::vector<std::string>{"Sent1nel"});
        CHECK(c.hot.size() == 4 && c.hot[0].value == 9 && c.hot[0].threshold == 10000000);  // a non-null pattern, even ""
        CHECK(c.rules[0].rule.hot_count == 1 && c.rules[2].rule.hot_begin == 2);
        CHECK((parse(c, 1, 0, {{"Wow", false}, {"warn", false}}) == std::vector<std::string>{"Wow", "warn"}));
        CHECK((parse(c, 1, 0, {{"Wow_foo", false}, {"warn_foo", false}}) == std::vector<std::string>{"$NM", "warn_foo"}));
        CHECK((parse(c, 1, 0, {{"foo", false}, {"foo", false}}) == std::vector<std::string>{"$NM", "$NM"}));
        CHECK((parse(c, 1, 0, {{nullptr, false}, {"foo", false}}) == std::vector<std::string>{"<null>", "$NM"}));
        CHECK(parse(c, 2, 1, {{"23", true}}) == std::vector<std::string>{"23"});
        CHECK(parse(c, 2, 1, {{"some233", false}}) == std::vector<std::string>{"$NM"});
    }
    {  // equal item-less rules collapse; invalid rules take no index; mixed modes; a parse strategy above 4
        blob.clear();
        sg_gateway_rule big = rule(3, 5);
        big.capacity_log2 = 9;  // not part of ParamFlowRule.equals
        sg_gateway_rule invalid = with_item(rule(3, 1), SG_GW_PARSE_HEADER, true);
        sg_gateway_rule other_mode = with_item(rule(3, 7), 9, false, "q", SG_GW_MATCH_PREFIX);
        other_mode.resource_mode = 1;
        const sg_gateway_rule rules[] = {rule(3, 5), rule(3, 5), invalid, rule(3, 6), with_item(rule(3, 5), 0, true),
                                         big, other_mode, rule(3, -0.0)};
        const GwConverted c = gw_convert(rules, 8, 4, 1);
        CHECK(c.rules.size() == 5);
        const uint32_t want_src[] = {4, 6, 0, 3, 7};
        const int32_t want_idx[] = {0, 1, 2, 2, 2};
        for (int k = 0; k < 5; ++k) CHECK(c.source[k] == want_src[k] && c.rules[k].param_idx == want_idx[k]);
        CHECK(c.res[3].n_items == 2 && c.res[3].has_item_less == 1 && c.res[0].n_items == 0 && c.res[0].has_item_less == 0);
        CHECK(parse(c, 3, 0, {{"a", false}, {"b", false}}).empty() && parse(c, 3, 1, {{"a", false}, {"b", false}}).empty());
        CHECK(gw_same_converted(rule(0, 0.0), rule(1, 0.0)) && !gw_same_converted(rule(0, 0.0), rule(0, -0.0)));
    }
    {  // a parse strategy above 4 answers null, whatever the item holds
        blob.clear();
        const sg_gateway_rule rules[] = {with_item(rule(0, 7), 9, false, "q", SG_GW_MATCH_EXACT)};
        const GwConverted c = gw_convert(rules, 1, 1, 1);
        CHECK(parse(c, 0, 0, {{"q", false}}) == std::vector<std::string>{"<null>"});
    }
    std::printf("gateway host ok\n");
    return 0;
}
