// TEST INFRASTRUCTURE: the gateway API definitions' host side and the matcher host and device share
// (sentinel_amd/csrc/gateway_api.h) on the CPU, built with the address and undefined-behaviour sanitizers by
// tests/cpp/gateway_api_host.mk: the Ant matcher's known answers, predicate classification, validity, the winner of
// duplicate names, the lookup tables and the verdict ids. `test_gateway_api_host match <file>` classifies and matches a
// file of definitions and paths for tests/test_gateway_api_host.py:
//   P <strategy> <flags> <pattern hex or ->      a predicate, in preds[] order
//   A <resource> <pred_begin> <pred_count> <flags>
//   Q <path hex or -> <true verdict ids, comma separated, or ->
// and prints "C <classes>", "V <verdict id → predicate>", then per Q line "M <matching resources in entry order>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../../sentinel_amd/csrc/gateway_api.h"

using namespace sg;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

static bool ant(const std::string& pattern, const std::string& path) {
    // exact-size heap copies: a read past either end is the sanitizer's
    std::vector<uint8_t> p(pattern.begin(), pattern.end()), s(path.begin(), path.end());
    return gwa_ant_match(p.data(), (uint32_t)p.size(), s.data(), (uint32_t)s.size());
}

static std::string blob;

static sg_gateway_api_pred pred(const char* pattern, int32_t strategy = SG_GW_URL_MATCH_EXACT, uint32_t flags = 0) {
    sg_gateway_api_pred p{strategy, flags, (uint32_t)blob.size(), 0};
    if (pattern) {
        p.pattern_len = (uint32_t)std::strlen(pattern);
        blob += pattern;
    } else {
        p.flags |= SG_GW_PRED_PATTERN_NULL;
    }
    return p;
}

static GwaClass cls(const char* pattern, int32_t strategy, uint32_t flags = 0) {
    blob.clear();
    const sg_gateway_api_pred p = pred(pattern, strategy, flags);
    return gwa_classify(p, u8(blob));
}

static std::vector<uint32_t> matches(const GwaTables& t, const std::string& path, std::vector<uint32_t> verdicts = {}) {
    std::vector<uint32_t> out;
    std::vector<uint8_t> s(path.begin(), path.end());
    gwa_match_host(t, u8(blob), s.data(), (uint32_t)s.size(), verdicts, out);
    for (uint32_t& a : out) a = t.api_res[a];
    return out;
}

static void known_answers() {
    struct { const char *pattern, *path; bool want; } kat[] = {
        {"/product/**", "/product", true},   {"/product/**", "/product/", true}, {"/product/**", "/product/a/b", true},
        {"/product/**", "/products", false}, {"/a/*", "/a/b", true},             {"/a/*", "/a/", true},
        {"/a/*", "/a", false},               {"/a/*", "/a/b/c", false},          {"/a/?", "/a/b", true},
        {"/a/?", "/a/\xc3\xa9", true},       {"/a/?", "/a/bc", false},           {"/a/*.html", "/a/x.html", true},
        {"/a/*.html", "/a/b/x.html", false}, {"/**/x.jsp", "/x.jsp", true},      {"/**/x.jsp", "/a/b/x.jsp", true},
        {"/a/**/b", "/a/b", true},           {"/a/**/b", "/a/x/y/b", true},      {"/a/**/b", "/a/b/c", false},
        {"/a/b", "/a/b/", false},            {"/a/b/", "/a/b", false},           {"a/*", "/a/b", false},
        {"/a/b*", "/a//bc", true},           {"/A/*", "/a/b", false},
        // the edges the walk-in-place matcher has: empty strings, `**` alone and last, `a**b`, `?` over 3 and 4 bytes
        {"/**", "/", true},                  {"/**", "", false},                 {"**", "", true},
        {"/*", "/", true},                   {"/a/**/", "/a/b", true},           {"/a/**/b/", "/a/b", false},
        {"/a/**/b/", "/a/x/b/", true},       {"/a**b", "/axyb", true},           {"/a**b", "/ab", true},
        {"/a**b", "/a/b", false},            {"/??", "/\xe2\x82\xac", false},    {"/?", "/\xe2\x82\xac", true},
        {"/*??", "/\xe2\x82\xac", false},    {"/*?", "/\xf0\x9f\x98\x80", true}, {"/a/**/b/c", "/a/c", false},
        {"/a/**/b/c", "/a/b/c", true},       {"/a/**/b/c", "/a/b/b/c", true},    {"/*a*b", "/xaxbxab", true},
        {"/*a*b", "/xaxbxa", false},         {"/a/*", "/a//", true},             {"/?/**", "/ab/c", false},
    };
    for (const auto& k : kat) {
        if (ant(k.pattern, k.path) != k.want) {
            std::printf("FAILED: %s on %s, want %d\n", k.pattern, k.path, (int)k.want);
            std::exit(1);
        }
    }
    // PREFIX without a wildcard never matches, not even its own text
    CHECK(cls("/abc", SG_GW_URL_MATCH_PREFIX) == kGwaNever);
    CHECK(cls("/abc", SG_GW_URL_MATCH_EXACT) == kGwaExact && cls("/abc", 7) == kGwaExact && cls("/abc", -1) == kGwaExact);
    CHECK(cls("/a/**", SG_GW_URL_MATCH_PREFIX) == kGwaAnt && cls("/a?", SG_GW_URL_MATCH_PREFIX) == kGwaAnt);
    CHECK(cls("/a/.*", SG_GW_URL_MATCH_REGEX) == kGwaHost);
    CHECK(cls("/a/(", SG_GW_URL_MATCH_REGEX, SG_GW_PRED_REGEX_INVALID) == kGwaNever);
    CHECK(cls("/a/{id}", SG_GW_URL_MATCH_PREFIX) == kGwaHost && cls("/a/{id}/*", SG_GW_URL_MATCH_PREFIX) == kGwaHost);
    CHECK(cls("/a}", SG_GW_URL_MATCH_PREFIX) == kGwaHost);
    CHECK(cls("/**/a/**", SG_GW_URL_MATCH_PREFIX) == kGwaHost && cls("/**/a**", SG_GW_URL_MATCH_PREFIX) == kGwaAnt);
    CHECK(cls(nullptr, 0) == kGwaSkip && cls("", 0) == kGwaSkip && cls(" \t\x1f", 1) == kGwaSkip);
    CHECK(cls("/a", 0, SG_GW_PRED_NOT_PATH) == kGwaSkip && cls("\xc2\xa0", 0) == kGwaExact);
}

static void junit() {
    // GatewayApiDefinitionManagerTest.testIsValidApi
    CHECK(!gwa_valid_api(sg_gateway_api{0, 0, 0, SG_GW_API_NAME_BLANK | SG_GW_API_PREDS_NULL}));
    CHECK(!gwa_valid_api(sg_gateway_api{0, 0, 0, SG_GW_API_PREDS_NULL}));
    CHECK(gwa_valid_api(sg_gateway_api{0, 0, 1, 0}));
    // SentinelGatewayFilterTest.testPickMatchingApiDefinitions: resources 0 and 1
    blob.clear();
    const sg_gateway_api_pred preds[] = {pred("/product/**", SG_GW_URL_MATCH_PREFIX), pred("/something"),
                                         pred("/other/**", SG_GW_URL_MATCH_PREFIX)};
    const sg_gateway_api apis[] = {{0, 0, 1, 0}, {1, 1, 2, 0}};
    CHECK(gwa_ranges_ok(apis, 2, preds, 3, blob.size(), 2));
    const GwaTables t = gwa_build(apis, 2, preds, 3, u8(blob));
    CHECK(matches(t, "/product/123") == std::vector<uint32_t>{0});
    CHECK(matches(t, "/products").empty());
    CHECK(matches(t, "/something") == std::vector<uint32_t>{1});
    CHECK(matches(t, "/other/foo/3") == std::vector<uint32_t>{1});
    CHECK(t.wild.empty() && t.ant.size() == 2 && t.exact_list.size() == 1 && t.vid_pred.empty());
}

static void tables() {
    blob.clear();
    // definitions 0 and 3 share resource 2: the last is the definition; 1 is dropped; 4 has no predicates
    const sg_gateway_api_pred preds[] = {
        pred("/old"),                                  // 0: of the losing definition
        pred("/x", 0),                                 // 1: of a dropped definition
        pred("/a/b"), pred("/a/b"),                    // 2, 3: one definition twice: listed once
        pred("/a/.*", SG_GW_URL_MATCH_REGEX),          // 4: verdict id 0
        pred("/*/b", SG_GW_URL_MATCH_PREFIX),          // 5: wild first
        pred("/a/{id}", SG_GW_URL_MATCH_PREFIX),       // 6: verdict id 1, of three definitions
        pred("/a/b"),                                  // 7
        pred("/abc", SG_GW_URL_MATCH_PREFIX),          // 8: never
        pred("a/**", SG_GW_URL_MATCH_PREFIX),          // 9: bucket "a", no leading slash
    };
    const sg_gateway_api apis[] = {{2, 0, 1, 0}, {5, 1, 1, SG_GW_API_NAME_BLANK}, {7, 5, 2, 0}, {2, 2, 5, 0},
                                   {9, 0, 0, 0}, {4, 6, 4, 0}};
    CHECK(gwa_ranges_ok(apis, 6, preds, 10, blob.size(), 10));
    CHECK(!gwa_ranges_ok(apis, 6, preds, 10, blob.size(), 9));       // resource 9
    CHECK(!gwa_ranges_ok(apis, 6, preds, 9, blob.size(), 10));       // predicates 6 .. 9
    CHECK(!gwa_ranges_ok(apis, 6, preds, 10, blob.size() - 1, 10));  // the last pattern
    const GwaTables t = gwa_build(apis, 6, preds, 10, u8(blob));
    CHECK((t.winners == std::vector<uint32_t>{2, 3, 4, 5}) && (t.api_res == std::vector<uint32_t>{7, 2, 9, 4}));
    CHECK((t.vid_pred == std::vector<uint32_t>{4, 6}));
    CHECK(matches(t, "/old").empty() && matches(t, "/x").empty());
    CHECK((matches(t, "/a/b") == std::vector<uint32_t>{7, 2, 4}));            // wild, exact twice → once, exact
    CHECK((matches(t, "/a/b", {0}) == std::vector<uint32_t>{7, 2, 4}));
    CHECK((matches(t, "/q", {0}) == std::vector<uint32_t>{2}));
    CHECK((matches(t, "/q", {1}) == std::vector<uint32_t>{7, 2, 4}));         // one verdict, three definitions
    CHECK((matches(t, "/q", {0, 1}) == std::vector<uint32_t>{7, 2, 4}));
    CHECK(matches(t, "/abc").empty());
    CHECK((matches(t, "a/z") == std::vector<uint32_t>{4}) && matches(t, "/a/z").empty());
    CHECK(matches(t, "").empty() && matches(t, "/").empty());
    // the gateway rules' verdict ids: kept REGEX item rules in caller order, behind the API predicates'
    sg_gateway_rule r{};
    r.grade = 1;
    r.interval_sec = 1;
    r.count = 1;
    r.has_item = 1;
    r.pattern_null = 1;
    sg_gateway_rule rules[5] = {r, r, r, r, r};
    rules[0].resource = 3;
    rules[0].match_strategy = SG_GW_MATCH_REGEX;
    rules[1].resource = 1;
    rules[2].resource = 1;
    rules[2].match_strategy = SG_GW_MATCH_REGEX;
    rules[3].resource = 1;
    rules[3].match_strategy = SG_GW_MATCH_REGEX;
    rules[3].count = -1;  // dropped: no id
    rules[4].resource = 0;
    rules[4].match_strategy = SG_GW_MATCH_REGEX;
    const GwConverted c = gw_convert(rules, 5, 4, 1);
    const std::vector<uint32_t> src = gwa_item_sources(c);
    CHECK((src == std::vector<uint32_t>{4, 1, 2, 0}));
    std::vector<uint32_t> vid_rule;
    const std::vector<uint32_t> vid = gwa_item_vids(c, src, 2, vid_rule);
    CHECK((vid_rule == std::vector<uint32_t>{0, 2, 4}) && (vid == std::vector<uint32_t>{4, kGwaNone, 3, 2}));
}

static std::string unhex(const std::string& h) {
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out += (char)std::stoi(h.substr(i, 2), nullptr, 16);
    return out;
}

static int match_file(const char* path) {
    std::ifstream in(path);
    CHECK(in.good());
    std::vector<sg_gateway_api_pred> preds;
    std::vector<sg_gateway_api> apis;
    std::vector<std::pair<std::string, std::vector<uint32_t>>> queries;
    blob.clear();
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind;
        ls >> kind;
        if (kind == "P") {
            int32_t strategy;
            uint32_t flags;
            std::string hex;
            ls >> strategy >> flags >> hex;
            const std::string pat = unhex(hex);
            preds.push_back(sg_gateway_api_pred{strategy, flags, (uint32_t)blob.size(), (uint32_t)pat.size()});
            blob += pat;
        } else if (kind == "A") {
            sg_gateway_api a{};
            ls >> a.resource >> a.pred_begin >> a.pred_count >> a.flags;
            apis.push_back(a);
        } else if (kind == "Q") {
            std::string hex, ids;
            ls >> hex >> ids;
            std::vector<uint32_t> v;
            if (ids != "-") {
                std::istringstream is(ids);
                std::string tok;
                while (std::getline(is, tok, ',')) v.push_back((uint32_t)std::stoul(tok));
            }
            queries.emplace_back(unhex(hex), v);
        }
    }
    CHECK(gwa_ranges_ok(apis.data(), (uint32_t)apis.size(), preds.data(), (uint32_t)preds.size(), blob.size(), 1u << 20));
    const GwaTables t = gwa_build(apis.data(), (uint32_t)apis.size(), preds.data(), (uint32_t)preds.size(), u8(blob));
    std::printf("C");
    for (uint8_t c : t.cls) std::printf(" %u", (unsigned)c);
    std::printf("\nV");
    for (uint32_t v : t.vid_pred) std::printf(" %u", v);
    std::printf("\n");
    for (const auto& q : queries) {
        std::printf("M");
        for (uint32_t r : matches(t, q.first, q.second)) std::printf(" %u", r);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "match") == 0) return match_file(argv[2]);
    known_answers();
    junit();
    tables();
    std::printf("gateway api host ok\n");
    return 0;
}
