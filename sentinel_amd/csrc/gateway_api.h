// gateway_api.h — the gateway's API definitions, host side and the functions host and device share: which definitions
// are kept (GatewayApiDefinitionManager.isValidApi), which of two with one name is the definition
// (GatewayApiMatcherManager.loadApiDefinitions keys by name), which predicates a matcher has
// (WebExchangeApiMatcher.fromApiPathPredicate), how each is decided (RouteMatchers.exactPath / antPath / regexPath), the
// Ant matcher itself (Spring 5.3.18 AntPathMatcher.doMatch, restated in include/sentinel_gpu.h), and the lookup tables
// sg_gateway_expand_batch walks. No HIP in here beyond the host/device marker: gateway_api.hip calls the matcher and the
// hash per request, the C ABI builds the tables, and tests/cpp/test_gateway_api_host.cpp runs all of it on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "gateway_rules.h"

namespace sg {

constexpr uint32_t kGwaNone = 0xFFFFFFFFu;

enum GwaClass : uint8_t {
    kGwaSkip = 0,   // not a path predicate, or a null / blank pattern: the matcher does not have it
    kGwaExact = 1,  // String.equals
    kGwaAnt = 2,    // the device's Ant matcher
    kGwaNever = 3,  // PREFIX without a wildcard, REGEX that did not compile
    kGwaHost = 4,   // the caller's verdict
};

struct GwaPred {  // an Ant predicate in a candidate list
    uint32_t api;  // ordinal of its definition among the kept ones (ascending caller index)
    uint32_t pat_off;
    uint32_t pat_len;
    uint32_t pred;  // index in the caller's preds[]
};

struct GwaSlot {  // open addressing, linear probing; count == 0: empty
    uint32_t hash;
    uint32_t key_off;  // the key's bytes in the pattern blob
    uint32_t key_len;
    uint32_t begin;    // its candidates: exact_list / ant [begin, begin + count), ascending api
    uint32_t count;
};

// ---- shared with the device

SG_GW_HD inline uint32_t gwa_hash(const uint8_t* s, uint32_t n) {  // FNV-1a
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
    return h;
}

// Bytes of the UTF-8 sequence at s[i] (i < n): from the lead byte, cut at n; a continuation or invalid byte is one.
SG_GW_HD inline uint32_t gwa_cp_len(const uint8_t* s, uint32_t i, uint32_t n) {
    const uint8_t c = s[i];
    const uint32_t l = c < 0x80 ? 1u : (c >> 5) == 6 ? 2u : (c >> 4) == 14 ? 3u : (c >> 3) == 30 ? 4u : 1u;
    return l < n - i ? l : n - i;
}

// One segment as a whole-segment glob: `?` one code point, `*` any run, the rest literal bytes.
SG_GW_HD inline bool gwa_seg_match(const uint8_t* p, uint32_t pn, const uint8_t* s, uint32_t sn) {
    uint32_t pi = 0, si = 0, star_p = kGwaNone, star_s = 0;
    while (si < sn) {
        if (pi < pn && p[pi] == '*') {
            star_p = ++pi;
            star_s = si;
        } else if (pi < pn && p[pi] == '?') {
            si += gwa_cp_len(s, si, sn);
            ++pi;
        } else if (pi < pn && p[pi] == s[si]) {
            ++pi;
            ++si;
        } else if (star_p != kGwaNone) {  // the last `*` takes one more code point
            star_s += gwa_cp_len(s, star_s, sn);
            si = star_s;
            pi = star_p;
        } else {
            return false;
        }
    }
    while (pi < pn && p[pi] == '*') ++pi;
    return pi == pn;
}

// The first token of s[pos, n): false when there is none.
SG_GW_HD inline bool gwa_next(const uint8_t* s, uint32_t n, uint32_t pos, uint32_t& b, uint32_t& e) {
    while (pos < n && s[pos] == '/') ++pos;
    if (pos >= n) return false;
    b = pos;
    while (pos < n && s[pos] != '/') ++pos;
    e = pos;
    return true;
}

// The last token of s[lo, end): false when there is none.
SG_GW_HD inline bool gwa_prev(const uint8_t* s, uint32_t lo, uint32_t end, uint32_t& b, uint32_t& e) {
    while (end > lo && s[end - 1] == '/') --end;
    if (end <= lo) return false;
    e = end;
    while (end > lo && s[end - 1] != '/') --end;
    b = end;
    return true;
}

SG_GW_HD inline bool gwa_is_dstar(const uint8_t* p, uint32_t b, uint32_t e) {
    return e - b == 2 && p[b] == '*' && p[b + 1] == '*';
}

// AntPathMatcher.doMatch(pattern, path, true) for a pattern with at most one `**` segment (a second one is never asked
// of this function: such predicates are the caller's; it answers false). No token arrays: both strings are walked in
// place from the front up to the `**` and from the back down to it.
SG_GW_HD inline bool gwa_ant_match(const uint8_t* p, uint32_t pn, const uint8_t* s, uint32_t sn) {
    if ((pn > 0 && p[0] == '/') != (sn > 0 && s[0] == '/')) return false;
    const bool pslash = pn > 0 && p[pn - 1] == '/', sslash = sn > 0 && s[sn - 1] == '/';
    uint32_t pp = 0, sp = 0, pb = 0, pe = 0, sb = 0, se = 0;
    bool hp, hs;
    for (;;) {
        hp = gwa_next(p, pn, pp, pb, pe);
        hs = gwa_next(s, sn, sp, sb, se);
        if (!hp || !hs || gwa_is_dstar(p, pb, pe)) break;
        if (!gwa_seg_match(p + pb, pe - pb, s + sb, se - sb)) return false;
        pp = pe;
        sp = se;
    }
    if (!hs) {  // the path is exhausted
        if (!hp) return pslash == sslash;
        uint32_t nb, ne;
        if (!gwa_next(p, pn, pe, nb, ne) && pe - pb == 1 && p[pb] == '*' && sslash) return true;
        for (;;) {
            if (!gwa_is_dstar(p, pb, pe)) return false;
            if (!gwa_next(p, pn, pe, nb, ne)) return true;
            pb = nb;
            pe = ne;
        }
    }
    if (!hp) return false;
    // p[pb, pe) is the `**`, the path's tokens from sp on are open
    const uint32_t plo = pe;
    uint32_t pend = pn, send = sn;
    for (bool last = true;; last = false) {
        uint32_t qb, qe, tb, te;
        if (!gwa_prev(p, plo, pend, qb, qe)) return true;   // only the `**` is left
        if (gwa_is_dstar(p, qb, qe)) return false;          // out of contract
        if (!gwa_prev(s, sp, send, tb, te)) return false;   // the path ran out with a segment left
        if (!gwa_seg_match(p + qb, qe - qb, s + tb, te - tb)) return false;
        if (last && pslash != sslash) return false;
        pend = qb;
        send = tb;
    }
}

SG_GW_HD inline bool gwa_bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// The slot of key s[0, n) with hash h, or nullptr. The tables hold at most half as many keys as slots.
SG_GW_HD inline const GwaSlot* gwa_find(const GwaSlot* slots, uint32_t mask, const uint8_t* blob, uint32_t h,
                                        const uint8_t* s, uint32_t n) {
    for (uint32_t i = h & mask;; i = (i + 1) & mask) {
        const GwaSlot* t = slots + i;
        if (t->count == 0) return nullptr;
        if (t->hash == h && t->key_len == n && gwa_bytes_equal(blob + t->key_off, s, n)) return t;
    }
}

// ---- host only

inline bool gwa_valid_api(const sg_gateway_api& a) {  // isValidApi
    return (a.flags & (SG_GW_API_NAME_BLANK | SG_GW_API_PREDS_NULL)) == 0;
}

inline bool gwa_is_ws(uint8_t c) {  // Character.isWhitespace over ASCII
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31);
}

inline uint32_t gwa_dstar_segments(const uint8_t* p, uint32_t n) {
    uint32_t pos = 0, b, e, k = 0;
    while (gwa_next(p, n, pos, b, e)) {
        k += gwa_is_dstar(p, b, e);
        pos = e;
    }
    return k;
}

inline GwaClass gwa_classify(const sg_gateway_api_pred& pr, const uint8_t* blob) {
    if (pr.flags & (SG_GW_PRED_NOT_PATH | SG_GW_PRED_PATTERN_NULL)) return kGwaSkip;
    const uint8_t* p = blob + pr.pattern_off;
    const uint32_t n = pr.pattern_len;
    if (std::all_of(p, p + n, gwa_is_ws)) return kGwaSkip;  // StringUtil.isBlank, the empty pattern included
    if (pr.match_strategy == SG_GW_URL_MATCH_REGEX) return (pr.flags & SG_GW_PRED_REGEX_INVALID) ? kGwaNever : kGwaHost;
    if (pr.match_strategy != SG_GW_URL_MATCH_PREFIX) return kGwaExact;
    const auto has = [&](char c) { return std::find(p, p + n, (uint8_t)c) != p + n; };
    if (has('{') || has('}')) return kGwaHost;        // URI template variables: Spring's
    if (!has('*') && !has('?')) return kGwaNever;     // AntPathMatcher.isPattern
    return gwa_dstar_segments(p, n) >= 2 ? kGwaHost : kGwaAnt;
}

// A resource >= n_resources, a predicate range outside preds or a pattern range outside the blob: false.
inline bool gwa_ranges_ok(const sg_gateway_api* apis, uint32_t n_apis, const sg_gateway_api_pred* preds, uint32_t n_preds,
                          uint64_t n_pattern_bytes, uint32_t n_resources) {
    for (uint32_t i = 0; i < n_apis; ++i) {
        if (apis[i].resource >= n_resources) return false;
        if (!(apis[i].flags & SG_GW_API_PREDS_NULL) && (uint64_t)apis[i].pred_begin + apis[i].pred_count > n_preds)
            return false;
    }
    for (uint32_t i = 0; i < n_preds; ++i)
        if (!(preds[i].flags & SG_GW_PRED_PATTERN_NULL) &&
            (uint64_t)preds[i].pattern_off + preds[i].pattern_len > n_pattern_bytes)
            return false;
    return true;
}

struct GwaTables {
    std::vector<uint8_t> cls;            // [n_preds] GwaClass
    std::vector<uint32_t> winners;       // kept definitions, ascending caller index: ordinal → apis[] index
    std::vector<uint32_t> api_res;       // ordinal → resource
    std::vector<GwaSlot> exact;          // whole-path table
    std::vector<uint32_t> exact_list;    // api ordinals
    std::vector<GwaSlot> bucket;         // first-segment table of the Ant predicates with a literal first segment
    std::vector<GwaPred> ant;            // their candidates
    std::vector<GwaPred> wild;           // Ant predicates with a wildcard first segment, ascending api
    std::vector<uint32_t> vid_pred;      // verdict id → preds[] index
    std::vector<uint32_t> vid_begin;     // [n vids + 1] → vid_apis: the definitions a true verdict matches
    std::vector<uint32_t> vid_apis;
    uint32_t max_res = 0;                // the largest api_res, for the caller's bounds
};

inline std::vector<GwaSlot> gwa_make_table(size_t keys) {
    size_t cap = 1;
    while (cap < 2 * keys) cap <<= 1;
    return std::vector<GwaSlot>(cap, GwaSlot{0, 0, 0, 0, 0});
}

inline void gwa_insert(std::vector<GwaSlot>& t, GwaSlot s) {
    const uint32_t mask = (uint32_t)t.size() - 1;
    uint32_t i = s.hash & mask;
    while (t[i].count) i = (i + 1) & mask;
    t[i] = s;
}

// The tables over input that passed gwa_ranges_ok.
inline GwaTables gwa_build(const sg_gateway_api* apis, uint32_t n_apis, const sg_gateway_api_pred* preds,
                           uint32_t n_preds, const uint8_t* blob) {
    GwaTables t;
    t.cls.resize(n_preds);
    for (uint32_t i = 0; i < n_preds; ++i) t.cls[i] = gwa_classify(preds[i], blob);
    std::map<uint32_t, uint32_t> by_name;  // resource → the last valid definition
    for (uint32_t i = 0; i < n_apis; ++i)
        if (gwa_valid_api(apis[i])) by_name[apis[i].resource] = i;
    for (const auto& kv : by_name) t.winners.push_back(kv.second);
    std::sort(t.winners.begin(), t.winners.end());
    std::vector<uint32_t> vid_of(n_preds, kGwaNone);
    for (uint32_t i = 0; i < n_preds; ++i)
        if (t.cls[i] == kGwaHost) {
            vid_of[i] = (uint32_t)t.vid_pred.size();
            t.vid_pred.push_back(i);
        }
    using Key = std::pair<uint32_t, uint32_t>;  // (offset, length) in the blob
    const auto key_less = [&](const Key& a, const Key& b) {
        return std::lexicographical_compare(blob + a.first, blob + a.first + a.second, blob + b.first,
                                            blob + b.first + b.second);
    };
    std::map<Key, std::vector<uint32_t>, decltype(key_less)> exact(key_less);
    std::map<Key, std::vector<GwaPred>, decltype(key_less)> bucket(key_less);
    std::vector<std::vector<uint32_t>> vid_apis(t.vid_pred.size());
    for (uint32_t a = 0; a < t.winners.size(); ++a) {
        const sg_gateway_api& d = apis[t.winners[a]];
        t.api_res.push_back(d.resource);
        t.max_res = std::max(t.max_res, d.resource);
        for (uint32_t k = 0; k < d.pred_count; ++k) {
            const uint32_t pi = d.pred_begin + k;
            const sg_gateway_api_pred& pr = preds[pi];
            switch (t.cls[pi]) {
                case kGwaExact: {
                    auto& l = exact[Key{pr.pattern_off, pr.pattern_len}];
                    if (l.empty() || l.back() != a) l.push_back(a);
                    break;
                }
                case kGwaAnt: {
                    const uint8_t* p = blob + pr.pattern_off;
                    uint32_t b = 0, e = 0;
                    gwa_next(p, pr.pattern_len, 0, b, e);  // a pattern with a wildcard has a token
                    const bool literal = std::none_of(p + b, p + e, [](uint8_t c) { return c == '*' || c == '?'; });
                    const GwaPred c{a, pr.pattern_off, pr.pattern_len, pi};
                    if (literal)
                        bucket[Key{pr.pattern_off + b, e - b}].push_back(c);
                    else
                        t.wild.push_back(c);
                    break;
                }
                case kGwaHost: {
                    auto& l = vid_apis[vid_of[pi]];
                    if (l.empty() || l.back() != a) l.push_back(a);
                    break;
                }
                default: break;
            }
        }
    }
    t.exact = gwa_make_table(exact.size());
    for (const auto& kv : exact) {
        gwa_insert(t.exact, GwaSlot{gwa_hash(blob + kv.first.first, kv.first.second), kv.first.first, kv.first.second,
                                    (uint32_t)t.exact_list.size(), (uint32_t)kv.second.size()});
        t.exact_list.insert(t.exact_list.end(), kv.second.begin(), kv.second.end());
    }
    t.bucket = gwa_make_table(bucket.size());
    for (const auto& kv : bucket) {
        gwa_insert(t.bucket, GwaSlot{gwa_hash(blob + kv.first.first, kv.first.second), kv.first.first, kv.first.second,
                                     (uint32_t)t.ant.size(), (uint32_t)kv.second.size()});
        t.ant.insert(t.ant.end(), kv.second.begin(), kv.second.end());
    }
    t.vid_begin.push_back(0);
    for (const auto& l : vid_apis) {
        t.vid_apis.insert(t.vid_apis.end(), l.begin(), l.end());
        t.vid_begin.push_back((uint32_t)t.vid_apis.size());
    }
    return t;
}

// Does the definition with ordinal `a` match `path`? The tables' answer on the CPU (verdicts: the true verdict ids,
// ascending): what the device computes per request, list by list.
inline void gwa_match_host(const GwaTables& t, const uint8_t* blob, const uint8_t* path, uint32_t n,
                           const std::vector<uint32_t>& verdicts, std::vector<uint32_t>& out) {
    out.clear();
    if (const GwaSlot* s = gwa_find(t.exact.data(), (uint32_t)t.exact.size() - 1, blob, gwa_hash(path, n), path, n))
        out.insert(out.end(), t.exact_list.begin() + s->begin, t.exact_list.begin() + s->begin + s->count);
    uint32_t b = 0, e = 0;
    if (gwa_next(path, n, 0, b, e))
        if (const GwaSlot* s = gwa_find(t.bucket.data(), (uint32_t)t.bucket.size() - 1, blob, gwa_hash(path + b, e - b),
                                        path + b, e - b))
            for (uint32_t k = s->begin; k < s->begin + s->count; ++k)
                if (gwa_ant_match(blob + t.ant[k].pat_off, t.ant[k].pat_len, path, n)) out.push_back(t.ant[k].api);
    for (const GwaPred& w : t.wild)
        if (gwa_ant_match(blob + w.pat_off, w.pat_len, path, n)) out.push_back(w.api);
    for (uint32_t v : verdicts)
        if (v + 1 < t.vid_begin.size())
            out.insert(out.end(), t.vid_apis.begin() + t.vid_begin[v], t.vid_apis.begin() + t.vid_begin[v + 1]);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
}

// Verdict ids of the gateway rules: per item rule of the converted tables (GwConverted::items order) the id, or
// kGwaNone. Kept item rules with SG_GW_MATCH_REGEX, in the caller's rule order, numbered from `first`.
// item_source[j] = the gateway rule behind item rule j.
inline std::vector<uint32_t> gwa_item_sources(const GwConverted& c) {
    std::vector<uint32_t> src(c.items.size(), 0);
    for (size_t i = 0; i < c.rules.size(); ++i) {
        const GwRes& gr = c.res[c.rules[i].resource];
        if ((uint32_t)c.rules[i].param_idx < gr.n_items) src[gr.rule_begin + c.rules[i].param_idx] = c.source[i];
    }
    return src;
}

inline std::vector<uint32_t> gwa_item_vids(const GwConverted& c, const std::vector<uint32_t>& item_source, uint32_t first,
                                           std::vector<uint32_t>& vid_rule) {
    std::vector<uint32_t> order;
    for (uint32_t j = 0; j < c.items.size(); ++j)
        if (c.items[j].match_strategy == SG_GW_MATCH_REGEX) order.push_back(j);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return item_source[a] < item_source[b]; });
    std::vector<uint32_t> vid(c.items.size(), kGwaNone);
    vid_rule.clear();
    for (uint32_t j : order) {
        vid[j] = first + (uint32_t)vid_rule.size();
        vid_rule.push_back(item_source[j]);
    }
    return vid;
}

}  // namespace sg
