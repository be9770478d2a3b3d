// authority_rules.h — AuthoritySlot's rule table and its host-side compiler. No HIP in here: the device reads
// LAuth (engine.h includes this file), the C ABI compiles sg_authority_rule arrays into it, and
// tests/cpp/test_authority_host.cpp runs the compiler on the CPU.
//
// AuthorityRuleManager.loadAuthorityConf (AuthorityRuleManager.java:108-139): rules in list order, an invalid rule
// (isValidRule :147-150: blank resource, strategy < 0, blank limitApp) is ignored, and the first valid rule of a
// resource wins — later ones are "redundant". AuthorityRuleChecker.passCheck (AuthorityRuleChecker.java:30-65): the
// origin is looked up among limitApp's comma-separated items; AUTHORITY_BLACK with a hit blocks, AUTHORITY_WHITE
// without one blocks, any other strategy >= 0 never blocks but still holds the resource's one rule slot.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/sentinel_gpu.h"

namespace sg {

constexpr uint32_t kAuthNone = 0;   // no rule: every origin passes
constexpr uint32_t kAuthWhite = 1;  // blocks an origin that is not listed
constexpr uint32_t kAuthBlack = 2;  // blocks a listed origin
constexpr uint32_t kAuthNever = 3;  // a rule of another strategy: never blocks
constexpr uint32_t kAuthMaskIds = 64;          // origin ids 1..64 live in the mask
constexpr uint32_t kAuthCount = 0x3FFFFFFFu;   // LAuth::cs: the tail's length below the state's two bits

// One resource's rule: origin ids 1..64 as bits 0..63 of mask (one load and a bit test decide the common case), the
// larger ids sorted and unique in ids[begin .. begin + count).
struct alignas(16) LAuth {
    uint64_t mask;
    uint32_t begin;
    uint32_t cs;  // state << 30 | count
};
static_assert(sizeof(LAuth) == 16, "one 16-byte word per resource");

// Compiles rules[0..n) for K resources: tab[K], the sorted tails in ids. Returns the number of rules kept (>= 0), or
// SG_E_INVAL for a resource index >= K, an origin id <= 0 or an id range outside origins[0..n_origin_ids); tab and
// ids are written only on success.
inline int authority_compile(const sg_authority_rule* rules, uint32_t n, const int32_t* origins, uint32_t n_origin_ids,
                             uint32_t K, std::vector<LAuth>& tab, std::vector<int32_t>& ids) {
    std::vector<LAuth> t(K, LAuth{0, 0, kAuthNone << 30});
    std::vector<int32_t> tail;
    int kept = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sg_authority_rule& r = rules[i];
        if (r.resource >= K) return SG_E_INVAL;
        if ((uint64_t)r.origin_begin + r.origin_count > n_origin_ids) return SG_E_INVAL;
        for (uint32_t j = 0; j < r.origin_count; ++j)
            if (origins[r.origin_begin + j] <= 0) return SG_E_INVAL;
        if (r.strategy < 0 || r.origin_count == 0) continue;  // isValidRule
        LAuth& a = t[r.resource];
        if ((a.cs >> 30) != kAuthNone) continue;  // redundant: the resource has its rule
        ++kept;
        const uint32_t state = r.strategy == SG_AUTHORITY_WHITE   ? kAuthWhite
                               : r.strategy == SG_AUTHORITY_BLACK ? kAuthBlack
                                                                  : kAuthNever;
        a.begin = (uint32_t)tail.size();
        if (state != kAuthNever) {
            for (uint32_t j = 0; j < r.origin_count; ++j) {
                const int32_t o = origins[r.origin_begin + j];
                if ((uint32_t)o <= kAuthMaskIds) a.mask |= 1ull << (o - 1);
                else tail.push_back(o);
            }
            std::sort(tail.begin() + a.begin, tail.end());
            tail.erase(std::unique(tail.begin() + a.begin, tail.end()), tail.end());
        }
        a.cs = (state << 30) | ((uint32_t)tail.size() - a.begin);
    }
    if (tail.size() > kAuthCount) return SG_E_INVAL;
    tab.swap(t);
    ids.swap(tail);
    return kept;
}

// AuthorityRuleChecker.passCheck on the compiled table (host restatement of the device's check, for tests).
inline bool authority_rejects(const LAuth& a, const int32_t* ids, int32_t origin) {
    const uint32_t state = a.cs >> 30;
    if (origin <= 0 || state == kAuthNone || state == kAuthNever) return false;
    bool contain;
    if ((uint32_t)origin <= kAuthMaskIds) {
        contain = (a.mask >> (origin - 1)) & 1ull;
    } else {
        const int32_t* b = ids + a.begin;
        contain = std::binary_search(b, b + (a.cs & kAuthCount), origin);
    }
    return state == kAuthBlack ? contain : !contain;
}

}  // namespace sg
