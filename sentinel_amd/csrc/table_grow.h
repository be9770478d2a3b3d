// table_grow.h — host-only size arithmetic and refusal order of the in-place table growth (sg_param_resize,
// sg_cparam_resize, sg_vdict_grow). No HIP in here: the C ABI asks these functions whether a growth may go ahead and
// where every sub-table lands, before it allocates anything, and tests/cpp/test_table_grow_host.cpp runs them on the
// CPU.
//
// One order of refusals for every call: what is wrong with the arguments (SG_E_INVAL: nothing loaded, a wrong rule
// count, a size out of range, a shrink) comes before what the grown tables could not carry (SG_E_UNSUPPORTED: 2^32
// slots or more, or a batch record layout that no longer fits). A growth that passes here never leaves a handle whose
// next batch is refused for width.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/sentinel_gpu.h"

namespace sg {

inline int grow_bits_for(uint64_t v) {  // bits needed to represent v
    int b = 0;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

struct GrowPlan {
    int code = SG_OK;             // SG_OK, SG_E_INVAL or SG_E_UNSUPPORTED
    const char* why = "";         // the refusal's message
    std::vector<uint64_t> base;   // per rule: first slot of its sub-table in the grown table
    std::vector<uint64_t> mask;   // per rule: 2^capacity_log2 - 1
    uint64_t total = 0;           // slots over all sub-tables, side slots included
};

inline GrowPlan grow_refuse(int code, const char* why) {
    GrowPlan p;
    p.code = code;
    p.why = why;
    return p;
}

// The hot-parameter tables. cur_mask[i]: rule i's table_mask in force; want[0..n): 0 keeps the size, else the new
// capacity_log2. max_batch: the handle's; pslot: sg_pslot_load_rules is in force (the slot chain reads these tables).
//   - sg_param_decide_batch's records {slot | acquire code : 8 | request index}: gshift + gbits <= 64;
//   - the slot chain's per-entry lookup keeps a slot in 32 bits beside four codes at the top (LArgs::pslot, CxSide::psl,
//     also what a node shard's compacted slice carries): slots below 0xFFFFFFFC.
// sg_pslot_decide_batch's records carry resources, not slots, so the tables' size does not reach them.
inline GrowPlan grow_plan_param(const std::vector<uint64_t>& cur_mask, const int32_t* want, uint32_t n, uint64_t max_batch,
                                bool pslot) {
    if (cur_mask.empty()) return grow_refuse(SG_E_INVAL, "no param rules loaded");
    if (n != cur_mask.size() || !want) return grow_refuse(SG_E_INVAL, "one capacity_log2 per loaded param rule");
    GrowPlan p;
    p.base.resize(n);
    p.mask.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t m = cur_mask[i];
        if (want[i] != 0) {
            if (want[i] < 1 || want[i] > 30) return grow_refuse(SG_E_INVAL, "capacity_log2 must be 0 or in [1, 30]");
            m = (1ull << want[i]) - 1;
            if (m < cur_mask[i]) return grow_refuse(SG_E_INVAL, "a param rule's table cannot shrink");
        }
        p.base[i] = p.total;
        p.mask[i] = m;
        p.total += m + 2;  // + the side slot for the value ~0
    }
    if (p.total >= (1ull << 32)) return grow_refuse(SG_E_UNSUPPORTED, "param tables larger than 2^32 slots");
    const int ibits = grow_bits_for(max_batch > 1 ? max_batch - 1 : 1);
    if (ibits + 8 + grow_bits_for(p.total + 1) > 64)
        return grow_refuse(SG_E_UNSUPPORTED, "param tables x max_batch too large for 64-bit records");
    if (pslot && p.total > 0xFFFFFFFCull)
        return grow_refuse(SG_E_UNSUPPORTED, "param tables too large for the slot chain's 32-bit lookups");
    return p;
}

// The cluster param tables: one size for all n_rules rules. cparam value records are {slot : gbits | multi : 1 |
// acquire code : 7 | id : idbits} with ids up to max_batch requests.
inline GrowPlan grow_plan_cparam(uint32_t n_rules, uint64_t cur_mask, int32_t want, uint64_t max_batch) {
    if (n_rules == 0) return grow_refuse(SG_E_INVAL, "no cluster param rules loaded");
    if (want < 1 || want > 28) return grow_refuse(SG_E_INVAL, "capacity_log2 must be in [1, 28]");
    const uint64_t m = (1ull << want) - 1;
    if (m < cur_mask) return grow_refuse(SG_E_INVAL, "the cluster param tables cannot shrink");
    GrowPlan p;
    p.base.resize(n_rules);
    p.mask.assign(n_rules, m);
    for (uint32_t i = 0; i < n_rules; ++i) {
        p.base[i] = p.total;
        p.total += m + 2;
    }
    if (p.total >= (1ull << 32)) return grow_refuse(SG_E_UNSUPPORTED, "param tables larger than 2^32 slots");
    const int gbits = grow_bits_for(p.total + 1);
    if (gbits > 32 || 64 - gbits - 8 < grow_bits_for(max_batch ? max_batch : 1))
        return grow_refuse(SG_E_UNSUPPORTED, "param tables x max_batch too large for 64-bit records");
    return p;
}

// The value dictionary: both sizes at least what they are.
inline GrowPlan grow_plan_vdict(bool on, uint64_t cur_capacity, uint64_t cur_arena, int32_t want_log2, uint64_t want_arena) {
    if (!on) return grow_refuse(SG_E_INVAL, "sg_vdict_init first");
    if (want_log2 < 1 || want_log2 > 28) return grow_refuse(SG_E_INVAL, "capacity_log2 must be in [1, 28]");
    if ((1ull << want_log2) < cur_capacity) return grow_refuse(SG_E_INVAL, "the value dictionary cannot shrink");
    if (want_arena < cur_arena) return grow_refuse(SG_E_INVAL, "the value dictionary's arena cannot shrink");
    GrowPlan p;
    p.total = 1ull << want_log2;
    return p;
}

}  // namespace sg
