// grow.hip — the exact value tables grown in place: the hot-parameter sub-tables (PSlot, pslot_dev.h) and the cluster
// param tables (keys + CPBucket rings, cparam_dev.h) rehashed into fresh, larger tables beside the old ones, and the
// occupancy counts a caller watches to grow ahead of a capacity refusal. The reference's maps (CacheMap,
// ClusterParamMetric's value → count buckets) simply grow; here the host allocates the new tables, these kernels
// fill them, and the host swaps them in (api.cpp sg_param_resize / sg_cparam_resize).
//
// Both rehashes keep what the rebuild kernels keep (k_ptable_rebuild, k_cp_rebuild): a value whose slot was claimed
// and never counted is not in the reference's maps and is dropped; the side slots carry over.
//   PSlot    one lane per old slot: find-or-claim the destination by param_slot's CAS, then the whole 32-byte struct.
//   cparam   a claim pass (one lane per old slot → destination index or "dropped" in a u32 map), then a move pass
//            over the old ring in memory order: consecutive lanes take consecutive 16-byte buckets of a slot, read
//            and written as one vector each, so both sides of the bulk copy are coalesced.
//
// The sweep (sg_param_sweep / sg_cparam_sweep) is the same rehash into fresh tables of the same size, with one more
// reason to leave an entry out: it is idle at the caller's now (table_sweep.h), so no later request can tell it from
// absence. Nothing in a probe loop changes: an entry leaves by not being re-inserted, never by a tombstone.
#include "pslot_dev.h"
#include "table_sweep.h"

namespace sg {

namespace {

constexpr uint32_t kGrowDropped = 0xFFFFFFFFu;  // the claim pass's map: this old slot moves nowhere

}  // namespace

// np: the new rules (table_base / table_mask of the grown sub-tables) and the cleared new table; orules / old: the
// tables in force. Rule i of both lists is the same rule.
__global__ void __launch_bounds__(256) k_pgrow(PArgs np, const PRule* orules, const PSlot* old, uint64_t old_total) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < old_total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t ri = rule_of_slot(orules, np.n_rules, g);
        const PRule o = orules[ri];
        const PRule r = np.rules[ri];
        const PSlot s = old[g];
        if (g == o.table_base + o.table_mask + 1) {  // the side slot (its value word stays ~0)
            np.table[r.table_base + r.table_mask + 1] = s;
            continue;
        }
        if (s.value == kEmptyValue || !s.flags) continue;
        const uint64_t ng = param_slot(np, r, s.value);
        if (ng == ~0ull) continue;  // cannot happen: the new sub-table is at least as large
        np.table[ng] = s;           // the value word again, beside its counters: one 32-byte store
    }
}

// out[0] += slots of table[base .. base + n) whose value word is taken, out[1] += those a walker has counted.
__global__ void __launch_bounds__(256) k_ptable_used(const PSlot* table, uint64_t base, uint64_t n,
                                                     unsigned long long* out) {
    uint64_t used = 0, live = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const PSlot s = table[base + i];
        if (s.value == kEmptyValue) continue;
        ++used;
        live += s.flags != 0;
    }
    used = (uint64_t)wave_sum((int64_t)used);
    live = (uint64_t)wave_sum((int64_t)live);
    if (__lane_id() == 0 && used) {
        atomicAdd(out, (unsigned long long)used);
        if (live) atomicAdd(out + 1, (unsigned long long)live);
    }
}

// nc: the new rules and the cleared new keys / rings; orules, oper (slots per old rule), okeys, oring: the tables in
// force. map[g] = the new slot of old slot g, or kGrowDropped.
__global__ void __launch_bounds__(256) k_cpgrow_claim(CPArgs nc, const CPRule* orules, uint64_t oper, const uint64_t* okeys,
                                                      const CPBucket* oring, uint64_t old_total, uint32_t* map) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < old_total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t ri = (uint32_t)(g / oper);
        const CPRule o = orules[ri];
        const CPRule r = nc.rules[ri];
        uint64_t ng = ~0ull;
        if (g == o.table_base + o.table_mask + 1) {
            ng = r.table_base + r.table_mask + 1;
        } else {
            const uint64_t v = okeys[g];
            if (v != kCpEmpty) {
                const CPBucket* src = oring + g * (uint64_t)nc.stride;
                bool live = false;
                for (int j = 0; j < o.S && !live; ++j) live = src[j].start != INT64_MIN;
                if (live) ng = cp_slot(nc, r, v);
            }
        }
        map[g] = ng == ~0ull ? kGrowDropped : (uint32_t)ng;
    }
}

// Bucket i of the old ring → its slot's new ring, 16 bytes per lane. Buckets past the rule's sampleCount are never
// written by any walker and stay as the clear left them.
__global__ void __launch_bounds__(256) k_cpgrow_move(const CPRule* orules, uint64_t oper, const uint4* oring, uint4* nring,
                                                     int stride, const uint32_t* map, uint64_t old_total) {
    const uint64_t cells = old_total * (uint64_t)stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = i / (uint64_t)stride;
        const int j = (int)(i - g * (uint64_t)stride);
        const uint32_t ng = map[g];
        if (ng == kGrowDropped || j >= orules[g / oper].S) continue;
        nring[(uint64_t)ng * (uint64_t)stride + j] = oring[i];
    }
}

// out[0] += slots of keys[base .. base + n) that hold a value, out[1] += those with at least one written bucket.
__global__ void __launch_bounds__(256) k_cptable_used(const uint64_t* keys, const CPBucket* ring, int stride, int S,
                                                      uint64_t base, uint64_t n, unsigned long long* out) {
    uint64_t used = 0, live = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (keys[base + i] == kCpEmpty) continue;
        ++used;
        const CPBucket* src = ring + (base + i) * (uint64_t)stride;
        bool l = false;
        for (int j = 0; j < S && !l; ++j) l = src[j].start != INT64_MIN;
        live += l;
    }
    used = (uint64_t)wave_sum((int64_t)used);
    live = (uint64_t)wave_sum((int64_t)live);
    if (__lane_id() == 0 && used) {
        atomicAdd(out, (unsigned long long)used);
        if (live) atomicAdd(out + 1, (unsigned long long)live);
    }
}

// What a lane of a sweep kernel counted over its slots, summed per wave as in k_ptable_used: cnt[0] += entries given
// back as idle, cnt[1] += claimed-never-counted entries dropped, cnt[2] += thread counts at 0, cnt[3] += entries kept.
// The side slots are outside the counts, as they are outside sg_*_table_used.
struct SweepTally {
    uint64_t n[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void add(SweepVerdict v) { n[v == kSweepIdle ? 0 : v == kSweepClaim ? 1 : 3] += 1; }
    __device__ __forceinline__ void flush(unsigned long long* cnt) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t s = (uint64_t)wave_sum((int64_t)n[k]);
            if (__lane_id() == 0 && s) atomicAdd(cnt + k, (unsigned long long)s);
        }
    }
};

// k_pgrow into a cleared table of the same size under the same rules (np.rules, np.hot), entries idle at `now` left
// out. An idle side slot stays as the clear left it: its empty state.
__global__ void __launch_bounds__(256) k_psweep(PArgs np, const PSlot* old, int64_t now, unsigned long long* cnt) {
    SweepTally tally;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < np.total_slots; g += (uint64_t)gridDim.x * blockDim.x) {
        const PRule r = np.rules[rule_of_slot(np.rules, np.n_rules, g)];
        const PSlot s = old[g];
        const bool side = g == r.table_base + r.table_mask + 1;
        if (!side && s.value == kEmptyValue) continue;
        const SweepVerdict v = sweep_pslot(s.flags, s.time, s.tokens, r.behavior, param_token_count(np, r, s.value),
                                           r.burst, r.duration_sec * 1000, now);
        if (!side) tally.add(v);
        if (v != kSweepKeep) continue;
        const uint64_t ng = side ? g : param_slot(np, r, s.value);
        if (ng == ~0ull) continue;  // cannot happen: the sub-table held these entries
        np.table[ng] = s;           // the value word again, beside its counters: one 32-byte store
    }
    tally.flush(cnt);
}

// k_cpgrow_claim for tables of the same size (nc.rules are the rules in force), a ring with no bucket live at `now`
// mapped nowhere; k_cpgrow_move then moves the mapped rings only.
__global__ void __launch_bounds__(256) k_cpsweep_claim(CPArgs nc, const uint64_t* okeys, const CPBucket* oring, int64_t now,
                                                       uint32_t* map, unsigned long long* cnt) {
    SweepTally tally;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nc.total_slots; g += (uint64_t)gridDim.x * blockDim.x) {
        const CPRule r = nc.rules[(uint32_t)(g / nc.per)];
        const bool side = g == r.table_base + r.table_mask + 1;
        const uint64_t val = okeys[g];
        uint64_t ng = ~0ull;
        if (side || val != kCpEmpty) {
            const SweepVerdict v = sweep_ring(oring + g * (uint64_t)nc.stride, r.S, (int64_t)r.S * (int64_t)r.wl, now);
            if (!side) tally.add(v);
            if (v == kSweepKeep) ng = side ? g : cp_slot(nc, r, val);
        }
        map[g] = ng == ~0ull ? kGrowDropped : (uint32_t)ng;
    }
    tally.flush(cnt);
}

// ParameterMetric's thread counts into a cleared table of the same size: owner, value and count of every entry above
// 0, at the first free slot of ps_tc's probe sequence. Entries are distinct, so a lane claims by the owner word alone
// (ps_tc's own claim also accepts a slot that holds its owner: there only one wave inserts for an owner).
__global__ void __launch_bounds__(256) k_tcsweep(const PSThread* old, PSThread* tc, uint64_t slots, unsigned long long* cnt) {
    const uint64_t mask = slots - 1;
    SweepTally tally;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < slots; g += (uint64_t)gridDim.x * blockDim.x) {
        const PSThread e = old[g];
        if (e.owner == 0) continue;
        if (sweep_thread_idle(e.count)) {
            tally.n[2] += 1;
            continue;
        }
        uint64_t h = ps_hash(e.owner, e.value) & mask;
        for (uint64_t probes = 0; probes <= mask; ++probes, h = (h + 1) & mask) {
            if (atomicCAS(&tc[h].owner, 0ull, e.owner) != 0ull) continue;
            tc[h].value = e.value;
            tc[h].count = e.count;
            break;
        }
    }
    tally.flush(cnt);
}

static_assert(sizeof(CPBucket) == sizeof(uint4), "the move pass copies a bucket as one 16-byte vector");

static unsigned ggrid(uint64_t n, unsigned cap) {
    uint64_t g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

hipError_t launch_param_grow(const PRule* orules, const PSlot* old, uint64_t old_total, const PRule* nrules,
                             uint32_t n_rules, PSlot* table, uint64_t new_total, hipStream_t stream) {
    if (n_rules == 0 || new_total == 0) return hipSuccess;
    hipError_t e = launch_param_clear(table, new_total, stream);
    if (e != hipSuccess) return e;
    PArgs p{};
    p.rules = nrules;
    p.n_rules = n_rules;
    p.table = table;
    p.total_slots = new_total;
    hipLaunchKernelGGL(k_pgrow, dim3(ggrid(old_total, 8192)), dim3(256), 0, stream, p, orules, old, old_total);
    return hipGetLastError();
}

hipError_t launch_param_used(const PSlot* table, uint64_t base, uint64_t n, unsigned long long* out2, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ptable_used, dim3(ggrid(n, 2048)), dim3(256), 0, stream, table, base, n, out2);
    return hipGetLastError();
}

hipError_t launch_cp_grow(const CPArgs& nc, const CPRule* orules, uint64_t oper, const uint64_t* okeys,
                          const CPBucket* oring, uint64_t old_total, uint32_t* map, hipStream_t stream) {
    if (nc.n_rules == 0 || nc.total_slots == 0) return hipSuccess;
    hipError_t e = launch_cp_clear(nc.keys, nc.ring, nc.total_slots, nc.stride, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cpgrow_claim, dim3(ggrid(old_total, 8192)), dim3(256), 0, stream, nc, orules, oper, okeys, oring,
                       old_total, map);
    hipLaunchKernelGGL(k_cpgrow_move, dim3(ggrid(old_total * (uint64_t)nc.stride, 16384)), dim3(256), 0, stream, orules,
                       oper, reinterpret_cast<const uint4*>(oring), reinterpret_cast<uint4*>(nc.ring), nc.stride,
                       (const uint32_t*)map, old_total);
    return hipGetLastError();
}

hipError_t launch_param_sweep(const PRule* rules, uint32_t n_rules, const sg_param_hot_item* hot, const PSlot* old,
                              PSlot* table, uint64_t total, int64_t now, unsigned long long* cnt4, hipStream_t stream) {
    if (n_rules == 0 || total == 0) return hipSuccess;
    hipError_t e = launch_param_clear(table, total, stream);
    if (e != hipSuccess) return e;
    PArgs p{};
    p.rules = rules;
    p.n_rules = n_rules;
    p.hot = hot;
    p.table = table;
    p.total_slots = total;
    hipLaunchKernelGGL(k_psweep, dim3(ggrid(total, 8192)), dim3(256), 0, stream, p, old, now, cnt4);
    return hipGetLastError();
}

hipError_t launch_cp_sweep(const CPArgs& nc, const uint64_t* okeys, const CPBucket* oring, int64_t now, uint32_t* map,
                           unsigned long long* cnt4, hipStream_t stream) {
    if (nc.n_rules == 0 || nc.total_slots == 0) return hipSuccess;
    hipError_t e = launch_cp_clear(nc.keys, nc.ring, nc.total_slots, nc.stride, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cpsweep_claim, dim3(ggrid(nc.total_slots, 8192)), dim3(256), 0, stream, nc, okeys, oring, now, map,
                       cnt4);
    hipLaunchKernelGGL(k_cpgrow_move, dim3(ggrid(nc.total_slots * (uint64_t)nc.stride, 16384)), dim3(256), 0, stream,
                       nc.rules, nc.per, reinterpret_cast<const uint4*>(oring), reinterpret_cast<uint4*>(nc.ring),
                       nc.stride, (const uint32_t*)map, nc.total_slots);
    return hipGetLastError();
}

hipError_t launch_tc_sweep(const PSThread* old, PSThread* tc, uint64_t slots, unsigned long long* cnt4, hipStream_t stream) {
    if (slots == 0) return hipSuccess;
    hipError_t e = launch_pslot_clear(tc, slots, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tcsweep, dim3(ggrid(slots, 8192)), dim3(256), 0, stream, old, tc, slots, cnt4);
    return hipGetLastError();
}

hipError_t launch_cp_used(const uint64_t* keys, const CPBucket* ring, int stride, int S, uint64_t base, uint64_t n,
                          unsigned long long* out2, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cptable_used, dim3(ggrid(n, 2048)), dim3(256), 0, stream, keys, ring, stride, S, base, n, out2);
    return hipGetLastError();
}

}  // namespace sg
