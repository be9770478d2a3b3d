// serverlog_rules.h — the host-side arithmetic of the token server stat log (sentinel-server.log): the counter layout
// of a table slot, the expansion of a slot's non-zero counters into sg_server_row rows, the merge of rows with equal
// keys (a node handle's parts), the row order and the capacity contract of the fetch. No HIP in here: the device fills
// the counters (engine.h includes this file for their layout), api.cpp expands, merges and sorts, and
// tests/cpp/test_serverlog_host.cpp runs all of it on the CPU.
//
// ClusterServerStatLogUtil.log(key, count) (cluster/server/log/ClusterServerStatLogUtil.java:32-52) is one COUNT_SUM
// entry per key string and second. The keys of one decision share their flowId (ClusterFlowChecker.java:102-107 writes
// flow|block|id, flow|block_request|id and flow|occupied_block|id for one blocked prioritized request), so the table
// keeps one slot per (second, family, flowId, value) and the family's counters side by side in it; a row exists if and
// only if its counter is non-zero, because every request that reaches a checker has acquireCount >= 1
// (DefaultTokenService.notValidRequest, DefaultTokenService.java:87-93).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "../../include/sentinel_gpu.h"

namespace sg {

constexpr int kSlogCtrs = 6;               // counters of a slot (the largest family's)
constexpr uint32_t kSlogFlow = 0;          // counters: SG_SLOG_FLOW_WAITING .. SG_SLOG_FLOW_PASS_REQUEST, in that order
constexpr uint32_t kSlogParam = 1;         // SG_SLOG_PARAM_PASS, SG_SLOG_PARAM_BLOCK
constexpr uint32_t kSlogConc = 2;          // SG_SLOG_CONC_PASS, SG_SLOG_CONC_BLOCK, SG_SLOG_CONC_RELEASE
constexpr uint32_t kSlogFamilies = 3;

#ifdef __HIPCC__
#define SG_SLOG_HD __host__ __device__
#else
#define SG_SLOG_HD
#endif

// The event of a family's counter i, or -1 (the family has fewer counters). The one function here the device calls too
// (the fetch's count pass).
SG_SLOG_HD inline int32_t slog_event(uint32_t family, int i) {
    const int32_t base = family == kSlogFlow ? SG_SLOG_FLOW_WAITING : family == kSlogParam ? SG_SLOG_PARAM_PASS
                                                                                           : SG_SLOG_CONC_PASS;
    const int32_t count = family == kSlogFlow ? 6 : family == kSlogParam ? 2 : 3;
    if (family >= kSlogFamilies || i < 0 || i >= count) return -1;
    return base + i;
}

// A slot as the device hands it out: the key and the family's counters.
struct SlogCounters {
    int64_t ts;
    int64_t flow_id;
    uint64_t value;
    uint32_t family;
    int64_t c[kSlogCtrs];
};

// The rows of one slot: its non-zero counters, in event order.
inline uint64_t slog_row_count(const SlogCounters& s) {
    uint64_t n = 0;
    for (int i = 0; i < kSlogCtrs; ++i) n += slog_event(s.family, i) >= 0 && s.c[i] != 0;
    return n;
}

inline void slog_expand(const SlogCounters& s, std::vector<sg_server_row>& out) {
    for (int i = 0; i < kSlogCtrs; ++i) {
        const int32_t ev = slog_event(s.family, i);
        if (ev < 0 || s.c[i] == 0) continue;
        sg_server_row r{};
        r.timestamp = s.ts;
        r.count = s.c[i];
        r.flow_id = s.flow_id;
        r.value = s.value;
        r.event = ev;
        out.push_back(r);
    }
}

// Row order of the fetch: (timestamp, event, flow_id, value).
inline bool slog_row_less(const sg_server_row& x, const sg_server_row& y) {
    return std::tie(x.timestamp, x.event, x.flow_id, x.value) < std::tie(y.timestamp, y.event, y.flow_id, y.value);
}

inline bool slog_same_key(const sg_server_row& x, const sg_server_row& y) {
    return x.timestamp == y.timestamp && x.event == y.event && x.flow_id == y.flow_id && x.value == y.value;
}

// Sorts the rows and sums those with equal keys into one (the parts of a node handle: a rule served by the front and by
// a shard stays one row). A single handle's rows have distinct keys: for them this is the sort alone.
inline void slog_sort_merge(std::vector<sg_server_row>& rows) {
    std::sort(rows.begin(), rows.end(), slog_row_less);
    size_t w = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
        if (w > 0 && slog_same_key(rows[w - 1], rows[i])) rows[w - 1].count += rows[i].count;
        else rows[w++] = rows[i];
    }
    rows.resize(w);
}

// capacity_log2 of an enable call: 4..24.
inline bool slog_capacity_ok(int32_t capacity_log2) { return capacity_log2 >= 4 && capacity_log2 <= 24; }
inline uint64_t slog_slots(int32_t capacity_log2) { return (uint64_t)1 << capacity_log2; }

// The fetch's answer to the caller's cap for `needed` rows: SG_OK (the rows fit and are handed out) or SG_E_CAPACITY
// (*n_rows = needed, nothing else changes).
inline int slog_cap_answer(uint64_t needed, uint64_t cap, uint64_t* n_rows) {
    *n_rows = needed;
    return needed > cap ? SG_E_CAPACITY : SG_OK;
}

}  // namespace sg
