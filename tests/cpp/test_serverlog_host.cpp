// TEST INFRASTRUCTURE: the host-only arithmetic of the token server stat log (sentinel_amd/csrc/serverlog_rules.h) on
// the CPU, under the address and undefined-behaviour sanitizers: the expansion of a slot's counters into rows, the
// merge of equal keys, the row order, the capacity arithmetic and the answer to a cap that is too small. No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sentinel_amd/csrc/serverlog_rules.h"

using namespace sg;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static SlogCounters slot(int64_t ts, uint32_t family, int64_t fid, uint64_t value, std::vector<int64_t> c) {
    SlogCounters s{};
    s.ts = ts;
    s.family = family;
    s.flow_id = fid;
    s.value = value;
    for (size_t i = 0; i < c.size() && i < (size_t)kSlogCtrs; ++i) s.c[i] = c[i];
    return s;
}

static sg_server_row row(int64_t ts, int32_t ev, int64_t fid, uint64_t value, int64_t count) {
    sg_server_row r{};
    r.timestamp = ts;
    r.event = ev;
    r.flow_id = fid;
    r.value = value;
    r.count = count;
    return r;
}

static bool same(const sg_server_row& x, const sg_server_row& y) {
    return slog_same_key(x, y) && x.count == y.count && x.reserved == y.reserved;
}

int main() {
    {  // the counters of each family name the events of the header, in its order
        CHECK(slog_event(kSlogFlow, 0) == SG_SLOG_FLOW_WAITING && slog_event(kSlogFlow, 1) == SG_SLOG_FLOW_BLOCK);
        CHECK(slog_event(kSlogFlow, 2) == SG_SLOG_FLOW_BLOCK_REQUEST);
        CHECK(slog_event(kSlogFlow, 3) == SG_SLOG_FLOW_OCCUPIED_BLOCK);
        CHECK(slog_event(kSlogFlow, 4) == SG_SLOG_FLOW_PASS && slog_event(kSlogFlow, 5) == SG_SLOG_FLOW_PASS_REQUEST);
        CHECK(slog_event(kSlogParam, 0) == SG_SLOG_PARAM_PASS && slog_event(kSlogParam, 1) == SG_SLOG_PARAM_BLOCK);
        CHECK(slog_event(kSlogParam, 2) == -1);
        CHECK(slog_event(kSlogConc, 0) == SG_SLOG_CONC_PASS && slog_event(kSlogConc, 1) == SG_SLOG_CONC_BLOCK);
        CHECK(slog_event(kSlogConc, 2) == SG_SLOG_CONC_RELEASE && slog_event(kSlogConc, 3) == -1);
        CHECK(slog_event(kSlogFlow, -1) == -1 && slog_event(kSlogFlow, kSlogCtrs) == -1);
        CHECK(slog_event(kSlogFamilies, 0) == -1);
    }
    {  // expansion: a row per non-zero counter, in event order; zero counters make no row
        std::vector<sg_server_row> out;
        const SlogCounters blocked_prio = slot(5000, kSlogFlow, 123, 0, {0, 7, 2, 1, 0, 0});
        CHECK(slog_row_count(blocked_prio) == 3);
        slog_expand(blocked_prio, out);
        CHECK(out.size() == 3);
        CHECK(same(out[0], row(5000, SG_SLOG_FLOW_BLOCK, 123, 0, 7)));
        CHECK(same(out[1], row(5000, SG_SLOG_FLOW_BLOCK_REQUEST, 123, 0, 2)));
        CHECK(same(out[2], row(5000, SG_SLOG_FLOW_OCCUPIED_BLOCK, 123, 0, 1)));
        out.clear();
        const SlogCounters empty = slot(5000, kSlogFlow, 9, 0, {});
        CHECK(slog_row_count(empty) == 0);
        slog_expand(empty, out);
        CHECK(out.empty());
        const SlogCounters all = slot(1000, kSlogFlow, 1, 0, {1, 2, 3, 4, 5, 6});
        CHECK(slog_row_count(all) == 6);
        slog_expand(all, out);
        CHECK(out.size() == 6);
        for (int i = 0; i < 6; ++i) CHECK(out[i].event == i && out[i].count == i + 1);
        out.clear();
        // a param slot carries its value; counters past the family's are never rows, whatever they hold
        const SlogCounters p = slot(2000, kSlogParam, 44, 0xFFFFFFFFFFFFFFFFull, {0, 3, 99, 99, 99, 99});
        CHECK(slog_row_count(p) == 1);
        slog_expand(p, out);
        CHECK(out.size() == 1 && same(out[0], row(2000, SG_SLOG_PARAM_BLOCK, 44, 0xFFFFFFFFFFFFFFFFull, 3)));
        out.clear();
        const SlogCounters c = slot(3000, kSlogConc, 8, 0, {5, 0, (int64_t)1 << 40});
        slog_expand(c, out);
        CHECK(out.size() == 2 && same(out[0], row(3000, SG_SLOG_CONC_PASS, 8, 0, 5)));
        CHECK(same(out[1], row(3000, SG_SLOG_CONC_RELEASE, 8, 0, (int64_t)1 << 40)));
        out.clear();
        const SlogCounters bad = slot(3000, 7, 8, 0, {5, 5, 5, 5, 5, 5});  // an unknown family has no events
        CHECK(slog_row_count(bad) == 0);
        slog_expand(bad, out);
        CHECK(out.empty());
    }
    {  // sort order: (timestamp, event, flow_id, value), the value as unsigned, the flowId as signed
        std::vector<sg_server_row> r = {
            row(2000, SG_SLOG_FLOW_BLOCK, 5, 0, 1),        row(1000, SG_SLOG_PARAM_BLOCK, 5, 0x8000000000000000ull, 2),
            row(1000, SG_SLOG_PARAM_BLOCK, 5, 3, 3),       row(1000, SG_SLOG_FLOW_BLOCK_REQUEST, 9, 0, 4),
            row(1000, SG_SLOG_FLOW_BLOCK_REQUEST, 2, 0, 5), row(1000, SG_SLOG_FLOW_WAITING, 1ll << 40, 0, 6),
            row(1000, SG_SLOG_FLOW_WAITING, 7, 0, 7),
        };
        slog_sort_merge(r);
        const int64_t want[] = {7, 6, 5, 4, 3, 2, 1};
        CHECK(r.size() == 7);
        for (size_t i = 0; i < r.size(); ++i) CHECK(r[i].count == want[i]);
        for (size_t i = 1; i < r.size(); ++i) CHECK(slog_row_less(r[i - 1], r[i]) && !slog_row_less(r[i], r[i - 1]));
    }
    {  // merge: equal keys become one row with the summed count (past 2^31 too); other fields must all match
        std::vector<sg_server_row> r = {
            row(1000, SG_SLOG_FLOW_BLOCK, 5, 0, 0x7FFFFFFF), row(1000, SG_SLOG_FLOW_BLOCK, 6, 0, 1),
            row(1000, SG_SLOG_FLOW_BLOCK, 5, 0, 0x7FFFFFFF), row(2000, SG_SLOG_FLOW_BLOCK, 5, 0, 2),
            row(1000, SG_SLOG_FLOW_BLOCK_REQUEST, 5, 0, 3),  row(1000, SG_SLOG_FLOW_BLOCK, 5, 0, 4),
            row(1000, SG_SLOG_PARAM_BLOCK, 5, 1, 5),         row(1000, SG_SLOG_PARAM_BLOCK, 5, 2, 6),
            row(1000, SG_SLOG_PARAM_BLOCK, 5, 1, 7),
        };
        slog_sort_merge(r);
        CHECK(r.size() == 6);
        CHECK(same(r[0], row(1000, SG_SLOG_FLOW_BLOCK, 5, 0, 2ll * 0x7FFFFFFF + 4)));
        CHECK(same(r[1], row(1000, SG_SLOG_FLOW_BLOCK, 6, 0, 1)));
        CHECK(same(r[2], row(1000, SG_SLOG_FLOW_BLOCK_REQUEST, 5, 0, 3)));
        CHECK(same(r[3], row(1000, SG_SLOG_PARAM_BLOCK, 5, 1, 12)));
        CHECK(same(r[4], row(1000, SG_SLOG_PARAM_BLOCK, 5, 2, 6)));
        CHECK(same(r[5], row(2000, SG_SLOG_FLOW_BLOCK, 5, 0, 2)));
        std::vector<sg_server_row> none;
        slog_sort_merge(none);
        CHECK(none.empty());
        std::vector<sg_server_row> one = {row(1, 0, 1, 0, 1)};
        slog_sort_merge(one);
        CHECK(one.size() == 1);
    }
    {  // capacity arithmetic: 4..24, 2^4 and 2^24 slots
        CHECK(!slog_capacity_ok(3) && slog_capacity_ok(4) && slog_capacity_ok(24) && !slog_capacity_ok(25));
        CHECK(!slog_capacity_ok(-1) && !slog_capacity_ok(0) && !slog_capacity_ok(64));
        CHECK(slog_slots(4) == 16 && slog_slots(24) == 16777216ull);
        CHECK(slog_slots(4) - 1 == 0xF && slog_slots(24) - 1 == 0xFFFFFF);  // the probe masks
    }
    {  // the cap-too-small answer: SG_E_CAPACITY with the rows needed; a fitting cap (0 rows into a null buffer too)
        uint64_t n = 99;
        CHECK(slog_cap_answer(5, 4, &n) == SG_E_CAPACITY && n == 5);
        CHECK(slog_cap_answer(5, 5, &n) == SG_OK && n == 5);
        CHECK(slog_cap_answer(0, 0, &n) == SG_OK && n == 0);
        CHECK(slog_cap_answer(1, 0, &n) == SG_E_CAPACITY && n == 1);
        CHECK(slog_cap_answer(6ull << 24, 1ull << 24, &n) == SG_E_CAPACITY && n == (6ull << 24));
    }
    std::printf("serverlog host ok\n");
    return 0;
}
