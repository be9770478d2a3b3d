// TEST INFRASTRUCTURE: sentinel_amd/csrc/vdict_sweep.h on the CPU against a brute-force restatement — a dictionary
// modelled as a plain array of live / free flags that hands out ids by searching for the lowest free one. Its own
// main, no GPU, no HIP; built by vdict_sweep_host.mk under the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sentinel_amd/csrc/vdict_sweep.h"

using namespace sg;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                             \
        }                                                           \
    } while (0)

// The model: state[id] for id in [1, high]: true = live. A fresh value takes the lowest free id, else high + 1.
struct Model {
    std::vector<bool> live{false};  // index 0 unused
    uint64_t high() const { return live.size() - 1; }
    uint64_t take() {
        for (uint64_t id = 1; id <= high(); ++id)
            if (!live[id]) {
                live[id] = true;
                return id;
            }
        live.push_back(true);
        return high();
    }
    uint64_t n_live() const {
        uint64_t n = 0;
        for (uint64_t id = 1; id <= high(); ++id) n += live[id];
        return n;
    }
};

// Every (high, free pattern over [1, high]) up to kHigh, every batch size up to kFresh: the ids of vd_next_id per rank
// equal the model's one-at-a-time search, and vd_after_batch lands on the model's counters.
static void id_rule_and_bookkeeping() {
    constexpr uint64_t kHigh = 7, kFresh = 10;
    for (uint64_t high = 0; high <= kHigh; ++high)
        for (uint64_t pattern = 0; pattern < (1ull << high); ++pattern) {
            Model m0;
            std::vector<uint32_t> free_ids;
            for (uint64_t id = 1; id <= high; ++id) {
                const bool is_free = (pattern >> (id - 1)) & 1;
                m0.live.push_back(!is_free);
                if (is_free) free_ids.push_back((uint32_t)id);
            }
            // the list as a sweep wrote it, with `head` of its entries taken already: put that many back in front
            for (uint64_t head = 0; head <= 2; ++head) {
                std::vector<uint32_t> list(head, 0xDEADu);
                list.insert(list.end(), free_ids.begin(), free_ids.end());
                for (uint64_t fresh = 0; fresh <= kFresh; ++fresh) {
                    Model m = m0;
                    const uint64_t n_free = free_ids.size();
                    for (uint64_t r = 0; r < fresh; ++r)
                        CHECK(vd_next_id(r, list.data() + head, n_free, high) == m.take());
                    const VdBook b = vd_after_batch(VdBook{head, n_free, high, high - n_free}, fresh);
                    CHECK(b.high == m.high());
                    CHECK(b.live == m.n_live());
                    CHECK(b.n_free == m.high() - m.n_live());
                    CHECK(b.head - head == n_free - b.n_free);
                    CHECK(b.high == b.live + b.n_free);
                    // a second batch continues where the first stopped
                    if (fresh <= 3) {
                        for (uint64_t r = 0; r < 3; ++r)
                            CHECK(vd_next_id(r, list.data() + b.head, b.n_free, b.high) == m.take());
                    }
                }
            }
        }
    // an empty free list: every id is high + 1 + rank, with a null list
    for (uint64_t high = 0; high < 5; ++high)
        for (uint64_t r = 0; r < 5; ++r) CHECK(vd_next_id(r, nullptr, 0, high) == high + 1 + r);
    // the largest ids: 2^28 values
    const uint32_t top[1] = {1u << 28};
    CHECK(vd_next_id(0, top, 1, 1ull << 28) == (1ull << 28));
    CHECK(vd_next_id(1, top, 1, 1ull << 28) == (1ull << 28) + 1);
}

static void refusal_order() {
    for (int on = 0; on < 2; ++on)
        for (uint64_t n_keep = 0; n_keep < 3; ++n_keep)
            for (int null = 0; null < 2; ++null)
                for (uint64_t bad = 0; bad < 3; ++bad) {
                    const VdsRefusal r = vd_sweep_refusal(on, n_keep, null, bad);
                    // restated: the first that applies of — no dictionary, a list promised and not given, a bad entry
                    const char first = !on ? 'i' : (n_keep > 0 && null) ? 'n' : bad ? 'b' : 0;
                    CHECK((r.code == kVdsOk) == (first == 0));
                    CHECK(r.code == kVdsOk || r.code == kVdsInval);
                    CHECK(r.why != nullptr);
                    if (first) CHECK(r.why[0] == (first == 'i' ? 's' : first == 'n' ? 'n' : 'a'));
                }
    CHECK(kVdsInval == -1 && kVdsOk == 0);
}

static void predicates() {
    for (uint64_t high = 0; high <= 4; ++high)
        for (uint64_t id : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, ~0ull, 1ull << 32, 1ull << 63}) {
            const bool in = id != 0 && id <= high;
            CHECK(vd_id_in_range(id, high) == in);
            CHECK(vd_keep_bad(id, high, false) == !in);
            CHECK(vd_keep_bad(id, high, true));
        }
    CHECK(!vd_thread_names_id(0));
    CHECK(vd_thread_names_id(1) && vd_thread_names_id(1ull << 32 | 1) && vd_thread_names_id(~0ull));
    const uint64_t tags[] = {0, 1 /* busy */, 0x7FFFFFFFFFFFFFFFull, 1ull << 63, ~0ull};
    for (uint64_t tag : tags)
        for (uint32_t k = 0; k <= 8; ++k) {
            const bool published = tag >= (1ull << 63);
            CHECK(vd_blog_names_id(tag, k) == (published && (k == 3 || k == 6)));  // SG_BLOCK_APP_VALUE, _LABEL
            CHECK(vd_slog_names_id(tag, k) == (published && k == 1));              // the param family
        }
    CHECK(kVdTombType > 7u);  // above every SG_PARAM_TYPE_*
    CHECK(kVdsCoopMin >= 16u);
}

int main() {
    id_rule_and_bookkeeping();
    refusal_order();
    predicates();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("vdict sweep host ok\n");
    return 0;
}
