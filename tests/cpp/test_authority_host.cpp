// TEST INFRASTRUCTURE: the host-only compiler of AuthoritySlot's rule table (sentinel_amd/csrc/authority_rules.h) on
// the CPU, no GPU and no HIP. Built with -fsanitize=address,undefined by tests/cpp/authority_host.mk; run by
// tests/test_authority_host.py. Expectations restate AuthorityRuleManagerTest / AuthorityRuleCheckerTest in our own
// words: validity (isValidRule), the first valid rule of a resource wins, exact item match.
#include <cstdio>
#include <vector>

#include "../../sentinel_amd/csrc/authority_rules.h"

using namespace sg;

static int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++g_fail;                                                   \
        }                                                               \
    } while (0)

static sg_authority_rule rule(uint32_t res, int32_t strategy, uint32_t begin, uint32_t count) {
    sg_authority_rule r;
    r.resource = res;
    r.strategy = strategy;
    r.origin_begin = begin;
    r.origin_count = count;
    return r;
}

int main() {
    std::vector<LAuth> tab;
    std::vector<int32_t> ids;

    {  // white and black lists; an empty origin passes; a resource without a rule passes everybody
        const int32_t og[] = {1, 3, 2};
        const sg_authority_rule rs[] = {rule(0, SG_AUTHORITY_WHITE, 0, 2), rule(1, SG_AUTHORITY_BLACK, 2, 1)};
        CHECK(authority_compile(rs, 2, og, 3, 3, tab, ids) == 2);
        CHECK(tab.size() == 3 && ids.empty());
        CHECK(!authority_rejects(tab[0], ids.data(), 1) && !authority_rejects(tab[0], ids.data(), 3));
        CHECK(authority_rejects(tab[0], ids.data(), 2) && authority_rejects(tab[0], ids.data(), 77));
        CHECK(authority_rejects(tab[1], ids.data(), 2) && !authority_rejects(tab[1], ids.data(), 1));
        for (int r = 0; r < 3; ++r) CHECK(!authority_rejects(tab[r], ids.data(), 0));
        for (int o = 0; o < 5; ++o) CHECK(!authority_rejects(tab[2], ids.data(), o));
    }
    {  // invalid rules are ignored and do not take the resource's slot: strategy < 0, blank limitApp
        const int32_t og[] = {1, 2};
        const sg_authority_rule rs[] = {rule(0, -1, 0, 1), rule(0, SG_AUTHORITY_BLACK, 0, 0),
                                        rule(0, SG_AUTHORITY_BLACK, 1, 1)};
        CHECK(authority_compile(rs, 3, og, 2, 1, tab, ids) == 1);
        CHECK(authority_rejects(tab[0], ids.data(), 2) && !authority_rejects(tab[0], ids.data(), 1));
    }
    {  // first wins: the second rule of a resource is redundant; a strategy other than 0 / 1 never blocks but shadows
        const int32_t og[] = {1, 2};
        const sg_authority_rule rs[] = {rule(0, SG_AUTHORITY_WHITE, 0, 1), rule(0, SG_AUTHORITY_BLACK, 0, 1),
                                        rule(1, 2, 0, 1), rule(1, SG_AUTHORITY_BLACK, 0, 2)};
        CHECK(authority_compile(rs, 4, og, 2, 2, tab, ids) == 2);
        CHECK(!authority_rejects(tab[0], ids.data(), 1) && authority_rejects(tab[0], ids.data(), 2));
        CHECK((tab[1].cs >> 30) == kAuthNever);
        CHECK(!authority_rejects(tab[1], ids.data(), 1) && !authority_rejects(tab[1], ids.data(), 2));
    }
    {  // ids above 64 go to the sorted tail, per resource, duplicates dropped; 64 is the mask's last bit
        const int32_t og[] = {200, 64, 65, 200, 65, 1, 1000000, 66};
        const sg_authority_rule rs[] = {rule(0, SG_AUTHORITY_BLACK, 0, 6), rule(1, SG_AUTHORITY_WHITE, 6, 2)};
        CHECK(authority_compile(rs, 2, og, 8, 2, tab, ids) == 2);
        CHECK(ids.size() == 4 && ids[0] == 65 && ids[1] == 200 && ids[2] == 66 && ids[3] == 1000000);
        CHECK(tab[0].begin == 0 && (tab[0].cs & kAuthCount) == 2 && tab[1].begin == 2 && (tab[1].cs & kAuthCount) == 2);
        CHECK(tab[0].mask == ((1ull << 63) | 1ull));
        for (int32_t o : {1, 64, 65, 200}) CHECK(authority_rejects(tab[0], ids.data(), o));
        for (int32_t o : {2, 63, 66, 199, 201, 1000000}) CHECK(!authority_rejects(tab[0], ids.data(), o));
        for (int32_t o : {66, 1000000}) CHECK(!authority_rejects(tab[1], ids.data(), o));
        for (int32_t o : {1, 64, 65, 67, 200, 2147483647}) CHECK(authority_rejects(tab[1], ids.data(), o));
    }
    {  // refused loads leave the caller's table untouched
        const int32_t og[] = {1, 0, -3, 2};
        const std::vector<LAuth> before = tab;
        const std::vector<int32_t> ids_before = ids;
        const sg_authority_rule bad_res[] = {rule(2, SG_AUTHORITY_BLACK, 0, 1)};
        CHECK(authority_compile(bad_res, 1, og, 4, 2, tab, ids) == SG_E_INVAL);
        const sg_authority_rule bad_range[] = {rule(0, SG_AUTHORITY_BLACK, 3, 2)};
        CHECK(authority_compile(bad_range, 1, og, 4, 2, tab, ids) == SG_E_INVAL);
        const sg_authority_rule wrap_range[] = {rule(0, SG_AUTHORITY_BLACK, 0xFFFFFFFFu, 2)};
        CHECK(authority_compile(wrap_range, 1, og, 4, 2, tab, ids) == SG_E_INVAL);
        const sg_authority_rule zero_id[] = {rule(0, SG_AUTHORITY_BLACK, 0, 2)};
        CHECK(authority_compile(zero_id, 1, og, 4, 2, tab, ids) == SG_E_INVAL);
        const sg_authority_rule neg_id[] = {rule(0, SG_AUTHORITY_WHITE, 2, 1)};
        CHECK(authority_compile(neg_id, 1, og, 4, 2, tab, ids) == SG_E_INVAL);
        CHECK(tab.size() == before.size() && ids == ids_before);
        for (size_t i = 0; i < tab.size(); ++i)
            CHECK(tab[i].mask == before[i].mask && tab[i].begin == before[i].begin && tab[i].cs == before[i].cs);
    }
    {  // an empty load clears
        CHECK(authority_compile(nullptr, 0, nullptr, 0, 2, tab, ids) == 0);
        CHECK(tab.size() == 2 && ids.empty());
        for (int r = 0; r < 2; ++r)
            for (int32_t o : {1, 65}) CHECK(!authority_rejects(tab[r], ids.data(), o));
    }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("authority host ok\n");
    return 0;
}
