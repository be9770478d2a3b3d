// TEST INFRASTRUCTURE: the host-only part of SystemSlot (sentinel_amd/csrc/system_rules.h) on the CPU, built with the
// address and undefined-behaviour sanitizers by tests/cpp/system_host.mk: the rule merge (loadSystemConf) and the
// record keys of the system image.
#include <cstdio>
#include <cstdlib>

#include "../../sentinel_amd/csrc/system_rules.h"

using namespace sg;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static sg_system_rule rule(double load, double cpu, double qps, int64_t rt, int64_t thr) {
    sg_system_rule r;
    r.highest_system_load = load;
    r.highest_cpu_usage = cpu;
    r.qps = qps;
    r.avg_rt = rt;
    r.max_thread = thr;
    return r;
}

int main() {
    {  // an empty list: defaults, checking off
        const LSysConf c = system_merge(nullptr, 0);
        CHECK(!c.check && !c.load_set && !c.cpu_set);
        CHECK(c.qps == DBL_MAX && c.highest_load == DBL_MAX && c.highest_cpu == DBL_MAX);
        CHECK(c.max_rt == INT64_MAX && c.max_thread == INT64_MAX);
    }
    {  // every field negative: invalid, nothing stored
        const sg_system_rule r[] = {rule(-1, -1, -4, -2, -3)};
        const LSysConf c = system_merge(r, 1);
        CHECK(!c.check && c.qps == DBL_MAX && c.max_rt == INT64_MAX && c.max_thread == INT64_MAX);
    }
    {  // the minimum of duplicates
        const sg_system_rule r[] = {rule(4, -1, 500, 300, 40), rule(3, -1, 800, 100, 60)};
        const LSysConf c = system_merge(r, 2);
        CHECK(c.check && c.load_set && !c.cpu_set);
        CHECK(c.highest_load == 3 && c.qps == 500 && c.max_rt == 100 && c.max_thread == 40);
    }
    {  // cpu > 1 ignored; the last rule decides the status
        const sg_system_rule r[] = {rule(-1, 0.6, -1, -1, -1), rule(-1, 1.0, -1, -1, -1), rule(-1, 1.0001, -1, -1, -1)};
        LSysConf c = system_merge(r, 3);
        CHECK(c.cpu_set && c.highest_cpu == 0.6 && !c.check);
        c = system_merge(r, 2);
        CHECK(c.check);
        const sg_system_rule q[] = {rule(-1, -1, 10, -1, -1), rule(-1, -1, -1, -1, -1)};
        c = system_merge(q, 2);
        CHECK(!c.check && c.qps == 10);
        const sg_system_rule z[] = {rule(-1, -1, 0, -1, -1)};
        c = system_merge(z, 1);
        CHECK(c.check && c.qps == 0);
    }
    {  // key groups: resources 1, 4 inbound; RELATE groups {2, 4} and {5, 6}
        const std::vector<uint32_t> gkey = {0, 1, 2, 3, 2, 5, 5};
        const std::vector<uint8_t> inbound = {0, 1, 0, 0, 1, 0, 0};
        std::vector<uint32_t> out;
        std::vector<uint8_t> in;
        system_group_keys(gkey, inbound, out, in);
        CHECK((out == std::vector<uint32_t>{0, 1, 1, 3, 1, 5, 5}));
        CHECK((in == std::vector<uint8_t>{0, 1, 1, 0, 1, 0, 0}));
        // one inbound resource alone is still a group of the image; none: the keys stay
        system_group_keys({0, 1, 2}, {0, 0, 1}, out, in);
        CHECK((out == std::vector<uint32_t>{0, 1, 2}) && (in == std::vector<uint8_t>{0, 0, 1}));
        system_group_keys({0, 0, 2}, {0, 0, 0}, out, in);
        CHECK((out == std::vector<uint32_t>{0, 0, 2}) && (in == std::vector<uint8_t>{0, 0, 0}));
        system_group_keys({0, 1}, {1}, out, in);  // a short entry-type array: the rest is outbound
        CHECK((out == std::vector<uint32_t>{0, 1}) && (in == std::vector<uint8_t>{1, 0}));
        system_group_keys({}, {}, out, in);
        CHECK(out.empty() && in.empty());
    }
    std::printf("system host ok\n");
    return 0;
}
