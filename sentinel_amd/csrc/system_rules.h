// system_rules.h — SystemSlot's thresholds and their host-side merge, and the key groups of the serial (system)
// rule image. No HIP in here: the device reads LSysConf (engine.h includes this file), the C ABI merges
// sg_system_rule arrays into it, and tests/cpp/test_system_host.cpp runs both on the CPU.
//
// SystemRuleManager.SystemPropertyListener.configUpdate (SystemRuleManager.java:183-227): restoreSetting, then
// loadSystemConf (:244-282) of every rule in list order — each field that is >= 0 lowers its threshold (Math.min),
// highestCpuUsage > 1 is ignored, and checkSystemStatus is SET (not or-ed) by every rule: the last rule decides it.
// An empty (or null) list leaves checking off.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <vector>

#include "../../include/sentinel_gpu.h"

namespace sg {

struct LSysConf {
    double qps;            // Double.MAX_VALUE when not set
    double highest_load;
    double highest_cpu;
    int64_t max_rt;        // Long.MAX_VALUE when not set
    int64_t max_thread;
    int32_t check;         // checkSystemStatus
    int32_t load_set;      // highestSystemLoadIsSet
    int32_t cpu_set;       // highestCpuUsageIsSet
    int32_t pad_;
};

inline LSysConf system_defaults() {  // restoreSetting
    LSysConf c{};
    c.qps = DBL_MAX;
    c.highest_load = DBL_MAX;
    c.highest_cpu = DBL_MAX;
    c.max_rt = INT64_MAX;
    c.max_thread = INT64_MAX;
    return c;
}

inline LSysConf system_merge(const sg_system_rule* rules, uint32_t n) {
    LSysConf c = system_defaults();
    for (uint32_t i = 0; i < n; ++i) {
        const sg_system_rule& r = rules[i];
        bool status = false;
        if (r.highest_system_load >= 0) {
            c.highest_load = std::min(c.highest_load, r.highest_system_load);
            c.load_set = 1;
            status = true;
        }
        if (r.highest_cpu_usage >= 0 && !(r.highest_cpu_usage > 1)) {
            c.highest_cpu = std::min(c.highest_cpu, r.highest_cpu_usage);
            c.cpu_set = 1;
            status = true;
        }
        if (r.avg_rt >= 0) {
            c.max_rt = std::min(c.max_rt, r.avg_rt);
            status = true;
        }
        if (r.max_thread >= 0) {
            c.max_thread = std::min(c.max_thread, r.max_thread);
            status = true;
        }
        if (r.qps >= 0) {
            c.qps = std::min(c.qps, r.qps);
            status = true;
        }
        c.check = status ? 1 : 0;
    }
    return c;
}

// Record keys of the system image: SystemSlot reads ENTRY_NODE, which every inbound resource writes, so all inbound
// resources walk on one lane in event order — one key group, united with every group (gkey: RELATE, embedded-server
// sharing) that holds one of them. gkey[k] is the smallest resource of k's group; so is the result. in_group[k] = 1
// for the members of the united group.
inline void system_group_keys(const std::vector<uint32_t>& gkey, const std::vector<uint8_t>& inbound,
                              std::vector<uint32_t>& out, std::vector<uint8_t>& in_group) {
    const size_t K = gkey.size();
    out = gkey;
    in_group.assign(K, 0);
    std::vector<uint8_t> hit(K, 0);  // group roots with an inbound member
    uint32_t root = UINT32_MAX;
    for (size_t k = 0; k < K; ++k) {
        if (k >= inbound.size() || !inbound[k] || gkey[k] >= K) continue;
        hit[gkey[k]] = 1;
        root = std::min(root, gkey[k]);
    }
    for (size_t k = 0; k < K; ++k) {
        if (gkey[k] < K && hit[gkey[k]]) {
            out[k] = root;
            in_group[k] = 1;
        }
    }
}

}  // namespace sg
