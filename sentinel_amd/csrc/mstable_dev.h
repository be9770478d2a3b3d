// mstable_dev.h — the batch's millisecond table on the device (MsTable, engine.h), shared by the hot-parameter and
// pace kernels: the prep kernel's update, the walkers' copy in LDS and the lookup request index → timestamp. `Args` is
// the batch's argument struct (PArgs, PaceArgs): its table `ms`, its requests `req` [n].
#pragma once
#include "engine.h"

namespace sg {

constexpr uint32_t kMsLds = 4096;  // millisecond table entries staged in LDS (a batch spanning <= 4 s)

// Request i (timestamp ts, the one before it tp, the batch's first t0) in a prep kernel: a new millisecond starts
// at i.
template <class Args>
__device__ __forceinline__ void ms_prep(const Args& p, uint64_t i, int64_t ts, int64_t tp, int64_t t0) {
    const MsTable& m = p.ms;
    if (i == 0) {
        *m.mt0 = ts;
    } else if (ts > tp) {
        for (int64_t ms = (tp < t0 ? t0 : tp) + 1; ms <= ts; ++ms) {
            const int64_t qq = ms - t0;
            if (qq >= (int64_t)kMaxPeriods) break;
            m.msb[qq] = (uint32_t)i;
        }
    }
    if (i == p.n - 1) *m.mnp = (uint32_t)min(ts - t0 + 1, (int64_t)kMaxPeriods + 1);
    if ((i & ((1ull << m.bshift) - 1ull)) == 0) m.mbk[i >> m.bshift] = (uint16_t)min(max(ts - t0, (int64_t)0), (int64_t)65535);
}

__shared__ uint32_t ms_sms[kMsLds];
__shared__ uint16_t ms_sbk[kPcBuckets];  // the millisecond of request b << bshift
__shared__ uint32_t ms_nms;  // table entries in LDS, 0: read the timestamps
__shared__ uint32_t ms_nbk;
__shared__ int64_t ms_t0;

// Every thread of a walker's block, before its first ms_ts.
template <class Args>
__device__ __forceinline__ void ms_stage(const Args& p) {
    const MsTable& m = p.ms;
    const uint32_t np = *m.mnp;
    const bool lds = np <= kMsLds;
    const uint32_t nb = (uint32_t)((p.n - 1) >> m.bshift) + 1;
    for (uint32_t x = threadIdx.x; lds && x < np; x += blockDim.x) ms_sms[x] = m.msb[x];
    for (uint32_t x = threadIdx.x; lds && x < nb; x += blockDim.x) ms_sbk[x] = m.mbk[x];
    if (threadIdx.x == 0) {
        ms_nms = lds ? np : 0u;
        ms_nbk = nb;
        ms_t0 = *m.mt0;
    }
    __syncthreads();
}

// Request idx's timestamp: the largest millisecond q whose first request index table[q] <= idx (entry 0 unused). Its
// bucket's first request and the next bucket's bound q to a few milliseconds (a bucket of a 16M batch holds 8192
// requests), so the binary search takes a step or two instead of twelve.
template <class Args>
__device__ __forceinline__ int64_t ms_ts(const Args& p, uint32_t idx) {
    const uint32_t np = ms_nms;
    if (np == 0) return p.req[idx].ts_ms;
    const uint32_t b = idx >> p.ms.bshift;
    uint32_t lo = ms_sbk[b], hi = b + 1 < ms_nbk ? (uint32_t)ms_sbk[b + 1] + 1u : np;
    while (hi - lo > 1) {  // last_le spelled out: through the template the walkers' code comes out differently
        const uint32_t mid = (lo + hi) >> 1;
        if (ms_sms[mid] <= idx) lo = mid;
        else hi = mid;
    }
    return ms_t0 + (int64_t)lo;
}

}  // namespace sg
