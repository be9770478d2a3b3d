// system_dev.h — SystemSlot on the device (included by local.hip inside namespace sg, after its bcast helpers).
//
// SystemSlot (@Spi order -5000: after AuthoritySlot, before ParamFlowSlot) runs SystemRuleManager.checkSystem
// (SystemRuleManager.java:290-340) for every EntryType.IN entry against Constants.ENTRY_NODE, the StatisticNode that
// StatisticSlot updates for every inbound event (StatisticSlot.java:71-75, 88-91, 106-109, 139-141). Three pieces:
//
//   sys_check / sys_entry / sys_exit   the exact check and updates, one event at a time, on ENTRY_NODE in memory —
//                                      called by cx_entry / cx_exit when the batch walks the system image (serial
//                                      path: every inbound resource in one key group, one lane, event order).
//   k_sys_scan                         the clear proof: from the batch alone (exits are given; passes cannot exceed
//                                      arrivals) bounds of what every inbound entry's check would read; a batch no
//                                      entry of which can trip a threshold keeps the parallel walkers.
//   k_sys_apply_*                      after such a batch: ENTRY_NODE's buckets and thread count from the events and
//                                      their results, equal to what the serial path leaves.
#pragma once

namespace {

// ---- ENTRY_NODE's second window: a plain BucketLeapArray in effect (its borrow array stays empty) ----

// LeapArray.currentWindow(t) (LeapArray.java:116-202): the bucket of t's window, created or reset when it holds an
// older one. (A newer one cannot be there: batches are time-ordered.)
__device__ __forceinline__ LBucket* sys_current(LSys& s, int S, int32_t wl, int64_t t) {
    const int64_t P = t / wl;
    LBucket* b = s.sec + (int)(P % S);
    const int64_t ws = P * wl;
    if (b->start != ws) {
        b->start = ws;
        for (int e = 0; e < kLEv; ++e) b->c[e] = 0;
        b->min_rt = kStatMaxRt;
    }
    return b;
}

// values(t) after currentWindow(t): the buckets whose window is not deprecated — start >= windowStart(t) - (S-1)·wl
__device__ __forceinline__ bool sys_valid(int64_t start, int64_t t, int S, int32_t wl) {
    return start != INT64_MIN && start >= t - t % wl - (int64_t)(S - 1) * wl;
}

// checkSystem for one inbound entry at t: -1 passes, else the SG_SYSTEM_* limit type it throws with. Every ArrayMetric
// read calls currentWindow first; one call here serves them all (same t).
__device__ int sys_check(LSys& s, int S, int32_t wl, double isec, int64_t t, int32_t count) {
    sys_current(s, S, wl, t);
    int64_t pass = 0, succ = 0, rt = 0, max_succ = 0, min_rt = kStatMaxRt;
    for (int j = 0; j < S; ++j) {
        const LBucket b = s.sec[j];
        if (!sys_valid(b.start, t, S, wl)) continue;
        pass += b.c[kLPass];
        succ += b.c[kLSucc];
        rt += b.c[kLRt];
        if (b.c[kLSucc] > max_succ) max_succ = b.c[kLSucc];
        if (b.min_rt < min_rt) min_rt = b.min_rt;
    }
    const LSysConf& c = s.conf;
    const double qps = avg_div((double)pass, isec);                 // passQps()
    if (qps + (double)count > c.qps) return SG_SYSTEM_QPS;
    const int32_t threads = (int32_t)s.threads;                     // (int) curThreadNum.sum()
    if ((int64_t)threads > c.max_thread) return SG_SYSTEM_THREAD;
    const double avg_rt = succ == 0 ? 0.0 : (double)rt * 1.0 / (double)succ;
    if (avg_rt > (double)c.max_rt) return SG_SYSTEM_RT;
    if (c.load_set && s.load > c.highest_load) {                     // checkBbr
        if (max_succ < 1) max_succ = 1;
        if (min_rt < 1) min_rt = 1;
        const double max_succ_qps = (double)max_succ * (double)S / isec;
        if (threads > 1 && (double)threads > max_succ_qps * (double)min_rt / 1000.0) return SG_SYSTEM_LOAD;
    }
    if (c.cpu_set && s.cpu > c.highest_cpu) return SG_SYSTEM_CPU;
    return -1;
}

// StatisticSlot's ENTRY_NODE updates of one decided inbound entry
__device__ void sys_entry(LSys& s, int S, int32_t wl, int64_t t, int32_t count, int32_t status) {
    if (status == SG_LOCAL_PASS) {
        s.threads += 1;
        sys_current(s, S, wl, t)->c[kLPass] += count;
    } else if (status == SG_LOCAL_PASS_WAIT) {
        s.threads += 1;
    } else {
        sys_current(s, S, wl, t)->c[kLBlock] += count;
    }
}

// ... and of one inbound exit
__device__ void sys_exit(LSys& s, int S, int32_t wl, int64_t t, int64_t create, int32_t count, bool error) {
    LBucket* b = sys_current(s, S, wl, t);
    const int64_t rt = t - create;
    b->c[kLSucc] += count;
    b->c[kLRt] += rt;
    if (rt < b->min_rt) b->min_rt = rt;
    if (error) b->c[kLExc] += count;
    s.threads -= 1;
}

// ---- the clear proof ----
//
// One block walks the batch in time order, kSysScanItems consecutive events per thread and chunk, with block-wide
// exclusive prefix sums of: inbound entry counts E (negative counts as 0), inbound entries N, inbound exits X, and
// the exits' RT and success counts R, U. At the first event of every window period q of the batch the prefixes E, U, R
// are kept (pb[.][q]), so a window sum at entry i is prefix(i) - pb[q_i - (S-1)]. With ENTRY_NODE's buckets B and
// thread count T0 at batch start, for an inbound entry i at time t:
//
//   pass()       <= Σ valid B.pass + E(i) - pbE      every pass of the batch is an arrival of the batch; a bucket of B
//                                                    that is valid at t was not reset before t (a reset of its slot
//                                                    needs a window S periods later, which deprecates it)
//   curThreadNum <= T0 + N(i) - X(i)                 exits are given events; a blocked entry adds no thread
//   avgRt         = (Σ valid B.rt + R(i) - pbR) / (Σ valid B.success + U(i) - pbU), exact: exits are given events
//
// The double expressions of checkSystem are monotone in pass() and curThreadNum, so an entry that passes them under the
// bounds passes them in fact. The load and CPU conditions depend on the status values alone; the host sends a batch
// under an armed one to the serial path without a scan.
constexpr int kSysScanThreads = 512;  // 256 VGPRs a lane: the four staged events stay in registers
constexpr int kSysScanItems = 4;

// Block-wide exclusive prefix sums of five values at once (one pair of barriers): v[q] becomes the sum of the
// lower threads' v[q], total[q] the block's sum.
constexpr int kSysScanVals = 5;
__device__ __forceinline__ void sys_block_excl(int64_t* v, int64_t (*wsum)[kSysScanThreads / 64], int64_t* total) {
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    int64_t inc[kSysScanVals];
#pragma unroll
    for (int q = 0; q < kSysScanVals; ++q) {
        inc[q] = wave_incl_scan(v[q], lane);
        if (lane == 63) wsum[q][w] = inc[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSysScanVals; ++q) {
        int64_t base = 0, tot = 0;
        for (int j = 0; j < kSysScanThreads / 64; ++j) {
            const int64_t x = wsum[q][j];
            if (j < w) base += x;
            tot += x;
        }
        total[q] = tot;
        v[q] = base + inc[q] - v[q];
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kSysScanThreads) k_sys_scan(SysArgs a) {
    __shared__ int64_t wsum[kSysScanVals][kSysScanThreads / 64];
    __shared__ unsigned int s_first;
    LSys& s = *a.sys;
    const int S = a.S;
    const int64_t wl = a.wl;
    const LSysConf c = s.conf;
    const int64_t T0 = s.threads;
    if (threadIdx.x == 0) s_first = 0xFFFFFFFFu;
    __syncthreads();
    const int64_t P0 = a.ev[0].ts_ms / wl;
    int64_t cE = 0, cN = 0, cX = 0, cR = 0, cU = 0;  // the prefixes at the chunk's first event
    for (uint64_t base = 0; base < a.n; base += (uint64_t)kSysScanThreads * kSysScanItems) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kSysScanItems;
        sg_local_event e[kSysScanItems];
        bool in[kSysScanItems];
        int64_t tE = 0, tN = 0, tX = 0, tR = 0, tU = 0;
#pragma unroll
        for (int j = 0; j < kSysScanItems; ++j) {
            in[j] = false;
            if (i0 + j >= a.n) continue;
            e[j] = a.ev[i0 + j];
            const uint32_t res = e[j].resource & SG_KEY_INDEX;
            in[j] = res < a.K && a.inbound[res];
            if (!in[j]) continue;
            if (e[j].kind == SG_LOCAL_ENTRY) {
                tE += e[j].count > 0 ? e[j].count : 0;
                tN += 1;
            } else {
                tX += 1;
                tR += e[j].ts_ms - e[j].create_ts;
                tU += e[j].count;
            }
        }
        int64_t pre[kSysScanVals] = {tE, tN, tX, tR, tU}, tot[kSysScanVals];
        sys_block_excl(pre, wsum, tot);
        int64_t pE = cE + pre[0], pN = cN + pre[1], pX = cX + pre[2], pR = cR + pre[3], pU = cU + pre[4];
        const int64_t totE = tot[0], totN = tot[1], totX = tot[2], totR = tot[3], totU = tot[4];
        // the prefixes at the first event of every period that starts in this thread's events
        int64_t q_of[kSysScanItems];
        {
            int64_t qp = i0 == 0 ? 0 : (i0 < a.n ? a.ev[i0 - 1].ts_ms / wl - P0 : 0);
            if (qp < 0) qp = 0;  // (an out-of-order batch)
            int64_t xE = pE, xR = pR, xU = pU;
#pragma unroll
            for (int j = 0; j < kSysScanItems; ++j) {
                q_of[j] = -1;
                if (i0 + j >= a.n) continue;
                int64_t q = e[j].ts_ms / wl - P0;
                if (q < 0 || q >= (int64_t)kMaxPeriods) {  // out of order or too long: the batch is refused anyway
                    atomicMin(&s_first, (unsigned int)(i0 + j));
                    q = q < 0 ? 0 : (int64_t)kMaxPeriods - 1;
                }
                q_of[j] = q;
                for (int64_t p = qp + 1; p <= q; ++p) {
                    a.pb[p] = xE;
                    a.pb[(size_t)kMaxPeriods + p] = xU;
                    a.pb[2 * (size_t)kMaxPeriods + p] = xR;
                }
                if (q > qp) qp = q;
                if (in[j]) {
                    if (e[j].kind == SG_LOCAL_ENTRY) xE += e[j].count > 0 ? e[j].count : 0;
                    else {
                        xR += e[j].ts_ms - e[j].create_ts;
                        xU += e[j].count;
                    }
                }
            }
        }
        __threadfence_block();
        __syncthreads();
        // every inbound entry under the bounds
#pragma unroll
        for (int j = 0; j < kSysScanItems; ++j) {
            if (i0 + j >= a.n) continue;
            if (in[j] && e[j].kind == SG_LOCAL_ENTRY && q_of[j] >= 0) {
                const int64_t t = e[j].ts_ms;
                int64_t pass = 0, succ = 0, rt = 0;
                for (int b = 0; b < S; ++b) {
                    const LBucket B = s.sec[b];
                    if (!sys_valid(B.start, t, S, (int32_t)wl)) continue;
                    pass += B.c[kLPass];
                    succ += B.c[kLSucc];
                    rt += B.c[kLRt];
                }
                const int64_t ql = q_of[j] - (S - 1);
                if (ql > 0) {
                    pass += pE - a.pb[ql];
                    succ += pU - a.pb[(size_t)kMaxPeriods + ql];
                    rt += pR - a.pb[2 * (size_t)kMaxPeriods + ql];
                } else {
                    pass += pE;
                    succ += pU;
                    rt += pR;
                }
                const int64_t thr = T0 + pN - pX;
                bool clear = !(avg_div((double)pass, a.isec) + (double)e[j].count > c.qps);
                // (int) curThreadNum.sum(): the bound must survive the narrowing
                clear = clear && thr <= INT32_MAX && thr >= INT32_MIN && !(thr > c.max_thread);
                const double avg_rt = succ == 0 ? 0.0 : (double)rt * 1.0 / (double)succ;
                clear = clear && !(avg_rt > (double)c.max_rt);
                if (!clear) atomicMin(&s_first, (unsigned int)(i0 + j));
            }
            if (in[j]) {  // the prefixes move past event j
                if (e[j].kind == SG_LOCAL_ENTRY) {
                    pE += e[j].count > 0 ? e[j].count : 0;
                    pN += 1;
                } else {
                    pX += 1;
                    pR += e[j].ts_ms - e[j].create_ts;
                    pU += e[j].count;
                }
            }
        }
        cE += totE;
        cN += totN;
        cX += totX;
        cR += totR;
        cU += totU;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s.unproven = s_first != 0xFFFFFFFFu ? 1u : 0u;
        s.first_unproven = s_first;
    }
}

// ---- ENTRY_NODE after a batch that walked the normal image ----
//
// The serial path leaves, in slot I of the window, the last window period P (P % S == I) that any inbound event of
// the batch touched (currentWindow), holding that period's sums on top of the old bucket when the old bucket is the
// same window; and curThreadNum moved by passes minus exits. All sums are integers, so their order is free:
// k_sys_apply_last finds the last touched period of each slot and the thread delta, k_sys_apply_acc sums the events of
// those periods (a held period of a slot is only ever the slot's last: lastp is final when it runs),
// k_sys_apply_fold writes the buckets and clears the scratch. An event touches its window unless it is
// an entry that ends in PriorityWaitException (thread count only) with checking off — with checking on, the check
// itself opened the window.
// Each wave takes kSysApplyRun consecutive events per lane-stride (64 * kSysApplyRun events a wave): a lane keeps the
// period it is in and what it summed for it, and gives that up (atomics) only when its period changes — the batch is
// time-ordered, so that is rare — and at the end, where the wave first combines the lanes that hold the same period.
constexpr int kSysApplyRun = 16;
constexpr uint32_t kSysApplyBlock = 256 * kSysApplyRun;  // events per block

__device__ __forceinline__ bool sys_apply_event(const SysArgs& a, uint64_t i, sg_local_event* e, int32_t* status) {
    *e = a.ev[i];
    const uint32_t res = e->resource & SG_KEY_INDEX;
    if (res >= a.K || !a.inbound[res]) return false;
    *status = e->kind == SG_LOCAL_ENTRY ? a.out[i].status : SG_LOCAL_PASS;
    return true;
}

__global__ void __launch_bounds__(256) k_sys_apply_last(SysArgs a) {
    if (*a.err) return;
    LSys& s = *a.sys;
    const bool check = s.conf.check != 0;
    const int lane = lane_id();
    const uint64_t base = (uint64_t)blockIdx.x * kSysApplyBlock + (uint64_t)(threadIdx.x >> 6) * (64 * kSysApplyRun);
    int64_t thr = 0;
    unsigned long long held = 0;  // 1 + the last period this lane saw touched (0: none)
    for (int it = 0; it < kSysApplyRun; ++it) {
        const uint64_t i = base + (uint64_t)it * 64 + (uint64_t)lane;
        if (i >= a.n) break;
        sg_local_event e;
        int32_t st;
        if (!sys_apply_event(a, i, &e, &st)) continue;
        bool touch = true;
        if (e.kind == SG_LOCAL_ENTRY) {
            if (st == SG_LOCAL_PASS || st == SG_LOCAL_PASS_WAIT) thr += 1;
            touch = st != SG_LOCAL_PASS_WAIT || check;
        } else {
            thr -= 1;
        }
        if (!touch) continue;
        const unsigned long long p1 = (unsigned long long)(e.ts_ms / a.wl) + 1ull;
        if (held && held != p1) atomicMax(s.lastp + (int)((held - 1) % (unsigned)a.S), held);
        held = p1;
    }
    uint64_t rem = __ballot(held != 0);
    while (rem) {  // one atomic per distinct period of the wave
        const int l = __builtin_ctzll(rem);
        const unsigned long long pv = (unsigned long long)bcast64((int64_t)held, l);
        if (lane == l) atomicMax(s.lastp + (int)((pv - 1) % (unsigned)a.S), pv);
        rem &= ~__ballot(held == pv);
    }
    thr = wave_sum(thr);
    if (lane == 0 && thr) atomicAdd((unsigned long long*)&s.d_threads, (unsigned long long)thr);
}

__device__ __forceinline__ void sys_apply_give(LSys& s, int S, unsigned long long p1, const int64_t* c, int64_t mn) {
    int64_t* acc = s.acc + 8 * (int)((p1 - 1) % (unsigned)S);
    for (int e = 0; e < kLEv; ++e)
        if (c[e]) atomicAdd((unsigned long long*)(acc + e), (unsigned long long)c[e]);
    if (mn != INT64_MAX) atomicMin((long long*)(acc + 7), (long long)mn);
}

__global__ void __launch_bounds__(256) k_sys_apply_acc(SysArgs a) {
    if (*a.err) return;
    LSys& s = *a.sys;
    const int lane = lane_id();
    const uint64_t base = (uint64_t)blockIdx.x * kSysApplyBlock + (uint64_t)(threadIdx.x >> 6) * (64 * kSysApplyRun);
    unsigned long long held = 0;  // 1 + the period the sums below belong to (0: none)
    int64_t c[kLEv] = {0, 0, 0, 0, 0, 0}, mn = INT64_MAX;
    for (int it = 0; it < kSysApplyRun; ++it) {
        const uint64_t i = base + (uint64_t)it * 64 + (uint64_t)lane;
        if (i >= a.n) break;
        sg_local_event e;
        int32_t st;
        if (!sys_apply_event(a, i, &e, &st)) continue;
        const unsigned long long p1 = (unsigned long long)(e.ts_ms / a.wl) + 1ull;
        if (s.lastp[(int)((p1 - 1) % (unsigned)a.S)] != p1) continue;  // a later period took the slot
        if (held != p1) {
            if (held) sys_apply_give(s, a.S, held, c, mn);
            for (int q = 0; q < kLEv; ++q) c[q] = 0;
            mn = INT64_MAX;
            held = p1;
        }
        if (e.kind == SG_LOCAL_ENTRY) {
            if (st == SG_LOCAL_PASS) c[kLPass] += e.count;
            else if (st != SG_LOCAL_PASS_WAIT) c[kLBlock] += e.count;
        } else {
            const int64_t rt = e.ts_ms - e.create_ts;
            c[kLSucc] += e.count;
            c[kLRt] += rt;
            if (rt < mn) mn = rt;
            if (e.kind == SG_LOCAL_EXIT_ERROR) c[kLExc] += e.count;
        }
    }
    uint64_t rem = __ballot(held != 0);
    while (rem) {  // the lanes that hold the same period give their sums as one
        const int l = __builtin_ctzll(rem);
        const unsigned long long pv = (unsigned long long)bcast64((int64_t)held, l);
        const bool same = held == pv;
        int64_t w[kLEv];
        for (int q = 0; q < kLEv; ++q) w[q] = wave_sum(same ? c[q] : 0);
        const int64_t wm = wave_min(same ? mn : INT64_MAX);
        if (lane == l) sys_apply_give(s, a.S, pv, w, wm);
        rem &= ~__ballot(same);
    }
}

__global__ void __launch_bounds__(64) k_sys_apply_fold(SysArgs a) {
    LSys& s = *a.sys;
    const bool ok = *a.err == 0;
    for (int I = (int)threadIdx.x; I < a.S; I += (int)blockDim.x) {
        const unsigned long long lp = s.lastp[I];
        if (ok && lp) {
            const int64_t ws = (int64_t)(lp - 1) * a.wl;
            LBucket b = s.sec[I];
            if (b.start != ws) {
                b.start = ws;
                for (int e = 0; e < kLEv; ++e) b.c[e] = 0;
                b.min_rt = kStatMaxRt;
            }
            for (int e = 0; e < kLEv; ++e) b.c[e] += s.acc[8 * I + e];
            if (s.acc[8 * I + 7] < b.min_rt) b.min_rt = s.acc[8 * I + 7];
            s.sec[I] = b;
        }
        s.lastp[I] = 0;
        for (int e = 0; e < 7; ++e) s.acc[8 * I + e] = 0;
        s.acc[8 * I + 7] = INT64_MAX;
    }
    if (threadIdx.x == 0) {
        if (ok) s.threads += s.d_threads;
        s.d_threads = 0;
    }
}

}  // namespace
