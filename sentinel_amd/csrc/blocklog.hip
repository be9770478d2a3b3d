// blocklog.hip — gfx950 kernels of LogSlot's rollup (core/slots/logger/LogSlot.java:35-47): the blocked entries of a
// decided local batch summed per (second, resource, exception class, ruleLimitApp, origin) into an exact
// open-addressing table in device memory that lives across batches (StatLogger / StatRollingData), and the rolling
// task's fetch of the complete seconds' rows (StatLogWriteTask).
//
// k_blog_add walks the batch in sorted-record order: records are grouped by resource and time-ordered inside a group,
// so the 64 records of a wave mostly share resource and second, and a saturated batch has far fewer distinct keys per
// wave than entries. The wave combines equal keys first (one leader per distinct key, the counts summed by shuffles)
// and carries the last key's sums from one chunk of its span to the next (BlogCarry): one slot lookup and one 64-bit
// integer add per run of a key in a wave's 2048 records, not per entry. Integer adds only, so the rows do not depend
// on the order of arrival.
//
// Removal: the key holds the second, so every row leaves for good a second or two after it came — tombstones would
// pile up for the life of the handle and stretch every probe chain. The fetch instead moves the complete rows out,
// lists the few survivors (the open second), clears the table and puts the survivors back (k_blog_take / k_blog_put):
// a once-a-second pass over a table that fits in L2.
#include "engine.h"

namespace sg {

namespace {

struct BlogKey {
    int64_t ts;
    uint64_t app;
    uint64_t ro;
    uint64_t sk;  // status << 32 | kind
};

__device__ __forceinline__ uint64_t blog_hash(const BlogKey& k) {
    uint64_t h = mix64(k.ro);
    h = mix64_final(h ^ k.app);
    h = mix64_final(h ^ (uint64_t)k.ts);
    return mix64_final(h ^ k.sk);
}

// One lane: find or claim the key's slot and add (sum, over `events` entries) to it; a full table counts them lost.
// Claim and publish as the node pool's keys, for a key of several words: the claimer takes an empty tag to kBlogBusy
// with a CAS, writes the key words and publishes the tag with release order; a prober that meets kBlogBusy waits for
// the tag (the claimer is a lane of another wave in straight-line code: lane 0 alone inserts for its wave), and
// compares key words only behind a published tag it read with acquire order.
__device__ void blog_insert(const BlogArgs& b, const BlogKey& k, int64_t sum, uint64_t events) {
    const uint64_t h = blog_hash(k);
    const uint64_t tag = h | (1ull << 63);
    uint64_t i = h & b.mask;
    for (uint64_t probes = 0; probes <= b.mask; ++probes) {
        BlogSlot& s = b.tab[i];
        for (;;) {
            uint64_t t = __hip_atomic_load(&s.tag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (t == 0) {
                const unsigned long long old = atomicCAS((unsigned long long*)&s.tag, 0ull, (unsigned long long)kBlogBusy);
                if (old != 0) continue;  // someone else claimed it: read the tag again
                s.ts = k.ts;
                s.app = k.app;
                s.ro = k.ro;
                s.status = (uint32_t)(k.sk >> 32);
                s.kind = (uint32_t)k.sk;
                __hip_atomic_store(&s.tag, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                t = tag;
            } else if (t == kBlogBusy) {
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            if (t == tag && s.ts == k.ts && s.app == k.app && s.ro == k.ro &&
                (((uint64_t)s.status << 32) | s.kind) == k.sk) {
                atomicAdd((unsigned long long*)&s.count, (unsigned long long)sum);
                return;
            }
            break;  // another key's slot
        }
        i = (i + 1) & b.mask;
    }
    atomicAdd(&b.lost[0], (unsigned long long)events);
    atomicAdd(&b.lost[1], (unsigned long long)sum);
}

// The last key a wave combined and its sums so far, wave-uniform. A wave walks a span of consecutive sorted records
// 64 at a time, and consecutive chunks mostly continue the same key (one resource, one second), so the sum is carried
// from chunk to chunk and reaches the table once per run of a key, not once per chunk: on a Zipf batch the hottest
// resource's second is over a million consecutive records, whose per-chunk adds all met at one address.
struct BlogCarry {
    BlogKey k;
    int64_t sum;
    uint64_t events;
    bool has;
};

__device__ __forceinline__ void blog_wave_flush(const BlogArgs& b, BlogCarry& c) {
    if (c.has && lane_id() == 0) blog_insert(b, c.k, c.sum, c.events);
    c.has = false;
}

// The wave's keys (act: this lane has one) combined into the carry, the carry's key added to the table when another
// key follows it: every lane of the wave calls it.
__device__ void blog_wave_add(const BlogArgs& b, BlogCarry& c, bool act, const BlogKey& k, int64_t cnt) {
    const int lane = lane_id();
    uint64_t todo = __ballot(act);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int64_t lts = __shfl((long long)k.ts, lead, 64);
        const uint64_t lapp = (uint64_t)__shfl((long long)k.app, lead, 64);
        const uint64_t lro = (uint64_t)__shfl((long long)k.ro, lead, 64);
        const uint64_t lsk = (uint64_t)__shfl((long long)k.sk, lead, 64);
        const bool same = ((todo >> lane) & 1ull) && k.ts == lts && k.app == lapp && k.ro == lro && k.sk == lsk;
        const uint64_t m = __ballot(same);
        int64_t sum = same ? cnt : 0;  // wave_sum spelled out: the call reorders this function's instructions
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor((long long)sum, o, 64);
        const uint64_t events = (uint64_t)__popcll(m);
        if (c.has && c.k.ts == lts && c.k.app == lapp && c.k.ro == lro && c.k.sk == lsk) {
            c.sum += sum;
            c.events += events;
        } else {
            blog_wave_flush(b, c);
            c.k.ts = lts;
            c.k.app = lapp;
            c.k.ro = lro;
            c.k.sk = lsk;
            c.sum = sum;
            c.events = events;
            c.has = true;
        }
        todo &= ~m;
    }
}

// The key of sorted record j, if it is a blocked entry (LogSlot sees BlockExceptions only: no pass, no
// PriorityWaitException, no exit).
__device__ __forceinline__ bool blog_key(const LArgs& a, uint64_t j, BlogKey& k, int64_t& cnt) {
    const uint64_t rec = a.rec_sorted[j];
    if (((rec & a.amask) >> 1) & 3ull) return false;  // an exit
    const uint64_t idx = (rec >> a.abits) & a.imask;
    if (idx >= a.n) return false;
    const sg_local_result r = a.out[idx];
    const int32_t st = r.status;
    if (st != SG_LOCAL_BLOCK_FLOW && st != SG_LOCAL_BLOCK_DEGRADE && st != SG_LOCAL_BLOCK_PARAM &&
        st != SG_LOCAL_BLOCK_AUTHORITY && st != SG_LOCAL_BLOCK_SYSTEM)
        return false;
    const sg_local_event e = a.ev[idx];
    if (e.kind != SG_LOCAL_ENTRY) return false;
    // the resource from the event, not from the record key: a RELATE group and the system image put several
    // resources under one key
    const uint32_t res = e.resource & ~SG_KEY_PRIO;
    if (res >= a.K) return false;
    uint64_t app = 0;
    uint32_t kind = SG_BLOCK_APP_LIMIT_APP;
    if (st == SG_LOCAL_BLOCK_FLOW) {
        int32_t la = a.res_app ? a.res_app[res] : SG_LIMIT_APP_DEFAULT;
        if (la == kBlogMixed) la = a.blog_app[idx];
        app = (uint64_t)(uint32_t)la;
    } else if (st == SG_LOCAL_BLOCK_AUTHORITY) {
        kind = SG_BLOCK_APP_ORIGIN;
        app = (uint64_t)(uint32_t)e.origin;
    } else if (st == SG_LOCAL_BLOCK_SYSTEM) {
        kind = SG_BLOCK_APP_SYSTEM;
        app = (uint64_t)(uint32_t)r.wait_ms;
    } else if (st == SG_LOCAL_BLOCK_PARAM) {
        // args[rule.getParamIdx()] with the index applyRealParamIdx left (rewritten at most once, at or before the
        // first entry the rule checked: the value after the batch is the one every block of the batch saw)
        kind = SG_BLOCK_APP_NO_ARG;
        const int32_t pidx = a.has_ps && r.wait_ms >= 0 ? a.ps.cur_idx[r.wait_ms] : -1;
        if (a.ext && pidx >= 0 && (uint32_t)pidx < a.ext[idx].arg_count) {
            const uint64_t ai = (uint64_t)a.ext[idx].arg_begin + (uint32_t)pidx;
            if (ai < a.ps.n_args) {
                const sg_pslot_arg g = a.ps.args[ai];
                if (g.kind == SG_ARG_COLLECTION) {
                    kind = SG_BLOCK_APP_LABEL;
                    app = (uint64_t)(uint32_t)g.reserved;
                } else if (g.kind == SG_ARG_NULL) {
                    kind = SG_BLOCK_APP_NULL_ARG;
                } else {
                    // a scalar: values[value_begin], as k_local_prep and the walkers read it whatever value_count says
                    // (the bound only keeps a malformed argument's read inside the array)
                    kind = SG_BLOCK_APP_VALUE;
                    app = g.value_begin < a.ps.n_values ? a.ps.values[g.value_begin] : 0;
                }
            }
        }
    }
    k.ts = e.ts_ms - e.ts_ms % 1000;
    k.app = app;
    k.ro = ((uint64_t)res << 32) | (uint32_t)e.origin;
    k.sk = ((uint64_t)(uint32_t)st << 32) | kind;
    cnt = e.count;
    return true;
}

}  // namespace

constexpr uint64_t kBlogSpan = 2048;  // consecutive sorted records per wave and turn

__global__ void __launch_bounds__(256) k_blog_add(LArgs a, BlogArgs b) {
    if (*a.err) return;  // a refused batch decided nothing
    const uint64_t lane = (uint64_t)lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    BlogCarry c{};
    for (uint64_t span = wave * kBlogSpan; span < a.n; span += waves * kBlogSpan) {
        const uint64_t end = span + kBlogSpan < a.n ? span + kBlogSpan : a.n;
        for (uint64_t base = span; base < end; base += 64) {
            const uint64_t j = base + lane;
            BlogKey k{};
            int64_t cnt = 0;
            const bool act = j < end && blog_key(a, j, k, cnt);
            blog_wave_add(b, c, act, k, cnt);
        }
    }
    blog_wave_flush(b, c);
}

__global__ void __launch_bounds__(256) k_blog_take(BlogArgs b, int64_t limit, int emit, sg_block_row* rows,
                                                   sg_block_row* keep, unsigned long long* count,
                                                   unsigned long long* n_keep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > b.mask) return;
    const BlogSlot s = b.tab[i];
    if (!(s.tag >> 63)) return;
    const bool done = s.ts + 1000 <= limit;
    if (!emit) {
        if (done) atomicAdd(count, 1ull);
        return;
    }
    sg_block_row r;
    r.timestamp = s.ts;
    r.count = s.count;
    r.app = s.app;
    r.resource = (uint32_t)(s.ro >> 32);
    r.origin = (int32_t)(uint32_t)s.ro;
    r.status = (int32_t)s.status;
    r.app_kind = (int32_t)s.kind;
    if (done) rows[atomicAdd(count, 1ull)] = r;
    else keep[atomicAdd(n_keep, 1ull)] = r;
}

__global__ void __launch_bounds__(256) k_blog_put(BlogArgs b, const sg_block_row* keep, const unsigned long long* n_keep) {
    const uint64_t n = *n_keep;
    const uint64_t lane = (uint64_t)lane_id();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    BlogCarry c{};
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += step) {
        const uint64_t j = base + lane;
        BlogKey k{};
        int64_t cnt = 0;
        const bool act = j < n && j <= b.mask;
        if (act) {
            const sg_block_row r = keep[j];
            k.ts = r.timestamp;
            k.app = r.app;
            k.ro = ((uint64_t)r.resource << 32) | (uint32_t)r.origin;
            k.sk = ((uint64_t)(uint32_t)r.status << 32) | (uint32_t)r.app_kind;
            cnt = r.count;
        }
        blog_wave_add(b, c, act, k, cnt);
    }
    blog_wave_flush(b, c);
}

hipError_t launch_blog_add(const LArgs& L, const BlogArgs& b, hipStream_t stream) {
    if (L.n == 0) return hipSuccess;
    const uint64_t blocks = (L.n + 4 * kBlogSpan - 1) / (4 * kBlogSpan);  // four waves a block, a span each
    k_blog_add<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream>>>(L, b);
    return hipGetLastError();
}

hipError_t launch_blog_take(const BlogArgs& b, int64_t limit, int emit, sg_block_row* rows, sg_block_row* keep,
                            unsigned long long* count, unsigned long long* n_keep, hipStream_t stream) {
    const uint64_t blocks = (b.mask + 256) / 256;
    k_blog_take<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(b, limit, emit, rows, keep, count, n_keep);
    return hipGetLastError();
}

hipError_t launch_blog_put(const BlogArgs& b, const sg_block_row* keep, const unsigned long long* n_keep,
                           hipStream_t stream) {
    const uint64_t blocks = (b.mask + 256) / 256;
    k_blog_put<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream>>>(b, keep, n_keep);
    return hipGetLastError();
}

}  // namespace sg
