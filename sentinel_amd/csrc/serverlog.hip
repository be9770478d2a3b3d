// serverlog.hip — gfx950 kernels of the token server's stat log (ClusterServerStatLogUtil, sentinel-server.log): the
// logged decisions of a decided flow, concurrent or cluster param token batch summed per (second, family, flowId,
// value) into an exact open-addressing table in device memory that lives across batches (StatLogger / StatRollingData
// with 1-second slots), and the rolling task's fetch of the complete seconds (StatLogWriteTask).
//
// What a decision logs is a pure function of its request, its result and the rule's flowId (ClusterFlowChecker.java:91,
// 102-107; SimpleClusterFlowChecker.java:49-50, 60-61 for the RLS server), so k_slog_add_flow runs behind the decisions
// and needs nothing from the walkers. It walks the batch in sorted-record order as k_blog_add does: records are grouped
// by flowId and time-ordered inside a group, so the 64 records of a wave mostly share flowId and second. The wave
// combines equal keys first and carries the last key's counters from one chunk of its span to the next (SlogCarry): one
// slot lookup and a few 64-bit integer adds per run of a key in a wave's 2048 records, not per decision. A slot holds
// the family's counters side by side (serverlog_rules.h), so the three keys of a blocked prioritized request are one
// carried key. Integer adds only: the rows do not depend on the order of arrival. k_slog_add_conc is the same walk over
// ConcArgs::rec_sorted (the walker left each released token's count in a side array); k_slog_add_param walks the param
// batch in request order (its requests are not sorted by rule, and param|block keys carry a value and rarely form runs).
//
// Removal as in blocklog.hip: the key holds the second, so the fetch moves the complete slots out, lists the survivors
// (the open second), clears the table and puts the survivors back (k_slog_take / k_slog_put).
//
// The claim / publish protocol of slog_wave_insert is blog_insert's, kept as a second copy: the key has other words, the
// add is several counters and the lanes of a wave insert side by side; k_blog_add's registers stay exactly as they were.
#include "engine.h"

namespace sg {

namespace {

struct SlogKey {
    int64_t ts;
    int64_t flow_id;
    uint64_t value;
    uint32_t family;
};

__device__ __forceinline__ uint64_t slog_hash(const SlogKey& k) {
    uint64_t h = mix64((uint64_t)k.flow_id);
    h = mix64_final(h ^ (uint64_t)k.ts);
    h = mix64_final(h ^ k.value);
    return mix64_final(h ^ (uint64_t)k.family);
}

// Every lane of the wave calls it; a lane with `act` finds or claims its key's slot and adds its counters to it, and a
// full table counts its `events` decisions and their summed acquireCount lost. Claim and publish as blog_insert: the
// claimer takes an empty tag to kSlogBusy with a CAS, writes the key words and publishes the tag with release order, and
// key words are compared only behind a published tag read with acquire order. Unlike there, the lanes of a wave insert
// side by side (a span of the Zipf tail has a new key every few records, and one lane's dependent round trips per key
// were the whole kernel's time), so no lane may wait inside its probe for a tag another lane of its own wave is about
// to publish: a lane that meets kSlogBusy, or loses the CAS, leaves its probe where it stands and every lane comes back
// to the wave-uniform loop; the claimer has published by the time that loop turns (it has to reach the same ballot),
// and a claimer in another wave runs on its own.
__device__ void slog_wave_insert(const SlogArgs& b, bool act, const SlogKey& k, const int64_t* c, uint64_t events,
                                 int64_t acq) {
    const uint64_t h = slog_hash(k);
    const uint64_t tag = h | (1ull << 63);
    uint64_t i = h & b.mask, probes = 0;
    bool pend = act;
    while (__ballot(pend)) {
        if (pend) {
            while (probes <= b.mask) {
                SlogSlot& s = b.tab[i];
                uint64_t t = __hip_atomic_load(&s.tag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (t == 0) {
                    if (atomicCAS((unsigned long long*)&s.tag, 0ull, (unsigned long long)kSlogBusy) != 0ull)
                        break;  // someone else claimed it: read the tag again in the next turn
                    s.ts = k.ts;
                    s.flow_id = k.flow_id;
                    s.value = k.value;
                    s.family = k.family;
                    __hip_atomic_store(&s.tag, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    t = tag;
                } else if (t == kSlogBusy) {
                    break;  // its key words are being written: the next turn reads the published tag
                }
                if (t == tag && s.ts == k.ts && s.flow_id == k.flow_id && s.value == k.value && s.family == k.family) {
#pragma unroll
                    for (int x = 0; x < kSlogCtrs; ++x)
                        if (c[x]) atomicAdd((unsigned long long*)&s.c[x], (unsigned long long)c[x]);
                    pend = false;
                    break;
                }
                i = (i + 1) & b.mask;  // another key's slot
                ++probes;
            }
            if (pend && probes > b.mask) {  // neither the key nor a free slot in the whole table
                atomicAdd(&b.lost[0], (unsigned long long)events);
                atomicAdd(&b.lost[1], (unsigned long long)acq);
                pend = false;
            }
        }
    }
}

// The last key a wave combined and its counters so far, wave-uniform (BlogCarry's role).
struct SlogCarry {
    SlogKey k;
    int64_t c[kSlogCtrs];
    uint64_t events;
    int64_t acq;
    bool has;
};

__device__ __forceinline__ void slog_wave_flush(const SlogArgs& b, SlogCarry& c) {
    slog_wave_insert(b, c.has && lane_id() == 0, c.k, c.c, c.events, c.acq);
    c.has = false;
}

// What one decision adds to its key's counters: acq to the counters of m_acq, 1 to those of m_one (bit x: counter x).
struct SlogAdd {
    int64_t acq;
    uint32_t m_acq, m_one;
};

// The wave's decisions (act: this lane has one) combined key by key — the first lane of each distinct key is its
// leader and keeps the key's sums, the carry joining the key that continues it. The last key (in sorted order the one
// the next chunk may continue) becomes the carry; a carry no key continued takes that key's lane. Then every lane that
// holds a finished key inserts it, side by side. Every lane of the wave calls it.
__device__ void slog_wave_add(const SlogArgs& b, SlogCarry& c, bool act, const SlogKey& k, const SlogAdd& d) {
    const int lane = lane_id();
    uint64_t todo = __ballot(act);
    if (!todo) return;
    SlogKey mk = k;                      // this lane's finished key and its sums
    int64_t mine[kSlogCtrs] = {0, 0, 0, 0, 0, 0};
    uint64_t mev = 0;
    int64_t macq = 0;
    bool mhas = false;
    int last = 0;
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int64_t lts = __shfl((long long)k.ts, lead, 64);
        const int64_t lfid = __shfl((long long)k.flow_id, lead, 64);
        const uint64_t lval = (uint64_t)__shfl((long long)k.value, lead, 64);
        const uint32_t lfam = (uint32_t)__shfl((int)k.family, lead, 64);
        const bool same = ((todo >> lane) & 1ull) && k.ts == lts && k.flow_id == lfid && k.value == lval &&
                          k.family == lfam;
        const uint64_t m = __ballot(same);
        int64_t acq;
        int64_t add[kSlogCtrs];
        if ((m & (m - 1)) == 0) {  // the key of one lane alone (request order, param|block values): its adds as they are
            acq = __shfl((long long)d.acq, lead, 64);
            const uint32_t la = (uint32_t)__shfl((int)d.m_acq, lead, 64), lo = (uint32_t)__shfl((int)d.m_one, lead, 64);
#pragma unroll
            for (int x = 0; x < kSlogCtrs; ++x) add[x] = (((la >> x) & 1u) ? acq : 0) + (int64_t)((lo >> x) & 1u);
        } else {
            acq = wave_sum(same ? d.acq : 0);
#pragma unroll
            for (int x = 0; x < kSlogCtrs; ++x) {
                const uint64_t ma = __ballot(same && ((d.m_acq >> x) & 1u));
                const uint64_t mo = __ballot(same && ((d.m_one >> x) & 1u));
                int64_t v = (int64_t)__popcll(mo);
                if (ma == m) v += acq;  // every decision of the key adds its count here: the sum is at hand
                else if (ma) v += wave_sum(same && ((d.m_acq >> x) & 1u) ? d.acq : 0);
                add[x] = v;
            }
        }
        uint64_t events = (uint64_t)__popcll(m);
        if (c.has && c.k.ts == lts && c.k.flow_id == lfid && c.k.value == lval && c.k.family == lfam) {
#pragma unroll
            for (int x = 0; x < kSlogCtrs; ++x) add[x] += c.c[x];  // the run goes on: the carry joins this key
            events += c.events;
            acq += c.acq;
            c.has = false;
        }
        if (lane == lead) {
#pragma unroll
            for (int x = 0; x < kSlogCtrs; ++x) mine[x] = add[x];
            mev = events;
            macq = acq;
            mhas = true;
        }
        last = lead;
        todo &= ~m;
    }
    SlogCarry nc;
    nc.k.ts = __shfl((long long)k.ts, last, 64);
    nc.k.flow_id = __shfl((long long)k.flow_id, last, 64);
    nc.k.value = (uint64_t)__shfl((long long)k.value, last, 64);
    nc.k.family = (uint32_t)__shfl((int)k.family, last, 64);
#pragma unroll
    for (int x = 0; x < kSlogCtrs; ++x) nc.c[x] = __shfl((long long)mine[x], last, 64);
    nc.events = (uint64_t)__shfl((long long)mev, last, 64);
    nc.acq = __shfl((long long)macq, last, 64);
    nc.has = true;
    if (lane == last) {  // its key moved into the carry; a carry that no key continued is finished and takes the lane
        mhas = c.has;
        if (c.has) {
            mk = c.k;
#pragma unroll
            for (int x = 0; x < kSlogCtrs; ++x) mine[x] = c.c[x];
            mev = c.events;
            macq = c.acq;
        }
    }
    c = nc;
    slog_wave_insert(b, mhas, mk, mine, mev, macq);
}

// The key and the adds of request idx of the decided flow batch, if its decision is logged.
//   ClusterFlowChecker (default server): SHOULD_WAIT → waiting += 1 (:91); BLOCKED → block += acquireCount,
//   block_request += 1 (:102-103) and for a prioritized request occupied_block += 1 (:107); passes are not logged.
//   SimpleClusterFlowChecker (s.rls): OK → pass += acquireCount, pass_request += 1 (:49-50); BLOCKED → block,
//   block_request (:60-61); it knows no priority.
// TOO_MANY_REQUEST, FAIL, NO_RULE_EXISTS and BAD_REQUEST return before any log call.
// rkey: the rule index the sorted record carries, or ~0 (compact records carry none: the request's). A node shard's
// slice holds the node batch's request indices and the shard's own rule indices, so the index is bounded by the node
// batch (s.n_req) and the rule always comes from the record there.
__device__ __forceinline__ bool slog_flow_key(const BatchArgs& a, const SlogArgs& s, uint64_t idx, uint32_t rkey,
                                              SlogKey& k, SlogAdd& d) {
    if (idx >= (s.n_req ? s.n_req : a.n)) return false;
    const int32_t st = a.out[idx].status;
    const bool pass = s.rls && st == SG_STATUS_OK;
    const bool wait = !s.rls && st == SG_STATUS_SHOULD_WAIT;
    if (st != SG_STATUS_BLOCKED && !pass && !wait) return false;
    const sg_req r = a.req[idx];
    const uint32_t key = rkey != 0xFFFFFFFFu ? rkey : (r.key & SG_KEY_INDEX);
    if (key >= a.K) return false;
    k.ts = r.ts_ms - r.ts_ms % 1000;
    k.flow_id = s.fid[key];
    k.value = 0;
    k.family = kSlogFlow;
    d.acq = r.acquire;
    if (pass) {
        d.m_acq = 1u << SG_SLOG_FLOW_PASS;
        d.m_one = 1u << SG_SLOG_FLOW_PASS_REQUEST;
    } else if (wait) {
        d.m_acq = 0;
        d.m_one = 1u << SG_SLOG_FLOW_WAITING;
    } else {
        d.m_acq = 1u << SG_SLOG_FLOW_BLOCK;
        d.m_one = 1u << SG_SLOG_FLOW_BLOCK_REQUEST;
        if (!s.rls && (r.key & SG_KEY_PRIO)) d.m_one |= 1u << SG_SLOG_FLOW_OCCUPIED_BLOCK;
    }
    return true;
}

}  // namespace

constexpr uint64_t kSlogSpan = 2048;  // consecutive sorted records per wave and turn

// The request index of sorted record j, or an index >= n for a record that stands for no accepted request. 8-byte
// records (the radix path and the binned path with SG_REC4=0): rejected and limited requests sit under the sentinel key
// K with no index. 4-byte records (R4): {request index : 24 | acquire code : 8}; rejected requests have no sorted copy
// and the caller stops before their stale tail.
template <bool R4>
__device__ __forceinline__ uint64_t slog_rec_index(const BatchArgs& a, uint64_t j, uint32_t& rkey) {
    if constexpr (R4) {
        rkey = 0xFFFFFFFFu;
        return (uint64_t)(reinterpret_cast<const uint32_t*>(a.rec_sorted)[j] >> kRec4Abits);
    } else {
        const uint64_t rec = a.rec_sorted[j];
        const uint64_t key = rec >> a.kshift;
        rkey = key >= (uint64_t)a.K ? a.K : (uint32_t)key;
        if (key >= (uint64_t)a.K) return ~0ull;
        return (rec >> a.abits) & a.imask;
    }
}

template <bool R4>
__global__ void __launch_bounds__(256) k_slog_add_flow(BatchArgs a, SlogArgs s) {
    if (*a.err) return;  // a refused batch decided nothing
    uint64_t n = a.n;
    if constexpr (R4) {
        const uint64_t drop = *s.drop;
        n = drop < n ? n - drop : 0;
    }
    const uint64_t lane = (uint64_t)lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    SlogCarry c{};
    for (uint64_t span = wave * kSlogSpan; span < n; span += waves * kSlogSpan) {
        const uint64_t end = span + kSlogSpan < n ? span + kSlogSpan : n;
        for (uint64_t base = span; base < end; base += 64) {
            const uint64_t j = base + lane;
            SlogKey k{};
            SlogAdd d{};
            bool act = false;
            if (j < end) {
                uint32_t rkey;
                const uint64_t idx = slog_rec_index<R4>(a, j, rkey);
                act = slog_flow_key(a, s, idx, rkey, k, d);
            }
            slog_wave_add(s, c, act, k, d);
        }
    }
    slog_wave_flush(s, c);
}

// The key and the add of request i (rule k) of the decided concurrent token batch, if its decision is logged
// (ConcurrentClusterFlowChecker.java): an acquire's OK → concurrent|pass += acquireCount (:73), its BLOCKED →
// concurrent|block += acquireCount (:58 or :67, one of the two runs); RELEASE_OK → concurrent|release += the token's
// acquireCount under the token's flowId (:96-99: the rule the release was sorted under, k_conc_prep). ALREADY_RELEASE,
// NO_RULE_EXISTS and BAD_REQUEST return before any log call.
__device__ __forceinline__ bool slog_conc_key(const ConcArgs& c, uint64_t rec, SlogKey& k, SlogAdd& d) {
    const uint64_t rule = rec >> c.kshift;
    const uint64_t i = rec & c.imask;
    if (rule >= (uint64_t)c.K || i >= c.n) return false;
    const int32_t st = c.out[i].status;
    const sg_conc_req q = c.req[i];
    if (q.kind == SG_CONC_ACQUIRE) {
        if (st != SG_STATUS_OK && st != SG_STATUS_BLOCKED) return false;
        d.acq = q.acquire;
        d.m_acq = st == SG_STATUS_OK ? 1u << (SG_SLOG_CONC_PASS - SG_SLOG_CONC_PASS)
                                     : 1u << (SG_SLOG_CONC_BLOCK - SG_SLOG_CONC_PASS);
    } else {
        if (st != SG_STATUS_RELEASE_OK) return false;
        d.acq = c.slog_rel[i];
        d.m_acq = 1u << (SG_SLOG_CONC_RELEASE - SG_SLOG_CONC_PASS);
    }
    d.m_one = 0;
    k.ts = q.ts_ms - q.ts_ms % 1000;
    k.flow_id = c.flow_id[rule];
    k.value = 0;
    k.family = kSlogConc;
    return true;
}

__global__ void __launch_bounds__(256) k_slog_add_conc(ConcArgs c, SlogArgs s) {
    if (*c.err) return;  // a refused batch decided nothing
    const uint64_t lane = (uint64_t)lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    SlogCarry carry{};
    for (uint64_t span = wave * kSlogSpan; span < c.n; span += waves * kSlogSpan) {
        const uint64_t end = span + kSlogSpan < c.n ? span + kSlogSpan : c.n;
        for (uint64_t base = span; base < end; base += 64) {
            const uint64_t j = base + lane;
            SlogKey k{};
            SlogAdd d{};
            const bool act = j < end && slog_conc_key(c, c.rec_sorted[j], k, d);
            slog_wave_add(s, carry, act, k, d);
        }
    }
    slog_wave_flush(s, carry);
}

// The key and the add of request i of the decided cluster param batch, if its decision is logged
// (ClusterParamFlowChecker.java:58-80): OK → param|pass|id += 1 (:77; a request that reaches the checker has a value);
// BLOCKED → param|block|id|blockObject += 1 (:79), blockObject the first value in request order whose check failed
// (:61-70). For a single-value request that is its value. For a multi-value request the converged checks name it —
// chk[value_begin + j] is position j's check on the state before the request, a repeated value's later positions
// carry 1 — unless the group fallback replayed the request, which stored the position itself (slog_blk).
// TOO_MANY_REQUEST (:45-47), NO_RULE_EXISTS and BAD_REQUEST return before any log call.
__device__ __forceinline__ bool slog_param_key(const CPArgs& c, const CPBatch& b, const SlogArgs& s, uint64_t i,
                                               SlogKey& k, SlogAdd& d) {
    const sg_cparam_req q = c.req[i];
    const uint32_t rule = q.key & SG_KEY_INDEX;
    if (rule == SG_KEY_BAD || q.acquire <= 0 || q.value_count == 0 || rule >= c.n_rules) return false;
    if ((uint64_t)q.value_begin + q.value_count > c.n_values) return false;  // kErrBounds refused the batch already
    const int32_t st = c.out[i].status;
    if (st != SG_STATUS_OK && st != SG_STATUS_BLOCKED) return false;
    k.ts = q.ts_ms - q.ts_ms % 1000;
    k.flow_id = s.cpfid[rule];
    k.value = 0;
    k.family = kSlogParam;
    d.acq = q.acquire;
    d.m_acq = 0;
    d.m_one = 1u << (SG_SLOG_PARAM_PASS - SG_SLOG_PARAM_PASS);
    if (st == SG_STATUS_BLOCKED) {
        uint32_t at = b.slog_blk[i];
        if (at >= q.value_count) {
            at = 0;
            while (at + 1 < q.value_count && b.chk[(uint64_t)q.value_begin + at] != 0) ++at;
        }
        k.value = c.values[(uint64_t)q.value_begin + at];
        d.m_one = 1u << (SG_SLOG_PARAM_BLOCK - SG_SLOG_PARAM_PASS);
    }
    return true;
}

__global__ void __launch_bounds__(256) k_slog_add_param(CPArgs c, CPBatch b, SlogArgs s) {
    if (*c.err) return;  // a refused batch decided nothing
    const uint64_t lane = (uint64_t)lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    SlogCarry carry{};
    for (uint64_t span = wave * kSlogSpan; span < c.n; span += waves * kSlogSpan) {
        const uint64_t end = span + kSlogSpan < c.n ? span + kSlogSpan : c.n;
        for (uint64_t base = span; base < end; base += 64) {
            const uint64_t i = base + lane;
            SlogKey k{};
            SlogAdd d{};
            const bool act = i < end && slog_param_key(c, b, s, i, k, d);
            slog_wave_add(s, carry, act, k, d);
        }
    }
    slog_wave_flush(s, carry);
}

__global__ void __launch_bounds__(256) k_slog_take(SlogArgs b, int64_t limit, int emit, SlogSlot* rows, SlogSlot* keep,
                                                   unsigned long long* count, unsigned long long* n_keep) {
    // every lane stays to the end (the wave aggregates its counter adds: one atomic per wave and counter, not one per
    // slot on a single address)
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = lane_id();
    const bool live = i <= b.mask && (b.tab[i].tag >> 63) != 0;
    const int64_t ts = live ? b.tab[i].ts : 0;
    const bool done = live && ts + 1000 <= limit;
    if (!emit) {
        long long r = 0;
        if (done) {
            const SlogSlot s = b.tab[i];
            for (int x = 0; x < kSlogCtrs; ++x) r += slog_event(s.family, x) >= 0 && s.c[x] != 0;
        }
        r = wave_sum(r);
        if (lane == 0 && r) atomicAdd(count, (unsigned long long)r);
        return;
    }
    const bool kept = live && !done;
    const uint64_t md = __ballot(done), mk = __ballot(kept);
    unsigned long long bd = 0, bk = 0;
    if (lane == 0) {
        if (md) bd = atomicAdd(count, (unsigned long long)__popcll(md));
        if (mk) bk = atomicAdd(n_keep, (unsigned long long)__popcll(mk));
    }
    bd = (unsigned long long)__shfl((long long)bd, 0, 64);
    bk = (unsigned long long)__shfl((long long)bk, 0, 64);
    const uint64_t below = (1ull << lane) - 1ull;
    if (done) rows[bd + __popcll(md & below)] = b.tab[i];
    else if (kept) keep[bk + __popcll(mk & below)] = b.tab[i];
}

// The survivors back into the cleared table, one a lane (their keys are distinct).
__global__ void __launch_bounds__(256) k_slog_put(SlogArgs b, const SlogSlot* keep, const unsigned long long* n_keep) {
    const uint64_t n = *n_keep <= b.mask + 1 ? *n_keep : b.mask + 1;
    const uint64_t lane = (uint64_t)lane_id();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += step) {
        const uint64_t j = base + lane;
        const bool act = j < n;
        SlogSlot r{};
        if (act) r = keep[j];
        SlogKey k;
        k.ts = r.ts;
        k.flow_id = r.flow_id;
        k.value = r.value;
        k.family = r.family;
        slog_wave_insert(b, act, k, r.c, 0, 0);
    }
}

hipError_t launch_slog_add_flow(const BatchArgs& a, const SlogArgs& s, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (a.rec4 && !s.drop) return hipErrorInvalidValue;  // compact records: the rejected requests' total bounds the walk
    const uint64_t blocks = (a.n + 4 * kSlogSpan - 1) / (4 * kSlogSpan);  // four waves a block, a span each
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (a.rec4) k_slog_add_flow<true><<<grid, dim3(256), 0, stream>>>(a, s);
    else k_slog_add_flow<false><<<grid, dim3(256), 0, stream>>>(a, s);
    return hipGetLastError();
}

hipError_t launch_slog_add_conc(const ConcArgs& c, const SlogArgs& s, hipStream_t stream) {
    if (c.n == 0) return hipSuccess;
    if (!c.slog_rel) return hipErrorInvalidValue;
    const uint64_t blocks = (c.n + 4 * kSlogSpan - 1) / (4 * kSlogSpan);
    k_slog_add_conc<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream>>>(c, s);
    return hipGetLastError();
}

hipError_t launch_slog_add_param(const CPArgs& c, const CPBatch& b, const SlogArgs& s, hipStream_t stream) {
    if (c.n == 0) return hipSuccess;
    if (!b.slog_blk || !s.cpfid) return hipErrorInvalidValue;
    const uint64_t blocks = (c.n + 4 * kSlogSpan - 1) / (4 * kSlogSpan);
    k_slog_add_param<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream>>>(c, b, s);
    return hipGetLastError();
}

hipError_t launch_slog_take(const SlogArgs& s, int64_t limit, int emit, SlogSlot* rows, SlogSlot* keep,
                            unsigned long long* count, unsigned long long* n_keep, hipStream_t stream) {
    const uint64_t blocks = (s.mask + 256) / 256;
    k_slog_take<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(s, limit, emit, rows, keep, count, n_keep);
    return hipGetLastError();
}

hipError_t launch_slog_put(const SlogArgs& s, const SlogSlot* keep, const unsigned long long* n_keep,
                           hipStream_t stream) {
    const uint64_t blocks = (s.mask + 256) / 256;
    k_slog_put<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream>>>(s, keep, n_keep);
    return hipGetLastError();
}

}  // namespace sg
