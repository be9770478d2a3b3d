// node.hip — the node handle's request routing (include/sentinel_gpu.h, sg_node_*): one token server's batch split
// over G shard handles by flowId owner, and the shards' results put back in the caller's order.
//
// The reference serves every flowId from one TokenService (DefaultTokenService.requestToken, DefaultTokenService.java
// :39-50, called by all Netty workers, NettyTransportServer.java:53-54). Here the flowIds are hashed over G shards
// (splitmix64(flowId) mod G); the node's front handle has already validated the batch and run the
// namespace limiter over it in caller order (k_prep + the limiter pre-pass), so each request of its packed records
// that survived carries its node rule index. Routing is a stable multisplit of those records by shard:
//   k_route_count    per 4096-record tile: requests per shard (LDS counters)
//   k_route_scan     one block per shard: the exclusive scan of its tile counts, its total; k_route_bases lays the
//                    shard slices out one after the other (shard g at base[g]) in one sub-batch buffer
//   k_route_scatter  per tile: each wave ranks its 64-record rounds by shard (match ballots, as the radix scatter)
//                    and writes the sub-request {ts, local rule index | prio, acquire} and the node position of
//                    every routed request — time order within a shard is kept (stable), so each slice is a valid
//                    batch for its shard
//   k_route_gather   out[pos[j]] = sub_out[j]: the shards' results in caller order
// Shards on the front's device take packed records instead (RouteArgs::sub_rec): 8 B read and 8 B written per routed
// request, and the shards write the caller's results in place (no gather).
// HBM-bound byte work: 16 B read + 16 B + 4 B written per request (scatter), 12 B + 4 B read and 12 B written
// (gather); no MFMA.
#include "engine.h"

namespace sg {

namespace {

constexpr int kRouteThreads = 256;
constexpr int kRouteRounds = 16;
constexpr uint32_t kRouteTile = kRouteThreads * kRouteRounds;
constexpr int kRouteWaveRecs = kRouteTile / (kRouteThreads / 64);

__device__ __forceinline__ int route_lane() { return (int)__lane_id(); }

// Lanes of the wave whose 6-bit shard equals this lane's (shard 64: not routed).
__device__ __forceinline__ uint64_t match_shard(uint32_t s) {
    uint64_t peers = ~0ull;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const uint64_t m = __ballot((s >> b) & 1u);
        peers &= ((s >> b) & 1u) ? m : ~m;
    }
    return peers;
}

__device__ __forceinline__ uint32_t shard_of_rec(const RouteArgs& r, uint64_t rec) {
    const uint32_t k = (uint32_t)(rec >> r.kshift);
    return k < r.K ? (uint32_t)r.shard_of[k] : (uint32_t)kRouteNone;
}

}  // namespace

__global__ void __launch_bounds__(kRouteThreads) k_route_count(RouteArgs r) {
    __shared__ uint32_t cnt[kMaxShards];
    const int tid = threadIdx.x;
    if (tid < kMaxShards) cnt[tid] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kRouteTile;
    // every record's load, then every owner lookup, issued before any is used (two round trips per thread)
    uint64_t rec[kRouteRounds];
    uint32_t sh[kRouteRounds];
#pragma unroll
    for (int it = 0; it < kRouteRounds; ++it) {
        const uint64_t i = base + (uint64_t)it * kRouteThreads + tid;
        rec[it] = i < r.n ? r.rec[i] : ~0ull;
    }
#pragma unroll
    for (int it = 0; it < kRouteRounds; ++it) sh[it] = shard_of_rec(r, rec[it]);
#pragma unroll
    for (int it = 0; it < kRouteRounds; ++it)
        if (sh[it] < (uint32_t)r.G) atomicAdd(&cnt[sh[it]], 1u);
    __syncthreads();
    if (tid < r.G) r.tile_cnt[(size_t)blockIdx.x * kMaxShards + tid] = cnt[tid];
}

// One block per shard: the exclusive scan of the shard's column of tile counts (1024 threads, a few tiles each,
// then a block scan), the shard's total for the host. (A serial column walk was one dependent load per tile:
// 1.4 ms for a 16M-request batch.)
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) k_route_scan(RouteArgs r, uint32_t ntiles) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const int g = blockIdx.x, tid = threadIdx.x, lane = route_lane(), wave = tid >> 6;
    const uint32_t per = (ntiles + kScanThreads - 1) / kScanThreads;
    const uint32_t t0 = (uint32_t)tid * per, t1 = min(t0 + per, ntiles);
    uint32_t mine = 0;
    for (uint32_t t = t0; t < t1; ++t) mine += r.tile_cnt[(size_t)t * kMaxShards + g];
    uint32_t x = mine;  // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, (unsigned)o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t run = x - mine, total = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
        if (w < wave) run += wsum[w];
        total += wsum[w];
    }
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t c = r.tile_cnt[(size_t)t * kMaxShards + g];
        r.tile_cnt[(size_t)t * kMaxShards + g] = run;
        run += c;
    }
    if (tid == 0) r.shard_tot[g] = total;
}

// The shard slices one after the other: base[g] = Σ totals before g (G <= 64: one wave).
__global__ void __launch_bounds__(64) k_route_bases(RouteArgs r) {
    const int lane = route_lane();
    const uint32_t v = lane < r.G ? r.shard_tot[lane] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, (unsigned)o, 64);
        if (lane >= o) x += y;
    }
    if (lane < r.G) r.shard_base[lane] = x - v;
    if (lane == 63) r.shard_base[r.G] = x;
}

__global__ void __launch_bounds__(kRouteThreads) k_route_scatter(RouteArgs r) {
    __shared__ uint32_t wrun[kRouteThreads / 64][kMaxShards];  // each wave's running count per shard in its range
    __shared__ uint32_t wtot[kRouteThreads / 64][kMaxShards];  // each wave's total per shard (its range's prefix)
    const int tid = threadIdx.x, lane = route_lane(), wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kRouteTile;
    const uint64_t w0 = base + (uint64_t)wave * kRouteWaveRecs;  // the wave's contiguous records
    for (int x = lane; x < kMaxShards; x += 64) {
        wrun[wave][x] = 0;
        wtot[wave][x] = 0;
    }
    // every record, then every owner and local index, loaded before any is used (kept for both passes: a dependent
    // load chain per round was the kernel's time beside the walkers)
    constexpr int kR = kRouteWaveRecs / 64;
    uint64_t recs[kR];
    uint32_t sh[kR], loc[kR];
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint64_t i = w0 + (uint64_t)it * 64 + lane;
        recs[it] = i < r.n ? r.rec[i] : ~0ull;
    }
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        sh[it] = shard_of_rec(r, recs[it]);
        const uint32_t k = (uint32_t)(recs[it] >> r.kshift);
        loc[it] = sh[it] < (uint32_t)r.G ? r.local_of[k] : 0u;
    }
    // 1. per wave: records per shard over its range (the tile's stable order is wave 0's records, then wave 1's …)
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint32_t s = sh[it];
        const uint64_t peers = match_shard(s);
        if (s < (uint32_t)r.G && (peers & ((1ull << lane) - 1ull)) == 0) wtot[wave][s] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_sched_barrier(0);  // round by round (hoisted ballots spilled)
    }
    __syncthreads();
    // 2. place: position = shard base + the tile's offset + earlier waves of the tile + earlier rounds + rank in round
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint64_t rec = recs[it];
        const uint32_t s = sh[it];
        const uint64_t peers = match_shard(s);
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (s < (uint32_t)r.G) {
            uint32_t before = 0;
            for (int w = 0; w < wave; ++w) before += wtot[w][s];
            const uint32_t pos = r.shard_base[s] + r.tile_cnt[(size_t)blockIdx.x * kMaxShards + s] + before +
                                 wrun[wave][s] + rank;
            if (r.sub_rec) {
                r.sub_rec[pos] = ((uint64_t)loc[it] << r.skshift[s]) | (rec & r.low_mask);
            } else {
                const uint32_t idx = (uint32_t)((rec >> r.abits) & r.imask);
                const sg_req q = r.req[idx];
                sg_req o;
                o.ts_ms = q.ts_ms;
                o.key = loc[it] | (q.key & SG_KEY_PRIO);
                o.acquire = q.acquire;
                r.sub_req[pos] = o;
                r.sub_pos[pos] = idx;
            }
        }
        if (s < (uint32_t)r.G && rank == 0) wrun[wave][s] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_sched_barrier(0);
    }
}

__global__ void __launch_bounds__(256) k_route_gather(const sg_result* sub_out, const uint32_t* sub_pos, uint64_t total,
                                                      sg_result* out) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (uint64_t)gridDim.x * blockDim.x)
        out[sub_pos[j]] = sub_out[j];
}

hipError_t launch_route(const RouteArgs& r, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)((r.n + kRouteTile - 1) / kRouteTile);
    if (tiles == 0) return hipSuccess;
    lds_poison(stream);
    hipLaunchKernelGGL(k_route_count, dim3(tiles), dim3(kRouteThreads), 0, stream, r);
    hipLaunchKernelGGL(k_route_scan, dim3((unsigned)r.G), dim3(kScanThreads), 0, stream, r, tiles);
    hipLaunchKernelGGL(k_route_bases, dim3(1), dim3(64), 0, stream, r);
    lds_poison(stream);
    hipLaunchKernelGGL(k_route_scatter, dim3(tiles), dim3(kRouteThreads), 0, stream, r);
    return hipGetLastError();
}

hipError_t launch_route_gather(const sg_result* sub_out, const uint32_t* sub_pos, uint64_t total, sg_result* out,
                               hipStream_t stream) {
    if (total == 0) return hipSuccess;
    uint64_t g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_route_gather, dim3((unsigned)g), dim3(256), 0, stream, sub_out, sub_pos, total, out);
    return hipGetLastError();
}

uint64_t route_tiles(uint64_t n) { return (n + kRouteTile - 1) / kRouteTile; }

// ---- cluster param and concurrent token batches over the node (sg_node_cparam_*, sg_node_conc_*) ----
//
// DefaultTokenService.requestParamToken / requestConcurrentToken / releaseConcurrentToken (DefaultTokenService.java
// :53-85) for the whole node: a request goes to the shard that owns its flowId (a param rule's flowId; a flow rule's
// for concurrent tokens; a release to the shard whose token it names: node token id = (shard token id - 1) * G +
// shard + 1), and every shard decides its slice in the node's order. Requests nothing owns (invalid keys, null
// tokens) go to shard 0, whose validation answers them. Routing is a stable partition by owner: a record {owner : 8 |
// request index} per request, one 8-bit radix pass, then the slices gathered (keys and token ids made shard-local;
// a param request's values copied after the slice's earlier ones, its value_begin rebased).

__global__ void __launch_bounds__(256) k_nreq_keys(NodeReqArgs q) {
    __shared__ uint32_t cnt[kMaxShards], vcnt[kMaxShards];
    const int tid = threadIdx.x;
    if (tid < kMaxShards) cnt[tid] = vcnt[tid] = 0;
    __syncthreads();
    // the loop runs block-uniformly (the shard counts below are wave-wide)
    for (uint64_t b0 = (uint64_t)blockIdx.x * 256; b0 < q.n; b0 += (uint64_t)gridDim.x * 256) {
        const uint64_t i = b0 + tid;
        const bool act = i < q.n;
        uint32_t g = 0, nv = 0;
        if (act) {
            {  // the node's time order (a batch older than the node's previous one, or unsorted, is refused whole)
                const int64_t t = q.cp ? q.cp[i].ts_ms : q.cc[i].ts_ms;
                const int64_t tp = i == 0 ? q.last_ts : (q.cp ? q.cp[i - 1].ts_ms : q.cc[i - 1].ts_ms);
                if (t < 0 || t < tp) atomicOr(q.err, kErrTime);
            }
            if (q.cp) {
                const sg_cparam_req r = q.cp[i];
                const uint32_t key = r.key & SG_KEY_INDEX;
                if (key < q.K) g = q.shard_of[key];
                // only a valid request's values are read (DefaultTokenService answers the others without them); an
                // invalid one reaches its shard with no values, and the shard answers it as one handle would
                const bool valid = key < q.K && r.acquire > 0 && r.value_count > 0;
                nv = valid ? r.value_count : 0u;
                if (nv && ((uint64_t)r.value_begin + nv > q.n_values)) {  // the whole batch is refused (SG_E_INVAL)
                    atomicOr(q.err, kErrBounds);
                    nv = 0;
                }
            } else {
                const sg_conc_req r = q.cc[i];
                if (r.kind == SG_CONC_RELEASE) g = r.token_id ? (uint32_t)((r.token_id - 1) % (uint64_t)q.G) : 0u;
                else if ((r.key & SG_KEY_INDEX) < q.K) g = q.shard_of[r.key & SG_KEY_INDEX];
            }
            q.rec[i] = ((uint64_t)g << 56) | i;
            q.nvals[i] = nv;
        }
        // per shard present in the wave: one LDS add of its request count and value count (the lanes of a wave hit
        // G addresses at most; per-lane atomics serialised on them and held back the next request's loads)
        bool todo = act;
        while (__ballot(todo)) {
            const uint32_t g0 = (uint32_t)__shfl((int)g, __builtin_ctzll(__ballot(todo)), 64);
            const bool mine = todo && g == g0;
            const uint64_t m = __ballot(mine);
            uint32_t v = mine ? nv : 0u;
            for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
            if (__lane_id() == (uint32_t)__builtin_ctzll(m)) {
                atomicAdd(&cnt[g0], (uint32_t)__popcll(m));
                if (v) atomicAdd(&vcnt[g0], v);
            }
            todo = todo && !mine;
        }
    }
    __syncthreads();
    if (tid < q.G) {
        if (cnt[tid]) atomicAdd(&q.cnt[tid], cnt[tid]);
        if (vcnt[tid]) atomicAdd(&q.vcnt[tid], vcnt[tid]);
    }
}

// Exclusive scan of the sorted requests' value counts (param batches): per 4096-request tile sums, one block over the
// tile sums, then each tile's requests (nvals in node order, read through the sorted records).
constexpr uint32_t kNvTile = 4096;
__global__ void __launch_bounds__(256) k_nreq_vsum(NodeReqArgs q, const uint64_t* sorted) {
    __shared__ uint32_t ws[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * kNvTile;
    uint32_t s = 0;
    for (uint64_t j = t0 + threadIdx.x; j < min(q.n, t0 + kNvTile); j += 256)
        s += q.nvals[sorted[j] & 0xFFFFFFFFFFFFFFull];
    for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) q.tsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ void __launch_bounds__(1024) k_nreq_vscan(NodeReqArgs q, uint32_t tiles) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < tiles; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < tiles ? q.tsum[i] : 0u;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const uint32_t x = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0u;
            __syncthreads();
            part[threadIdx.x] += x;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (i < tiles) q.tsum[i] = c + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + part[1023];
        __syncthreads();
    }
}

// The slices: sub_req[j] = the request of sorted record j with its key (and token id) made shard-local, its value
// range copied and rebased (param), sub_pos[j] its node position. One block per 4096 sorted records; the value
// offsets inside the tile by a block scan.
__global__ void __launch_bounds__(256) k_nreq_gather(NodeReqArgs q, const uint64_t* sorted) {
    __shared__ uint32_t ws[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * kNvTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t run = q.cp ? q.tsum[blockIdx.x] : 0u;
    for (uint64_t b0 = t0; b0 < min(q.n, t0 + kNvTile); b0 += 256) {
        const uint64_t j = b0 + threadIdx.x;
        const bool act = j < q.n;
        const uint64_t rec = act ? sorted[j] : 0ull;
        const uint32_t g = (uint32_t)(rec >> 56);
        const uint64_t i = rec & 0xFFFFFFFFFFFFFFull;
        uint32_t nv = (act && q.cp) ? q.nvals[i] : 0u;
        // block-exclusive scan of nv
        uint32_t x = nv;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, (unsigned)o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) ws[wave] = x;
        __syncthreads();
        uint32_t off = run + x - nv;
        uint32_t tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += ws[w];
            tot += ws[w];
        }
        __syncthreads();
        run += tot;
        if (!act) continue;
        q.sub_pos[j] = (uint32_t)i;
        if (q.cp) {
            sg_cparam_req r = q.cp[i];
            if ((r.key & SG_KEY_INDEX) < q.K) r.key = q.local_of[r.key & SG_KEY_INDEX] | (r.key & ~SG_KEY_INDEX);
            for (uint32_t v = 0; v < nv; ++v) q.sub_vals[off + v] = q.values[r.value_begin + v];
            r.value_begin = nv ? off - q.vbase[g] : 0u;
            q.sub_cp[j] = r;
        } else {
            sg_conc_req r = q.cc[i];
            if (r.kind == SG_CONC_RELEASE) {
                if (r.token_id) r.token_id = (r.token_id - 1) / (uint64_t)q.G + 1;
            } else if ((r.key & SG_KEY_INDEX) < q.K) {
                r.key = q.local_of[r.key & SG_KEY_INDEX] | (r.key & ~SG_KEY_INDEX);
            }
            q.sub_cc[j] = r;
        }
    }
}

// Concurrent results back in node order, shard g's slice [base, base + cnt): an acquire's token id in node terms.
__global__ void __launch_bounds__(256) k_nconc_scatter(const sg_conc_result* sub_out, const uint32_t* sub_pos,
                                                       const sg_conc_req* sub_req, uint64_t base, uint64_t cnt,
                                                       uint32_t g, uint32_t G, sg_conc_result* out) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < cnt; j += (uint64_t)gridDim.x * 256) {
        sg_conc_result r = sub_out[base + j];
        if (sub_req[base + j].kind != SG_CONC_RELEASE && r.token_id) r.token_id = (r.token_id - 1) * G + g + 1;
        out[sub_pos[base + j]] = r;
    }
}

// The node snapshot from shard g's part (its local rule order): out[2 node_key[j] + c] = part[2 j + c].
__global__ void __launch_bounds__(256) k_nsnap_scatter(const double* part, const uint32_t* node_key, uint64_t cnt,
                                                       double* out) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < cnt; j += (uint64_t)gridDim.x * 256) {
        const uint32_t k = node_key[j];
        out[2 * (uint64_t)k] = part[2 * j];
        out[2 * (uint64_t)k + 1] = part[2 * j + 1];
    }
}

hipError_t launch_nsnap_scatter(const double* part, const uint32_t* node_key, uint64_t cnt, double* out,
                                hipStream_t stream) {
    if (cnt == 0) return hipSuccess;
    uint64_t b = (cnt + 255) / 256;
    if (b > 8192) b = 8192;
    hipLaunchKernelGGL(k_nsnap_scatter, dim3((unsigned)b), dim3(256), 0, stream, part, node_key, cnt, out);
    return hipGetLastError();
}

// The contract on a param batch's value ranges (sg_cparam_decide_batch): the valid requests' ranges follow request
// order and do not overlap — each begins at or after the largest end of the earlier valid requests. One handle
// checks it slot by slot on its sorted records (k_cp_order); the node copies each request's values into its slice,
// so it checks the node batch as a whole: per 4096-request tile the largest end, one block's exclusive prefix max
// over the tiles, then each tile against that carry (16 consecutive requests per thread, a block-wide prefix max).
__device__ __forceinline__ bool nreq_valid(const NodeReqArgs& q, const sg_cparam_req& r) {
    return (r.key & SG_KEY_INDEX) < q.K && r.acquire > 0 && r.value_count > 0;
}

__global__ void __launch_bounds__(256) k_nreq_vmax(NodeReqArgs q) {
    __shared__ uint32_t wm[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * kNvTile;
    uint32_t m = 0;
    for (uint64_t i = t0 + threadIdx.x; i < min(q.n, t0 + kNvTile); i += 256) {
        const sg_cparam_req r = q.cp[i];
        if (nreq_valid(q, r)) m = max(m, r.value_begin + r.value_count);
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) q.tsum[blockIdx.x] = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
}

__global__ void __launch_bounds__(1024) k_nreq_vmax_scan(NodeReqArgs q, uint32_t tiles) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < tiles; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < tiles ? q.tsum[i] : 0u;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const uint32_t x = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0u;
            __syncthreads();
            part[threadIdx.x] = max(part[threadIdx.x], x);
            __syncthreads();
        }
        const uint32_t c = carry;
        const uint32_t excl = threadIdx.x ? part[threadIdx.x - 1] : 0u;
        if (i < tiles) q.tsum[i] = max(c, excl);
        __syncthreads();
        if (threadIdx.x == 1023) carry = max(c, part[1023]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_nreq_vorder(NodeReqArgs q) {
    __shared__ uint32_t tm[256];
    constexpr int kPer = (int)(kNvTile / 256);
    const uint64_t i0 = (uint64_t)blockIdx.x * kNvTile + (uint64_t)threadIdx.x * kPer;
    uint32_t m = 0;
    for (int u = 0; u < kPer && i0 + u < q.n; ++u) {
        const sg_cparam_req r = q.cp[i0 + u];
        if (nreq_valid(q, r)) m = max(m, r.value_begin + r.value_count);
    }
    tm[threadIdx.x] = m;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive prefix max of the threads' maxima
        const uint32_t x = threadIdx.x >= (unsigned)o ? tm[threadIdx.x - o] : 0u;
        __syncthreads();
        tm[threadIdx.x] = max(tm[threadIdx.x], x);
        __syncthreads();
    }
    uint32_t carry = max(q.tsum[blockIdx.x], threadIdx.x ? tm[threadIdx.x - 1] : 0u);
    bool bad = false;
    for (int u = 0; u < kPer && i0 + u < q.n; ++u) {
        const sg_cparam_req r = q.cp[i0 + u];
        if (!nreq_valid(q, r)) continue;
        bad |= r.value_begin < carry;
        carry = max(carry, r.value_begin + r.value_count);
    }
    if (bad) atomicOr(q.err, kErrBounds);
}

hipError_t launch_nreq_keys(const NodeReqArgs& q, hipStream_t stream) {
    if (q.n == 0) return hipSuccess;
    uint64_t g = (q.n + 255) / 256;
    if (g > 4096) g = 4096;
    lds_poison(stream);
    hipLaunchKernelGGL(k_nreq_keys, dim3((unsigned)g), dim3(256), 0, stream, q);
    if (q.cp) {  // the value ranges' order (the tile maxima use tsum before the gather's value scan does)
        const uint32_t tiles = (uint32_t)((q.n + kNvTile - 1) / kNvTile);
        hipLaunchKernelGGL(k_nreq_vmax, dim3(tiles), dim3(256), 0, stream, q);
        hipLaunchKernelGGL(k_nreq_vmax_scan, dim3(1), dim3(1024), 0, stream, q, tiles);
        hipLaunchKernelGGL(k_nreq_vorder, dim3(tiles), dim3(256), 0, stream, q);
    }
    return hipGetLastError();
}

hipError_t launch_nreq_gather(const NodeReqArgs& q, const uint64_t* sorted, hipStream_t stream) {
    if (q.n == 0) return hipSuccess;
    const uint32_t tiles = (uint32_t)((q.n + kNvTile - 1) / kNvTile);
    if (q.cp) {
        hipLaunchKernelGGL(k_nreq_vsum, dim3(tiles), dim3(256), 0, stream, q, sorted);
        hipLaunchKernelGGL(k_nreq_vscan, dim3(1), dim3(1024), 0, stream, q, tiles);
    }
    hipLaunchKernelGGL(k_nreq_gather, dim3(tiles), dim3(256), 0, stream, q, sorted);
    return hipGetLastError();
}

uint64_t nreq_tiles(uint64_t n) { return (n + kNvTile - 1) / kNvTile; }

hipError_t launch_nconc_scatter(const sg_conc_result* sub_out, const uint32_t* sub_pos, const sg_conc_req* sub_req,
                                uint64_t base, uint64_t cnt, uint32_t g, uint32_t G, sg_conc_result* out,
                                hipStream_t stream) {
    if (cnt == 0) return hipSuccess;
    uint64_t b = (cnt + 255) / 256;
    if (b > 8192) b = 8192;
    hipLaunchKernelGGL(k_nconc_scatter, dim3((unsigned)b), dim3(256), 0, stream, sub_out, sub_pos, sub_req, base, cnt, g,
                       G, out);
    return hipGetLastError();
}

// ---- the local slot chain over the node (sg_node_local_*) ----
//
// StatisticSlot → FlowSlot → DegradeSlot for the whole node: every shard holds the node's rules under the node's
// resource indices and decides the events of the resources it owns (sg_local_owners: key groups on one owner), so
// routing is a stable multisplit of the 32-byte events by owner[resource], the events unchanged:
//   k_lroute_count    per 4096-event tile: events per shard, and the whole batch's validation — a slice of an
//                     unsorted batch can itself be sorted and spans less time than the batch, so the shards cannot
//                     see what one handle refuses from the events alone (time order, origin ids, the period span)
//   k_route_scan / k_route_bases   as for the token batches
//   k_lroute_scatter  per tile: each wave ranks its 64-event rounds by shard (match ballots) and moves the event and
//                     its caller position; arrival order within a slice is kept (an exit may share its entry's ms)
//   k_route_gather8   out[pos[j]] = sub_out[j] for the 8-byte results
// HBM-bound byte work: 32 B read (count), 32 B read + 32 B + 4 B written (scatter), 8 B + 4 B read and 8 B written
// (gather) per event; no MFMA.
// The whole slot chain (sg_node_slot_decide_batch) adds each event's 16-byte sg_slot_ext: 16 B more read by the count
// pass, which validates the contexts and — with param rules on the node — the argument ranges (16 B per arg record
// read), and 16 B more read and written by the scatter, the record at its event's slice position.

namespace {
__device__ __forceinline__ uint32_t lroute_shard(const LRouteArgs& r, uint32_t resource) {
    const uint32_t k = resource & SG_KEY_INDEX;
    return k < r.K ? (uint32_t)r.owner[k] : 0u;
}
}  // namespace

// kExt: the batch carries sg_slot_ext records (sg_node_slot_decide_batch); without them the kernels are the ones
// sg_node_local_decide_batch always ran.
template <bool kExt>
__global__ void __launch_bounds__(kRouteThreads) k_lroute_count(LRouteArgs r) {
    __shared__ uint32_t cnt[kMaxShards];
    const int tid = threadIdx.x;
    if (tid < kMaxShards) cnt[tid] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kRouteTile;
    const int64_t t0 = r.ev[0].ts_ms;
    // the period span k_local_prep refuses: some window's period index reaches kMaxPeriods past the first event's
    // (only an event at least that many of the shortest windows after it can; the divisions are for those alone)
    int64_t span = INT64_MAX;
    for (int w = 0; w < r.n_wl; ++w) {
        const int64_t s = (int64_t)(kMaxPeriods - 1) * r.wl[w];
        span = s < span ? s : span;
    }
    int bad = 0;
#pragma unroll 4
    for (int it = 0; it < kRouteRounds; ++it) {
        const uint64_t i = base + (uint64_t)it * kRouteThreads + tid;
        if (i >= r.n) break;
        const int64_t t = r.ev[i].ts_ms;
        const int64_t tp = i ? r.ev[i - 1].ts_ms : r.last_ts;  // the predecessor: the node's previous batch for the first
        const uint32_t res = r.ev[i].resource;
        const int32_t origin = r.ev[i].origin;
        if (t < 0 || t < tp) bad |= kErrTime;
        if (origin < 0 || origin > r.n_origins) bad |= kErrBounds;
        if (t >= t0 && t - t0 >= span)
            for (int w = 0; w < r.n_wl; ++w)
                if (t / r.wl[w] - t0 / r.wl[w] >= (int64_t)kMaxPeriods) bad |= kErrPeriods;
        if (kExt) {  // what k_local_prep refuses from the event's context and argument records
            const sg_slot_ext x = r.ext[i];
            if ((int64_t)x.context >= (int64_t)(r.n_contexts > 0 ? r.n_contexts : 1)) bad |= kErrExt;
            if (r.has_ps && !x.args_null && (res & SG_KEY_INDEX) < r.K) {
                bool ok = (uint64_t)x.arg_begin + x.arg_count <= r.n_args;
                for (uint32_t k = 0; ok && k < x.arg_count; ++k) {
                    const sg_pslot_arg g = r.args[x.arg_begin + k];
                    const uint64_t m = g.kind == SG_ARG_COLLECTION ? g.value_count : (g.kind == SG_ARG_VALUE ? 1 : 0);
                    ok = (uint64_t)g.value_begin + m <= r.n_values;
                }
                if (!ok) bad |= kErrExt;
            }
        }
        atomicAdd(&cnt[lroute_shard(r, res)], 1u);
    }
    if (bad) atomicOr(r.err, bad);
    __syncthreads();
    if (tid < r.G) r.tile_cnt[(size_t)blockIdx.x * kMaxShards + tid] = cnt[tid];
}

template <bool kExt>
__global__ void __launch_bounds__(kRouteThreads) k_lroute_scatter(LRouteArgs r) {
    __shared__ uint32_t wrun[kRouteThreads / 64][kMaxShards];  // each wave's running count per shard in its range
    __shared__ uint32_t wtot[kRouteThreads / 64][kMaxShards];  // each wave's total per shard (its range's prefix)
    const int tid = threadIdx.x, lane = route_lane(), wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kRouteTile;
    const uint64_t w0 = base + (uint64_t)wave * kRouteWaveRecs;  // the wave's contiguous events
    for (int x = lane; x < kMaxShards; x += 64) {
        wrun[wave][x] = 0;
        wtot[wave][x] = 0;
    }
    // every resource word, then every owner, loaded before any is used; the events themselves are read again when
    // they move (16 of them would not fit the registers; the tile's 128 KB are in the cache by then)
    constexpr int kR = kRouteWaveRecs / 64;
    uint32_t res[kR], sh[kR];
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint64_t i = w0 + (uint64_t)it * 64 + lane;
        res[it] = i < r.n ? r.ev[i].resource : 0u;
    }
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint64_t i = w0 + (uint64_t)it * 64 + lane;
        sh[it] = i < r.n ? lroute_shard(r, res[it]) : (uint32_t)kRouteNone;
    }
    // 1. per wave: events per shard over its range (the tile's stable order is wave 0's events, then wave 1's …)
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint32_t s = sh[it];
        const uint64_t peers = match_shard(s);
        if (s < (uint32_t)r.G && (peers & ((1ull << lane) - 1ull)) == 0) wtot[wave][s] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_sched_barrier(0);  // round by round, as k_route_scatter
    }
    __syncthreads();
    // 2. place: position = shard base + the tile's offset + earlier waves of the tile + earlier rounds + rank in round
#pragma unroll
    for (int it = 0; it < kR; ++it) {
        const uint64_t i = w0 + (uint64_t)it * 64 + lane;
        const uint32_t s = sh[it];
        const uint64_t peers = match_shard(s);
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (s < (uint32_t)r.G) {
            uint32_t before = 0;
            for (int w = 0; w < wave; ++w) before += wtot[w][s];
            const uint32_t pos = r.shard_base[s] + r.tile_cnt[(size_t)blockIdx.x * kMaxShards + s] + before +
                                 wrun[wave][s] + rank;
            r.sub_ev[pos] = r.ev[i];
            if (kExt) r.sub_ext[pos] = r.ext[i];  // 16 B more read and written: the record keeps its event's position
            r.sub_pos[pos] = (uint32_t)i;
        }
        if (s < (uint32_t)r.G && rank == 0) wrun[wave][s] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_sched_barrier(0);
    }
}

__global__ void __launch_bounds__(256) k_route_gather8(const sg_local_result* sub_out, const uint32_t* sub_pos,
                                                       uint64_t total, sg_local_result* out) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (uint64_t)gridDim.x * blockDim.x)
        out[sub_pos[j]] = sub_out[j];
}

hipError_t launch_lroute(const LRouteArgs& r, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)((r.n + kRouteTile - 1) / kRouteTile);
    if (tiles == 0) return hipSuccess;
    RouteArgs s{};  // the scan and the bases read the counts alone
    s.G = r.G;
    s.tile_cnt = r.tile_cnt;
    s.shard_base = r.shard_base;
    s.shard_tot = r.shard_tot;
    lds_poison(stream);
    if (r.ext) hipLaunchKernelGGL(k_lroute_count<true>, dim3(tiles), dim3(kRouteThreads), 0, stream, r);
    else hipLaunchKernelGGL(k_lroute_count<false>, dim3(tiles), dim3(kRouteThreads), 0, stream, r);
    hipLaunchKernelGGL(k_route_scan, dim3((unsigned)r.G), dim3(kScanThreads), 0, stream, s, tiles);
    hipLaunchKernelGGL(k_route_bases, dim3(1), dim3(64), 0, stream, s);
    lds_poison(stream);
    if (r.ext) hipLaunchKernelGGL(k_lroute_scatter<true>, dim3(tiles), dim3(kRouteThreads), 0, stream, r);
    else hipLaunchKernelGGL(k_lroute_scatter<false>, dim3(tiles), dim3(kRouteThreads), 0, stream, r);
    return hipGetLastError();
}

// ---- a slice's arguments compacted (sg_node_slot_decide_batch; a shard off devices[0], or SG_NODE_COMPACT_ARGS) ----
//
// A shard on devices[0] reads the caller's arg and value arrays in place. Another shard gets its slice's own arrays,
// built here on devices[0] in the style of k_nreq_vsum / k_nreq_vscan / k_nreq_gather: every event of the slice with
// args_null == 0 and resource < K (the ones whose ranges the count pass validated and a shard reads) brings its
// arg_count records and each record's values (1 for a VALUE, value_count for a COLLECTION, none for a null argument).
//   k_lcmp_sum     per 4096-event tile: its arg records and values (64-bit: a slice's totals may pass 2^32, which the
//                  host refuses before any shard runs)
//   k_lcmp_scan    one block: the exclusive scans of both tile sums, the slice's totals
//   k_lcmp_gather  per tile: a block scan of the events' counts per 256-event round gives each event its first arg
//                  record and first value; it copies the records (value_begin rebased, value_count and kind as
//                  given) and the values, and rebases its ext.arg_begin
// Positions are exclusive scans over slice order: a pure function of the batch. A range several events share is
// copied once per event. Per event taken: 32 B + 16 B read per pass (event, ext), 16 B per arg record and 8 B per value
// read twice (sum, gather) and written once, 16 B of ext written; no MFMA. One thread walks its event's records: the
// copies of a round are as long as its longest argument list.

namespace {

constexpr uint32_t kCmpTile = 4096;

// The event's ext record; whether its arguments go to the shard.
__device__ __forceinline__ bool lcmp_takes(const LCompactArgs& c, uint64_t j, sg_slot_ext& x) {
    x = c.ext[j];
    return !x.args_null && (c.ev[j].resource & SG_KEY_INDEX) < c.K;
}

__device__ __forceinline__ uint32_t lcmp_arg_values(const sg_pslot_arg& g) {
    return g.kind == SG_ARG_COLLECTION ? g.value_count : (g.kind == SG_ARG_VALUE ? 1u : 0u);
}

// Exclusive scan of (a, v) over the 256 threads of the block (ws: [2][4] wave totals); tot: the block's sums.
__device__ __forceinline__ void lcmp_block_scan(unsigned long long& a, unsigned long long& v, unsigned long long* ws,
                                                unsigned long long& tot_a, unsigned long long& tot_v) {
    const int lane = route_lane(), wave = threadIdx.x >> 6;
    unsigned long long xa = a, xv = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long ya = (unsigned long long)__shfl_up((long long)xa, (unsigned)o, 64);
        const unsigned long long yv = (unsigned long long)__shfl_up((long long)xv, (unsigned)o, 64);
        if (lane >= o) {
            xa += ya;
            xv += yv;
        }
    }
    if (lane == 63) {
        ws[wave] = xa;
        ws[4 + wave] = xv;
    }
    __syncthreads();
    unsigned long long oa = xa - a, ov = xv - v;
    tot_a = tot_v = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) {
            oa += ws[w];
            ov += ws[4 + w];
        }
        tot_a += ws[w];
        tot_v += ws[4 + w];
    }
    __syncthreads();  // ws is written again by the next round
    a = oa;
    v = ov;
}

}  // namespace

__global__ void __launch_bounds__(256) k_lcmp_sum(LCompactArgs c, uint32_t tiles) {
    __shared__ unsigned long long ws[8];
    const uint64_t t0 = (uint64_t)blockIdx.x * kCmpTile;
    const uint64_t t1 = t0 + kCmpTile < c.n ? t0 + kCmpTile : c.n;
    unsigned long long a = 0, v = 0;
    for (uint64_t j = t0 + threadIdx.x; j < t1; j += 256) {
        sg_slot_ext x;
        if (!lcmp_takes(c, j, x)) continue;
        a += x.arg_count;
        for (uint32_t k = 0; k < x.arg_count; ++k) v += lcmp_arg_values(c.args[x.arg_begin + k]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += (unsigned long long)__shfl_xor((long long)a, o, 64);
        v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        ws[threadIdx.x >> 6] = a;
        ws[4 + (threadIdx.x >> 6)] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        c.tsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
        c.tsum[(size_t)tiles + blockIdx.x] = ws[4] + ws[5] + ws[6] + ws[7];
    }
}

// One block, thread 0 .. 1: the serial exclusive scan of one of the two tile-sum rows (a slice of max_batch = 2^20
// events has 256 tiles; the scan is not worth a block's tree).
__global__ void __launch_bounds__(64) k_lcmp_scan(LCompactArgs c, uint32_t tiles) {
    if (threadIdx.x >= 2) return;
    unsigned long long* row = c.tsum + (size_t)threadIdx.x * tiles;
    unsigned long long run = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        const unsigned long long x = row[t];
        row[t] = run;
        run += x;
    }
    c.tot[threadIdx.x] = run;
}

__global__ void __launch_bounds__(256) k_lcmp_gather(LCompactArgs c, uint32_t tiles) {
    __shared__ unsigned long long ws[8];
    const uint64_t t0 = (uint64_t)blockIdx.x * kCmpTile;
    const uint64_t t1 = t0 + kCmpTile < c.n ? t0 + kCmpTile : c.n;
    unsigned long long run_a = c.tsum[blockIdx.x], run_v = c.tsum[(size_t)tiles + blockIdx.x];
    // the loop runs block-uniformly (the scan is block-wide)
    for (uint64_t b0 = t0; b0 < t1; b0 += 256) {
        const uint64_t j = b0 + threadIdx.x;
        sg_slot_ext x{};
        const bool take = j < t1 && lcmp_takes(c, j, x);
        unsigned long long a = 0, v = 0;
        if (take) {
            a = x.arg_count;
            for (uint32_t k = 0; k < x.arg_count; ++k) v += lcmp_arg_values(c.args[x.arg_begin + k]);
        }
        unsigned long long tot_a, tot_v;
        lcmp_block_scan(a, v, ws, tot_a, tot_v);  // a, v: the event's offsets inside the round
        a += run_a;
        v += run_v;
        run_a += tot_a;
        run_v += tot_v;
        if (!take) continue;
        // the host refused a slice whose totals reach 2^32, so the positions fit the 32-bit fields
        for (uint32_t k = 0; k < x.arg_count; ++k) {
            sg_pslot_arg g = c.args[x.arg_begin + k];
            const uint32_t m = lcmp_arg_values(g);
            for (uint32_t u = 0; u < m; ++u) c.out_vals[v + u] = c.values[(uint64_t)g.value_begin + u];
            g.value_begin = (uint32_t)v;
            c.out_args[a + k] = g;
            v += m;
        }
        x.arg_begin = (uint32_t)a;
        c.ext[j] = x;
    }
}

uint64_t lcompact_tiles(uint64_t n) { return (n + kCmpTile - 1) / kCmpTile; }

hipError_t launch_lcompact_count(const LCompactArgs& c, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)lcompact_tiles(c.n);
    if (tiles == 0) return hipSuccess;
    lds_poison(stream);
    hipLaunchKernelGGL(k_lcmp_sum, dim3(tiles), dim3(256), 0, stream, c, tiles);
    hipLaunchKernelGGL(k_lcmp_scan, dim3(1), dim3(64), 0, stream, c, tiles);
    return hipGetLastError();
}

hipError_t launch_lcompact_gather(const LCompactArgs& c, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)lcompact_tiles(c.n);
    if (tiles == 0) return hipSuccess;
    lds_poison(stream);
    hipLaunchKernelGGL(k_lcmp_gather, dim3(tiles), dim3(256), 0, stream, c, tiles);
    return hipGetLastError();
}

hipError_t launch_route_gather8(const sg_local_result* sub_out, const uint32_t* sub_pos, uint64_t total,
                                sg_local_result* out, hipStream_t stream) {
    if (total == 0) return hipSuccess;
    uint64_t g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_route_gather8, dim3((unsigned)g), dim3(256), 0, stream, sub_out, sub_pos, total, out);
    return hipGetLastError();
}

// ---- the node's metric rows merged (sg_node_local_merge_rows; cluster.merge_metric_rows on the device, no sort) ----
//
// MetricTimerListener.run for the node: the shards' raw rows of one fetch at now — timestamps multiples of 1000 in
// the minute before now, so the slot (ts / 1000) % 60 names a row's second (at most 59 of them), and a resource's row
// of a second comes from its owner alone.
//   k_merge_mark   per row: a resource row sets bit `resource` of bits[slot][W] (one 64-bit atomic OR per (slot,
//                  word) present in the wave, nothing returned; the resource rows are counted, and fewer bits than
//                  rows in the end is a duplicated row); an ENTRY_NODE row adds its five
//                  counters to the slot's sums (a few rows per shard: global adds). The slot's timestamp is claimed by
//                  the first row (compare-and-swap); another timestamp in it, one that is no multiple of 1000, or a
//                  resource that is neither below K nor the ENTRY_NODE's breaks the contract.
//   k_merge_scan   one block per slot a row named: the exclusive popcount scan of its words, 512 words a pass
//   k_merge_bases  one wave: the slots' bases in ascending timestamp order (the minute ring wraps), each second's
//                  ENTRY_NODE row — rt = Σrt / Σsuccess, kept when isValidMetricNode — after its resource rows (the
//                  largest resource id), the row count; any contract error or a table larger than the caller's
//                  buffer: nothing is written
//   k_merge_place  per row: a resource row to base[slot] + pre[slot][word] + popc(word & lower bits), rt = rt /
//                  success when success != 0
// The table is exact and its order deterministic. 64 B read twice and 64 B written per row, 8 B + 4 B of bitmap and
// prefix per row from the cache.

constexpr int kMergeScanThreads = 256;
constexpr int kMergeScanPer = 2;
constexpr uint32_t kMergeScanPass = kMergeScanThreads * kMergeScanPer;
static_assert(sizeof(sg_metric_node) == 64 && offsetof(sg_metric_node, rt) == 40 && offsetof(sg_metric_node, resource) == 56,
              "k_merge_place moves a row as eight 64-bit words");

__global__ void __launch_bounds__(64) k_merge_reset(MergeSlots* st) {
    const int j = threadIdx.x;
    if (j < kMinuteS) {
        st->ts[j] = kMergeNoTs;
        for (int c = 0; c < 5; ++c) st->acc[j][c] = 0;
        st->base[j] = 0;
        st->res_cnt[j] = 0;
        st->has_entry[j] = 0;
    }
    if (j == 0) {
        st->n_out = 0;
        st->n_res = 0;
        st->err = 0;
    }
}

__global__ void __launch_bounds__(256) k_merge_mark(MergeArgs m) {
    const int lane = route_lane();
    int bad = 0;
    uint32_t n_res = 0;  // this thread's resource rows
    // the loop runs block-uniformly (the bitmap writes below are wave-wide)
    for (uint64_t b0 = (uint64_t)blockIdx.x * 256; b0 < m.n; b0 += (uint64_t)gridDim.x * 256) {
        const uint64_t i = b0 + threadIdx.x;
        bool todo = false;
        uint64_t key = 0;
        unsigned long long bit = 0;
        // the row's timestamp and resource; `claim`: the row passed the checks that need no other row
        int64_t ts = 0;
        uint32_t res = 0;
        int slot = 0;
        bool claim = false;
        if (i < m.n) {
            ts = m.rows[i].timestamp;
            res = m.rows[i].resource;
            if (ts < 0 || ts % 1000 != 0 || (res >= m.K && res != SG_ENTRY_NODE_RESOURCE)) {
                bad = 1;
            } else {
                slot = (int)((ts / 1000) % kMinuteS);
                claim = true;
            }
        }
        // the slot's timestamp, claimed by its first row (compare-and-swap): one lane per timestamp present in the
        // wave asks (every lane asking was a pile-up of compare-and-swaps on a slot's word while the first waves all
        // found it unclaimed: 0.8 ms of a 2M-row pass)
        bool same = false;
        for (bool ask = claim; __ballot(ask);) {
            const int first = __builtin_ctzll(__ballot(ask));
            const int64_t t0 = (int64_t)__shfl((long long)ts, first, 64);
            const bool mine = ask && ts == t0;
            unsigned long long seen = 0;
            if (lane == first) {
                seen = __hip_atomic_load(&m.st->ts[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (seen == kMergeNoTs) {
                    seen = atomicCAS(&m.st->ts[slot], (unsigned long long)kMergeNoTs, (unsigned long long)ts);
                    if (seen == kMergeNoTs) seen = (unsigned long long)ts;
                }
            }
            seen = (unsigned long long)__shfl((long long)seen, first, 64);
            if (mine) same = seen == (unsigned long long)t0;
            ask = ask && !mine;
        }
        if (claim && !same) {
            bad = 1;  // two seconds in one slot: rows 60 s or more apart
        } else if (claim && res == SG_ENTRY_NODE_RESOURCE) {
            const sg_metric_node r = m.rows[i];
            const int64_t v[5] = {r.pass_qps, r.block_qps, r.success_qps, r.exception_qps, r.rt};
            for (int c = 0; c < 5; ++c)
                if (v[c]) atomicAdd(&m.st->acc[slot][c], (unsigned long long)v[c]);
            m.st->has_entry[slot] = 1;
        } else if (claim) {
            todo = true;
            key = (uint64_t)slot * m.W + (res >> 6);
            bit = 1ull << (res & 63u);
        }
        // per (slot, word) present in the wave: one OR of its lanes' bits (a shard's rows come resource by resource,
        // so a wave holds a few words; rows in any order fall back to one atomic each after eight rounds). The ORs
        // return nothing — a wave does not wait for them; a duplicated (timestamp, resource) shows as fewer bits set
        // than resource rows counted (k_merge_bases compares the two).
        n_res += todo ? 1u : 0u;
        for (int round = 0; __ballot(todo); ++round) {
            if (round == 8) {
                if (todo) atomicOr(&m.bits[key], bit);
                break;
            }
            const int first = __builtin_ctzll(__ballot(todo));
            const uint64_t k0 = (uint64_t)__shfl((long long)key, first, 64);
            const bool mine = todo && key == k0;
            unsigned long long v = mine ? bit : 0ull;
            for (int o = 32; o > 0; o >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, o, 64);
            if (lane == first) atomicOr(&m.bits[k0], v);
            todo = todo && !mine;
        }
    }
    for (int o = 32; o > 0; o >>= 1) n_res += (uint32_t)__shfl_xor((int)n_res, o, 64);
    if (lane == 0 && n_res) atomicAdd(&m.st->n_res, (unsigned long long)n_res);
    if (bad) atomicOr(&m.st->err, kMergeBad);
}

__global__ void __launch_bounds__(kMergeScanThreads) k_merge_scan(MergeArgs m) {
    __shared__ uint32_t wsum[kMergeScanThreads / 64];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = route_lane(), wave = tid >> 6;
    if (m.st->ts[slot] == kMergeNoTs) return;  // no row named the slot (the whole block leaves)
    const unsigned long long* bits = m.bits + (size_t)slot * m.W;
    uint32_t* pre = m.pre + (size_t)slot * m.W;
    uint32_t carry = 0;
    for (uint32_t p0 = 0; p0 < m.W; p0 += kMergeScanPass) {
        const uint32_t w = p0 + (uint32_t)tid * kMergeScanPer;
        uint32_t c[kMergeScanPer], mine = 0;
#pragma unroll
        for (int u = 0; u < kMergeScanPer; ++u) {
            c[u] = w + u < m.W ? (uint32_t)__popcll(bits[w + u]) : 0u;
            mine += c[u];
        }
        uint32_t x = mine;  // inclusive scan within the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, (unsigned)o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t run = carry + x - mine, total = 0;
        for (int v = 0; v < kMergeScanThreads / 64; ++v) {
            if (v < wave) run += wsum[v];
            total += wsum[v];
        }
#pragma unroll
        for (int u = 0; u < kMergeScanPer; ++u) {
            if (w + u < m.W) pre[w + u] = run;
            run += c[u];
        }
        carry += total;
        __syncthreads();  // wsum is written again by the next pass
    }
    if (tid == 0) m.st->res_cnt[slot] = carry;
}

__global__ void __launch_bounds__(64) k_merge_bases(MergeArgs m) {
    const int j = route_lane();
    MergeSlots* st = m.st;
    const bool in = j < kMinuteS;
    const unsigned long long ts = in ? st->ts[j] : kMergeNoTs;
    const bool used = ts != kMergeNoTs;
    const uint32_t rc = used ? st->res_cnt[j] : 0u;
    int64_t v[5] = {0, 0, 0, 0, 0};
    bool entry = false;
    if (used && st->has_entry[j]) {
        for (int c = 0; c < 5; ++c) v[c] = (int64_t)st->acc[j][c];
        if (v[2] != 0) v[4] /= v[2];  // rt = Σrt / Σsuccess (ArrayMetric.fromBucket on the sums)
        entry = v[0] > 0 || v[1] > 0 || v[2] > 0 || v[3] > 0 || v[4] > 0;  // isValidMetricNode
    }
    const unsigned long long cnt = (unsigned long long)rc + (entry ? 1u : 0u);
    // rows of the earlier seconds (ascending timestamp, not slot order: the ring wraps); unused slots sort last
    unsigned long long base = 0, total = 0, placed = 0;
    for (int i = 0; i < kMinuteS; ++i) {
        const unsigned long long ti = (unsigned long long)__shfl((long long)ts, i, 64);
        const unsigned long long ci = (unsigned long long)__shfl((long long)cnt, i, 64);
        placed += (uint32_t)__shfl((int)rc, i, 64);
        if (ti < ts) base += ci;
        total += ci;
    }
    int err = st->err;
    if (placed != st->n_res) err |= kMergeBad;  // fewer bits than resource rows: a (timestamp, resource) came twice
    if (total > m.cap) err |= kMergeCap;
    if (used) st->base[j] = base;
    if (j == 0) {
        st->n_out = total;
        st->err = err;
    }
    if (!err && entry) {
        sg_metric_node r;
        r.timestamp = (int64_t)ts;
        r.pass_qps = v[0];
        r.block_qps = v[1];
        r.success_qps = v[2];
        r.exception_qps = v[3];
        r.rt = v[4];
        r.occupied_pass_qps = 0;
        r.resource = SG_ENTRY_NODE_RESOURCE;
        r.concurrency = 0;
        m.out[base + rc] = r;
    }
}

__global__ void __launch_bounds__(256) k_merge_place(MergeArgs m) {
    if (m.st->err) return;  // a contract error or too small a buffer: the caller's table stays untouched
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m.n; i += (uint64_t)gridDim.x * 256) {
        // the row as its eight 64-bit words (timestamp, pass, block, success, exception, rt, occupied pass,
        // resource | concurrency << 32), kept in registers
        const long long* src = reinterpret_cast<const long long*>(m.rows + i);
        const long long w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3], w4 = src[4], w5 = src[5], w6 = src[6],
                        w7 = src[7];
        const uint32_t res = (uint32_t)w7;
        if (res == SG_ENTRY_NODE_RESOURCE) continue;  // written once per second from the sums
        const int slot = (int)((w0 / 1000) % kMinuteS);
        const size_t word = (size_t)slot * m.W + (res >> 6);
        const unsigned long long below = m.bits[word] & ((1ull << (res & 63u)) - 1ull);
        const unsigned long long pos = m.st->base[slot] + m.pre[word] + (unsigned long long)__popcll(below);
        long long* dst = reinterpret_cast<long long*>(m.out + pos);
        dst[0] = w0;
        dst[1] = w1;
        dst[2] = w2;
        dst[3] = w3;
        dst[4] = w4;
        dst[5] = w3 != 0 ? w5 / w3 : w5;  // rt / success (ArrayMetric.fromBucket)
        dst[6] = w6;
        dst[7] = w7;
    }
}

hipError_t launch_merge_rows(const MergeArgs& m, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(m.bits, 0, sizeof(unsigned long long) * kMinuteS * (size_t)(m.W ? m.W : 1), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_merge_reset, dim3(1), dim3(64), 0, stream, m.st);
    uint64_t g = (m.n + 255) / 256;
    if (g > 4096) g = 4096;
    if (g) hipLaunchKernelGGL(k_merge_mark, dim3((unsigned)g), dim3(256), 0, stream, m);
    lds_poison(stream);
    if (g) hipLaunchKernelGGL(k_merge_scan, dim3(kMinuteS), dim3(kMergeScanThreads), 0, stream, m);
    hipLaunchKernelGGL(k_merge_bases, dim3(1), dim3(64), 0, stream, m);
    if (g) hipLaunchKernelGGL(k_merge_place, dim3((unsigned)g), dim3(256), 0, stream, m);
    return hipGetLastError();
}

}  // namespace sg
