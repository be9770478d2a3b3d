// pcodec.hip — the param-flow half of the token server's wire codec, and the exact value dictionary behind it.
//
// A MSG_TYPE_PARAM_FLOW request is [i32 xid][u8 type = 2][i64 flowId][i32 count][i32 amount] followed by `amount`
// typed parameters (ParamFlowRequestDataDecoder.decode / decodeParam, srv/codec/data/ParamFlowRequestDataDecoder.java
// :35-90; types ClusterConstants.PARAM_TYPE_*). sg_cparam_decide_batch takes u64 values, so every parameter goes
// through a dictionary: key = (type tag, canonical payload bytes) → dense id 1, 2, 3, … in order of first appearance.
//
//   k_pcodec_count   one frame per lane (payload staged in LDS where a block step's frames fit, as k_codec_decode):
//                    kind, xid, key, acquire and the number of valid parameters
//   scan             exclusive u64 scan of the counts → value_begin (block-wide, then over the block sums)
//   k_pcodec_emit    walks the parameters again: canonical payload, hash, read-only lookup in the main table. Hits
//                    get their id, misses 0 (and are counted)
//   k_vd_dedupe      misses → a per-batch table of batch positions: CAS(EMPTY → position), and atomicMin on an equal
//                    key, so the first occurrence represents the key. The bytes behind a position are the immutable
//                    batch payload: no two-phase publish
//   k_vd_flags+scan  representatives ranked in batch order → the new ids and arena offsets; the totals go to the host,
//                    which refuses a batch that does not fit (nothing has been written to the dictionary by then)
//   k_vd_commit      every miss reads its representative's id (rank → vd_next_id, vdict_sweep.h: the ids a sweep gave
//                    back first, then high + 1, …); the representative writes entries[id], its arena bytes
//                    and CAS(0 → tag | id) into the main table. The insert reads no other entry, and no lookup runs in
//                    this launch: kernel boundaries do all publishing, nothing on the device waits for another lane.
#include "engine.h"
#include "vdict_dev.h"
#include "vdict_sweep.h"

namespace sg {

namespace {

__device__ __forceinline__ int32_t be32(const uint8_t* p) {
    return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}

__device__ __forceinline__ int64_t be64(const uint8_t* p) {
    return (int64_t)(((uint64_t)(uint32_t)be32(p) << 32) | (uint64_t)(uint32_t)be32(p + 4));
}

__device__ __forceinline__ bool same_key(const VDictArgs& v, uint64_t a, uint64_t b) {
    if (v.hash[a] != v.hash[b]) return false;
    const VDesc x = v.desc[a], y = v.desc[b];
    if (x.tl != y.tl) return false;
    const uint32_t len = x.tl >> 8;
    return len <= 8 ? x.inl == y.inl : bytes_eq(v.src + x.off, v.src + y.off, len);
}

// ---- u64 scan ----

// Exclusive prefix of x over the block's 256 threads; total = the block's sum.
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t x, uint64_t* wsum, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t incl = x;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)incl, d);
        if (lane >= d) incl += y;
    }
    __syncthreads();  // wsum may still be read from the previous call
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t base = 0;
    total = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < w) base += wsum[k];
        total += wsum[k];
    }
    return base + incl - x;
}

constexpr int kScanPer = kScanTile / 256;  // elements per thread

__global__ void __launch_bounds__(256) k_scan_sums(const uint64_t* v, uint64_t n, uint64_t* sums) {
    __shared__ uint64_t wsum[4];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
    uint64_t s = 0;
    for (int k = 0; k < kScanPer; ++k)
        if (base + k < n) s += v[base + k];
    uint64_t total;
    block_scan_excl(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_scan_top(uint64_t* sums, uint64_t nb, uint64_t* total_out) {  // one block
    __shared__ uint64_t wsum[4];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += 256) {
        const uint64_t b = b0 + threadIdx.x;
        const uint64_t x = b < nb ? sums[b] : 0;
        uint64_t total;
        const uint64_t ex = block_scan_excl(x, wsum, total);
        if (b < nb) sums[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(256) k_scan_apply(uint64_t* v, uint64_t n, const uint64_t* sums) {
    __shared__ uint64_t wsum[4];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
    uint64_t x[kScanPer];
    uint64_t s = 0;
    for (int k = 0; k < kScanPer; ++k) {
        x[k] = base + k < n ? v[base + k] : 0;
        s += x[k];
    }
    uint64_t total;
    uint64_t run = sums[blockIdx.x] + block_scan_excl(s, wsum, total);
    for (int k = 0; k < kScanPer; ++k) {
        if (base + k < n) v[base + k] = run;
        run += x[k];
    }
}

// ---- the frame walk ----

constexpr int kDecFrames = 256;        // frames per block step (one per thread)
constexpr uint32_t kDecStage = 16384;  // LDS bytes staged per step
constexpr uint32_t kHead = 5 + 16;     // xid, type, flowId, count, amount

// decodeParam `amount` times over frame p[0, len), f(k, type, pos, size) for the k-th valid parameter whose payload
// is p[pos, pos + size). False where the Java decoder would throw: a read past the frame's end or a negative string
// length. An unknown type byte consumes that byte and adds no parameter.
template <class F>
__device__ __forceinline__ bool walk_params(const uint8_t* p, uint32_t len, int32_t amount, uint32_t& n_valid, F f) {
    n_valid = 0;
    if ((uint32_t)amount > len - kHead) return false;  // every parameter takes at least its type byte
    uint32_t pos = kHead;
    for (int32_t a = 0; a < amount; ++a) {
        if (pos >= len) return false;
        const uint32_t t = p[pos++];
        uint32_t size = 0;
        bool valid = true;
        switch (t) {
            case SG_PARAM_TYPE_INTEGER: size = 4; break;
            case SG_PARAM_TYPE_LONG: size = 8; break;
            case SG_PARAM_TYPE_BYTE: size = 1; break;
            case SG_PARAM_TYPE_DOUBLE: size = 8; break;
            case SG_PARAM_TYPE_FLOAT: size = 4; break;
            case SG_PARAM_TYPE_SHORT: size = 2; break;
            case SG_PARAM_TYPE_BOOLEAN: size = 1; break;
            case SG_PARAM_TYPE_STRING: {
                if (len - pos < 4) return false;
                const int32_t L = be32(p + pos);
                pos += 4;
                if (L < 0) return false;  // new byte[length]: NegativeArraySizeException
                size = (uint32_t)L;
                break;
            }
            default: valid = false; break;
        }
        if (size > len - pos) return false;
        if (valid) f(n_valid++, t, pos, size);
        pos += size;
    }
    return true;
}

__device__ __forceinline__ uint64_t fid_hash(int64_t fid) { return mix64((uint64_t)fid); }

__device__ __forceinline__ void count_frame(const PCodecArgs& c, uint64_t i, const uint8_t* p, uint32_t len) {
    sg_cparam_req r;
    r.ts_ms = c.ts[i];
    r.key = SG_KEY_BAD;
    r.acquire = 0;
    r.value_begin = 0;  // k_pcodec_emit
    r.value_count = 0;
    int32_t xid = 0;
    uint8_t kind;
    if (len < 5) {  // DefaultRequestEntityDecoder.decode: readableBytes() >= 5, else null
        kind = SG_FRAME_SHORT;
    } else {
        xid = be32(p);
        const int type = (int)(int8_t)p[4];
        if (type != SG_MSG_TYPE_PARAM_FLOW) {
            kind = SG_FRAME_OTHER;
        } else if (len >= (1u << 24)) {  // a value record keeps the payload length in 24 bits (header: frame size)
            kind = SG_FRAME_MALFORMED;
        } else if (len - 5 < 16) {  // ParamFlowRequestDataDecoder.decode: readableBytes() >= 16, else null (:36)
            kind = SG_FRAME_NO_DATA;
        } else {
            const int64_t fid = be64(p + 5);
            const int32_t count = be32(p + 13), amount = be32(p + 17);
            uint32_t nv = 0;
            if (amount <= 0) {  // (:42) null
                kind = SG_FRAME_NO_DATA;
            } else if (!walk_params(p, len, amount, nv, [](uint32_t, uint32_t, uint32_t, uint32_t) {})) {
                kind = SG_FRAME_MALFORMED;
            } else {
                kind = SG_FRAME_PARAM;
                r.acquire = count;
                r.value_count = nv;
                if (fid > 0) {  // else SG_KEY_BAD: DefaultTokenService.requestParamToken → badRequest() (:54-56)
                    uint32_t key = SG_KEY_NO_RULE;
                    for (uint64_t h = fid_hash(fid) & c.fid_mask;; h = (h + 1) & c.fid_mask) {
                        const FidSlot s = c.fid_tab[h];
                        if (s.fid == fid) {
                            key = s.idx;
                            break;
                        }
                        if (s.fid == 0) break;  // the table is never full
                    }
                    r.key = key;
                }
            }
        }
    }
    c.req[i] = r;
    c.xid[i] = xid;
    c.kind[i] = kind;
    c.cnt[i] = r.value_count;
}

// The block-step frame loop of k_codec_decode (codec.hip): kDecFrames consecutive frames staged in LDS with aligned
// 4-byte loads where their bytes fit, read from HBM in place where they do not. f(i, p, len, off) per frame.
template <class F>
__device__ __forceinline__ void for_each_frame(const PCodecArgs& c, uint32_t* stage, F f) {
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
    for (uint64_t i0 = (uint64_t)blockIdx.x * kDecFrames; i0 < c.n; i0 += (uint64_t)gridDim.x * kDecFrames) {
        const uint64_t i1 = min(i0 + (uint64_t)kDecFrames, c.n);
        const uint32_t lo = c.offsets[i0], hi = c.offsets[i1];
        const uint32_t a0 = lo & ~3u;
        const bool staged = hi >= lo && hi - a0 <= kDecStage;
        if (staged && hi > lo) {
            const uint32_t words = (hi - a0 + 3) / 4;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(c.payload) + a0 / 4;
            for (uint32_t w = threadIdx.x; w < words; w += kDecFrames) stage[w] = src[w];
        }
        __syncthreads();
        const uint64_t i = i0 + threadIdx.x;
        if (i < i1) {
            const uint32_t off = c.offsets[i], end = c.offsets[i + 1];
            const uint32_t len = end >= off ? end - off : 0u;  // a backwards frame decodes as SG_FRAME_SHORT
            // a frame of a staged step lies inside [lo, hi) when the offsets are non-decreasing; one that does not
            // (offsets out of order) is read in place
            const bool in_stage = staged && off >= lo && end <= hi;
            f(i, in_stage ? sb + (off - a0) : c.payload + off, len, off);
        }
        __syncthreads();  // the stage is refilled by the next step
    }
}

__global__ void __launch_bounds__(kDecFrames) k_pcodec_count(PCodecArgs c) {
    __shared__ uint32_t stage[kDecStage / 4];
    for_each_frame(c, stage, [&](uint64_t i, const uint8_t* p, uint32_t len, uint32_t) { count_frame(c, i, p, len); });
}

__global__ void __launch_bounds__(kDecFrames) k_pcodec_emit(PCodecArgs c) {
    __shared__ uint32_t stage[kDecStage / 4];
    for_each_frame(c, stage, [&](uint64_t i, const uint8_t* p, uint32_t len, uint32_t off) {
        const uint64_t vb = c.cnt[i];
        c.req[i].value_begin = (uint32_t)vb;
        if (c.kind[i] != SG_FRAME_PARAM) return;
        uint32_t nv;
        walk_params(p, len, be32(p + 17), nv, [&](uint32_t k, uint32_t type, uint32_t pos, uint32_t size) {
            vd_lookup_store(c.vd, vb + k, type, p + pos, off + pos, size);
        });
    });
}

__global__ void __launch_bounds__(256) k_pcodec_encode(PCodecArgs c) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (c.kind_in[i] == SG_FRAME_PARAM) {
            const sg_result r = c.res[i];
            const uint32_t x = (uint32_t)c.xid_in[i];
            // [u16 14][i32 xid][u8 type][u8 status][i32 remaining][i32 waitInMs = 0]: ParamFlowRequestProcessor
            // .toResponse builds FlowTokenResponseData without a wait time (srv/processor/ParamFlowRequestProcessor)
            w.x = (14u << 8) | ((x >> 24) << 16) | (((x >> 16) & 0xFFu) << 24);
            w.y = ((x >> 8) & 0xFFu) | ((x & 0xFFu) << 8) | ((uint32_t)SG_MSG_TYPE_PARAM_FLOW << 16) |
                  (((uint32_t)r.status & 0xFFu) << 24);
            w.z = __builtin_bswap32((uint32_t)r.remaining);
        }
        reinterpret_cast<uint4*>(c.frames)[i] = w;
    }
}

// ---- the dictionary's batch kernels ----

// sg_vdict_intern: the uploaded (types, offsets, bytes) arrays through the decoder's lookup
__global__ void __launch_bounds__(256) k_vd_host_lookup(VDictArgs v) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m) return;
    const uint32_t off = v.offsets[j];
    vd_lookup_store(v, j, v.types[j], v.src + off, off, v.offsets[j + 1] - off);
}

__global__ void __launch_bounds__(256) k_vd_dedupe(VDictArgs v) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m || v.ids[j] != 0) return;
    for (uint64_t s = v.hash[j] & v.dedupe_mask;; s = (s + 1) & v.dedupe_mask) {  // >= 2 slots per miss: it ends
        uint32_t cur = v.dedupe[s];
        if (cur == kVdEmpty) cur = atomicCAS(&v.dedupe[s], kVdEmpty, (uint32_t)j);
        // whatever position the slot holds now or later has the key of `cur`: atomicMin keeps the key
        if (cur == kVdEmpty || same_key(v, j, cur)) {
            if (cur != kVdEmpty) atomicMin(&v.dedupe[s], (uint32_t)j);
            v.slot_of[j] = (uint32_t)s;
            return;
        }
    }
}

__global__ void __launch_bounds__(256) k_vd_flags(VDictArgs v) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m) return;
    uint64_t f = 0;
    if (v.ids[j] == 0 && v.dedupe[v.slot_of[j]] == (uint32_t)j) {
        const uint32_t len = v.desc[j].tl >> 8;
        f = (1ull << 32) | (len > 8 ? len : 0u);  // the arena bytes of a batch sum to less than its source's 2^32
    }
    v.scan[j] = f;
}

__global__ void __launch_bounds__(256) k_vd_commit(VDictArgs v) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m || v.ids[j] != 0) return;  // ids[j] is read and written by this lane alone
    const uint32_t rep = v.dedupe[v.slot_of[j]];
    const uint64_t sc = v.scan[rep];
    const uint64_t id = vd_next_id(sc >> 32, v.free_ids, v.n_free, v.high);  // a swept id again while they last
    v.ids[j] = id;
    if (rep != (uint32_t)j) return;
    const VDesc d = v.desc[j];
    const uint64_t h = v.hash[j];
    VEntry e;
    e.hash = h;
    e.len = d.tl >> 8;
    e.type = d.tl & 0xFFu;
    if (e.len <= 8) {
        e.data = d.inl;
    } else {
        e.data = v.arena_used + (sc & 0xFFFFFFFFu);
        for (uint32_t k = 0; k < e.len; ++k) v.arena[e.data + k] = v.src[d.off + k];
    }
    v.entries[id] = e;
    const uint64_t val = (h & 0xFFFFFFFF00000000ull) | id;
    for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask)  // new keys are pairwise distinct: no compare
        if (v.tab[s] == 0 && atomicCAS((unsigned long long*)&v.tab[s], 0ull, (unsigned long long)val) == 0ull) return;
}

__global__ void __launch_bounds__(256) k_vd_gather(const VEntry* entries, const uint64_t* ids, uint64_t n, VEntry* out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = entries[ids[j]];
}

__global__ void __launch_bounds__(256) k_vd_bytes(const VEntry* e, const uint32_t* offsets, uint64_t n,
                                                  const uint8_t* arena, uint8_t* out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const VEntry x = e[j];
    uint8_t* o = out + offsets[j];
    for (uint32_t k = 0; k < x.len; ++k) o[k] = x.len <= 8 ? (uint8_t)(x.data >> (8 * k)) : arena[x.data + k];
}

// sg_vdict_grow: the zeroed main table of the grown dictionary filled from its entries, one lane per id in [1, high]
// (a swept id's tombstone is skipped). The hash
// is computed again from the entry's payload with the lookup's function (vd_lookup_store), so the slot an id lands
// on is the one every later lookup of its value probes from.
__global__ void __launch_bounds__(256) k_vd_rehash(VDictArgs v) {
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (id > v.high) return;
    const VEntry e = v.entries[id];
    if (e.type == kVdTombType) return;  // a swept id: in no table until a batch takes it again
    const bool inl = e.len <= 8;
    const uint64_t h = value_hash((e.len << 8) | e.type, inl ? e.data : 0, inl ? v.arena : v.arena + e.data);
    const uint64_t val = (h & 0xFFFFFFFF00000000ull) | id;
    for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask)  // the entries are pairwise distinct: no compare
        if (v.tab[s] == 0 && atomicCAS((unsigned long long*)&v.tab[s], 0ull, (unsigned long long)val) == 0ull) return;
}

unsigned grid_for(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

unsigned frame_grid(uint64_t n) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}

}  // namespace

hipError_t launch_scan_u64(uint64_t* v, uint64_t n, uint64_t* sums, uint64_t* total, hipStream_t stream) {
    const uint64_t nb = scan_blocks(n);
    if (nb) hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(256), 0, stream, v, n, sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, stream, sums, nb, total);
    if (nb) hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(256), 0, stream, v, n, sums);
    return hipGetLastError();
}

hipError_t launch_pcodec_count(const PCodecArgs& c, hipStream_t stream) {
    if (((uintptr_t)c.payload & 3u) != 0) return hipErrorInvalidValue;  // staged loads are 4-byte words
    lds_poison(stream);
    hipLaunchKernelGGL(k_pcodec_count, dim3(frame_grid(c.n)), dim3(kDecFrames), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_pcodec_emit(const PCodecArgs& c, hipStream_t stream) {
    if (((uintptr_t)c.payload & 3u) != 0) return hipErrorInvalidValue;
    lds_poison(stream);
    hipLaunchKernelGGL(k_pcodec_emit, dim3(frame_grid(c.n)), dim3(kDecFrames), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_pcodec_encode(const PCodecArgs& c, hipStream_t stream) {
    hipLaunchKernelGGL(k_pcodec_encode, dim3(frame_grid(c.n)), dim3(256), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_vd_host_lookup(const VDictArgs& v, hipStream_t stream) {
    hipLaunchKernelGGL(k_vd_host_lookup, dim3(grid_for(v.m, 256)), dim3(256), 0, stream, v);
    return hipGetLastError();
}

hipError_t launch_vd_dedupe(const VDictArgs& v, hipStream_t stream) {
    hipLaunchKernelGGL(k_vd_dedupe, dim3(grid_for(v.m, 256)), dim3(256), 0, stream, v);
    hipLaunchKernelGGL(k_vd_flags, dim3(grid_for(v.m, 256)), dim3(256), 0, stream, v);
    return hipGetLastError();
}

hipError_t launch_vd_commit(const VDictArgs& v, hipStream_t stream) {
    hipLaunchKernelGGL(k_vd_commit, dim3(grid_for(v.m, 256)), dim3(256), 0, stream, v);
    return hipGetLastError();
}

hipError_t launch_vd_rehash(const VDictArgs& v, hipStream_t stream) {
    if (v.high == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vd_rehash, dim3(grid_for(v.high, 256)), dim3(256), 0, stream, v);
    return hipGetLastError();
}

hipError_t launch_vd_gather(const VEntry* entries, const uint64_t* ids, uint64_t n, VEntry* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_vd_gather, dim3(grid_for(n, 256)), dim3(256), 0, stream, entries, ids, n, out);
    return hipGetLastError();
}

hipError_t launch_vd_bytes(const VEntry* e, const uint32_t* offsets, uint64_t n, const uint8_t* arena, uint8_t* out,
                           hipStream_t stream) {
    hipLaunchKernelGGL(k_vd_bytes, dim3(grid_for(n, 256)), dim3(256), 0, stream, e, offsets, n, arena, out);
    return hipGetLastError();
}

}  // namespace sg
