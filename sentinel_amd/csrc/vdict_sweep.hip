// vdict_sweep.hip — sg_vdict_sweep's device passes: which ids of the value dictionary something still names, and the
// dictionary built again beside the one in force without the others (api.cpp swaps it in).
//
//   mark     a zeroed bitmap of high + 1 bits; one pass per kind of source sets the bit of every id it names:
//              k_vds_mark_words  value words at a fixed stride (PSlot tables, the cluster param keys[], the thread
//                                counts behind their owner word, the hot-item arrays, the gateway's two ids)
//              k_vds_mark_blog   block-log rows not yet fetched whose app word is a value or a label id
//              k_vds_mark_slog   server-log slots not yet fetched of the param family
//              k_vds_mark_keep   the caller's keep list, which also counts the entries that are no live id
//            A lane reads its bitmap word and issues the atomicOr only while its bit is clear: hot values repeat across
//            rules and tables. Bounds: vds_mark returns unless 1 <= id <= high, so the word index id >> 5 is at most
//            high >> 5, the last of the (high >> 5) + 1 words; table extents are the handle's own sizes.
//   flags    one lane per id in [1, high]: dead (a tombstone already, or not marked) → 1 in dead[], and the length of
//            a live payload longer than 8 bytes in bytes[]. The host scans both with launch_scan_u64 (two scans: ids
//            stay below 2^29 but the arena may pass 2^32 bytes, so the two do not share a word) → each dead id's
//            position in the ascending free list and each live long payload's offset in the compacted arena.
//   move     one lane per id: a dead id gets a tombstone and its place in the free list; a live one its entry with the
//            new arena offset, its bytes, and hash[63:32] << 32 | id in the zeroed new main table (entries are
//            pairwise distinct: CAS on empty, no compare, as k_vd_rehash). Payloads of up to kVdsCoopMin bytes are
//            copied by their lane, as k_vd_commit copies; longer ones by the whole wave, one string after the other,
//            with 16-byte accesses where source and destination are congruent modulo 16.
// Nothing here waits for another lane: kernel boundaries publish the bitmap, the scans and the new tables.
#include "engine.h"
#include "serverlog_rules.h"
#include "vdict_sweep.h"

namespace sg {

static_assert(kVdsOk == SG_OK && kVdsInval == SG_E_INVAL, "vdict_sweep.h restates the status codes");
static_assert(SG_BLOCK_APP_VALUE == 3 && SG_BLOCK_APP_LABEL == 6 && kSlogParam == 1u,
              "vdict_sweep.h restates the log tables' kinds");
static_assert(sizeof(PSlot) == 32 && sizeof(PSThread) == 32 && sizeof(sg_param_hot_item) == 16,
              "the strided mark pass reads these as u64 words");

namespace {

__device__ __forceinline__ void vds_mark(uint32_t* bits, uint64_t high, uint64_t id) {
    if (!vd_id_in_range(id, high)) return;  // not a dictionary id: the ~0 of an empty or side slot, a caller's own number
    uint32_t* w = bits + (id >> 5);         // id <= high: within the (high >> 5) + 1 words
    const uint32_t bit = 1u << (id & 31);
    if (!(*w & bit)) atomicOr(w, bit);
}

__device__ __forceinline__ bool vds_marked(const uint32_t* bits, uint64_t id) { return (bits[id >> 5] >> (id & 31)) & 1u; }

// words[i * stride + value_off] for i < n; with guard_off >= 0 only behind a taken owner word (PSThread).
__global__ void __launch_bounds__(256) k_vds_mark_words(uint32_t* bits, uint64_t high, const uint64_t* words, uint64_t n,
                                                        uint32_t stride, uint32_t value_off, int guard_off) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t* e = words + i * stride;
        if (guard_off >= 0 && !vd_thread_names_id(e[guard_off])) continue;
        vds_mark(bits, high, e[value_off]);
    }
}

__global__ void __launch_bounds__(256) k_vds_mark_blog(uint32_t* bits, uint64_t high, const BlogSlot* tab, uint64_t slots) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
        if (vd_blog_names_id(tab[i].tag, tab[i].kind)) vds_mark(bits, high, tab[i].app);
}

__global__ void __launch_bounds__(256) k_vds_mark_slog(uint32_t* bits, uint64_t high, const SlogSlot* tab, uint64_t slots) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
        if (vd_slog_names_id(tab[i].tag, tab[i].family)) vds_mark(bits, high, tab[i].value);
}

__global__ void __launch_bounds__(256) k_vds_mark_keep(uint32_t* bits, uint64_t high, const uint64_t* keep, uint64_t n,
                                                       const VEntry* entries, unsigned long long* bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t id = keep[i];
        const bool is_free = vd_id_in_range(id, high) && entries[id].type == kVdTombType;
        if (vd_keep_bad(id, high, is_free))
            atomicAdd(bad, 1ull);  // a refusal follows: no need to be fast
        else
            vds_mark(bits, high, id);
    }
}

__global__ void __launch_bounds__(256) k_vds_flags(VdSweepArgs a) {
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (id > a.high) return;
    const VEntry e = a.entries[id];
    const bool dead = e.type == kVdTombType || !vds_marked(a.bits, id);
    a.dead[id - 1] = dead;
    a.bytes[id - 1] = !dead && e.len > 8 ? e.len : 0;
}

// All 64 lanes copy s[0, len) → d[0, len).
__device__ __forceinline__ void vds_wave_copy(const uint8_t* s, uint8_t* d, uint32_t len, uint32_t lane) {
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) != 0) {  // no common 16-byte phase: bytes, consecutive lanes side by side
        for (uint32_t k = lane; k < len; k += 64) d[k] = s[k];
        return;
    }
    const uint32_t head = min((uint32_t)(-(uintptr_t)d & 15u), len);
    if (lane < head) d[lane] = s[lane];
    const uint32_t vecs = (len - head) >> 4;  // whole 16-byte words inside [head, len)
    const uint4* sv = reinterpret_cast<const uint4*>(s + head);
    uint4* dv = reinterpret_cast<uint4*>(d + head);
    for (uint32_t k = lane; k < vecs; k += 64) dv[k] = sv[k];
    const uint32_t done = head + (vecs << 4);  // len - done < 16
    if (done + lane < len) d[done + lane] = s[done + lane];
}

__global__ void __launch_bounds__(256) k_vds_move(VdSweepArgs a) {
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    const uint8_t* src = nullptr;  // this lane's payload, left to the wave
    uint8_t* dst = nullptr;
    uint32_t clen = 0;
    if (id <= a.high) {
        VEntry e = a.entries[id];
        if (e.type == kVdTombType || !vds_marked(a.bits, id)) {
            VEntry t;
            t.hash = 0;
            t.data = 0;
            t.len = 0;
            t.type = kVdTombType;
            a.n_entries[id] = t;
            a.n_free_ids[a.dead[id - 1]] = (uint32_t)id;  // the scan's rank: below the dead total the list is sized for
        } else {
            if (e.len > 8) {
                const uint8_t* s = a.arena + e.data;
                e.data = a.bytes[id - 1];  // + e.len <= the live total <= arena_used: inside the new arena
                uint8_t* d = a.n_arena + e.data;
                if (e.len > kVdsCoopMin) {
                    src = s;
                    dst = d;
                    clen = e.len;
                } else {
                    for (uint32_t k = 0; k < e.len; ++k) d[k] = s[k];
                }
            }
            a.n_entries[id] = e;
            const uint64_t val = (e.hash & 0xFFFFFFFF00000000ull) | id;
            for (uint64_t s = e.hash & a.n_tab_mask;; s = (s + 1) & a.n_tab_mask)  // at most half full: it ends
                if (a.n_tab[s] == 0 && atomicCAS((unsigned long long*)&a.n_tab[s], 0ull, (unsigned long long)val) == 0ull)
                    break;
        }
    }
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t m = __ballot(clen != 0); m; m &= m - 1) {
        const int l = __ffsll((unsigned long long)m) - 1;
        const uint8_t* s = reinterpret_cast<const uint8_t*>(__shfl((unsigned long long)(uintptr_t)src, l));
        uint8_t* d = reinterpret_cast<uint8_t*>(__shfl((unsigned long long)(uintptr_t)dst, l));
        vds_wave_copy(s, d, (uint32_t)__shfl((int)clen, l), lane);
    }
}

unsigned vds_grid(uint64_t n, unsigned cap) {
    uint64_t g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

}  // namespace

hipError_t launch_vds_mark_words(uint32_t* bits, uint64_t high, const uint64_t* words, uint64_t n, uint32_t stride,
                                 uint32_t value_off, int guard_off, hipStream_t stream) {
    if (n == 0 || !words) return hipSuccess;
    hipLaunchKernelGGL(k_vds_mark_words, dim3(vds_grid(n, 8192)), dim3(256), 0, stream, bits, high, words, n, stride,
                       value_off, guard_off);
    return hipGetLastError();
}

hipError_t launch_vds_mark_blog(uint32_t* bits, uint64_t high, const BlogSlot* tab, uint64_t slots, hipStream_t stream) {
    if (slots == 0 || !tab) return hipSuccess;
    hipLaunchKernelGGL(k_vds_mark_blog, dim3(vds_grid(slots, 8192)), dim3(256), 0, stream, bits, high, tab, slots);
    return hipGetLastError();
}

hipError_t launch_vds_mark_slog(uint32_t* bits, uint64_t high, const SlogSlot* tab, uint64_t slots, hipStream_t stream) {
    if (slots == 0 || !tab) return hipSuccess;
    hipLaunchKernelGGL(k_vds_mark_slog, dim3(vds_grid(slots, 8192)), dim3(256), 0, stream, bits, high, tab, slots);
    return hipGetLastError();
}

hipError_t launch_vds_mark_keep(uint32_t* bits, uint64_t high, const uint64_t* keep, uint64_t n, const VEntry* entries,
                                unsigned long long* bad, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vds_mark_keep, dim3(vds_grid(n, 8192)), dim3(256), 0, stream, bits, high, keep, n, entries, bad);
    return hipGetLastError();
}

hipError_t launch_vds_flags(const VdSweepArgs& a, hipStream_t stream) {
    if (a.high == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vds_flags, dim3((unsigned)((a.high + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_vds_move(const VdSweepArgs& a, hipStream_t stream) {
    if (a.high == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vds_move, dim3((unsigned)((a.high + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sg
