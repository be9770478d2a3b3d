// vdict_sweep.h — the rules of sg_vdict_sweep that need no device: the order of its refusals, which id a fresh value
// takes once ids have been given back, the host's bookkeeping after a batch, and when a word of a log table or of the
// thread-count table names a dictionary id. Plain functions, no HIP runtime in here: api.cpp asks them on the host, the
// mark kernels (vdict_sweep.hip) and k_vd_commit (pcodec.hip) call the shared ones per lane, and
// tests/cpp/test_vdict_sweep_host.cpp checks all of them on the CPU against a brute-force restatement.
//
// The dictionary after a sweep: ids stay array positions in [1, high]; every one of them is live or free, so
// high = live + free at all times. The free ids are listed in ascending order; a batch's fresh values, ranked by first
// appearance, take them from the front and go on at high + 1 when the list runs out.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_VDS_FN __host__ __device__ inline
#else
#define SG_VDS_FN inline
#endif

namespace sg {

constexpr int kVdsOk = 0, kVdsInval = -1;  // SG_OK, SG_E_INVAL (static_asserted where sentinel_gpu.h is in sight)

constexpr uint32_t kVdTombType = 0xFFFFFFFFu;  // VEntry::type of a freed id (SG_PARAM_TYPE_* end at 7)
constexpr uint32_t kVdsCoopMin = 256;          // payloads above this many bytes are copied by a whole wave

// ---- the refusals, in order; nothing has changed when one of them is returned ----

struct VdsRefusal {
    int code;
    const char* why;
};

// on: sg_vdict_init has run. bad_keep: keep_ids entries that are 0, above high or already free (vd_keep_bad over the
// list; the range half is known on the host before any launch, the free half after the mark pass, and both come
// before the swap).
inline VdsRefusal vd_sweep_refusal(bool on, uint64_t n_keep, bool keep_null, uint64_t bad_keep) {
    if (!on) return {kVdsInval, "sg_vdict_init first"};
    if (n_keep > 0 && keep_null) return {kVdsInval, "null keep_ids"};
    if (bad_keep > 0) return {kVdsInval, "a keep_ids entry is 0, above the highest id or already free"};
    return {kVdsOk, ""};
}

SG_VDS_FN bool vd_id_in_range(uint64_t id, uint64_t high) { return id >= 1 && id <= high; }

// One keep_ids entry. is_free is read only for an id in range (entries[id] is a tombstone).
SG_VDS_FN bool vd_keep_bad(uint64_t id, uint64_t high, bool is_free) { return !vd_id_in_range(id, high) || is_free; }

// ---- ids of fresh values ----

// The id of the fresh value of rank `rank` (0-based, by first appearance in the batch): the rank-th remaining free id
// while they last, then high + 1, high + 2, …. free_ids[0 .. n_free) are the remaining free ids, ascending.
SG_VDS_FN uint64_t vd_next_id(uint64_t rank, const uint32_t* free_ids, uint64_t n_free, uint64_t high) {
    return rank < n_free ? (uint64_t)free_ids[rank] : high + 1 + (rank - n_free);
}

// The host's counters; head indexes the free list as the sweep wrote it (n_free_total entries).
struct VdBook {
    uint64_t head;   // free ids consumed since the sweep that wrote the list
    uint64_t n_free; // free ids remaining
    uint64_t high;   // largest id ever handed out
    uint64_t live;   // values
};

// After a batch that added `fresh` values.
inline VdBook vd_after_batch(VdBook b, uint64_t fresh) {
    const uint64_t reused = fresh < b.n_free ? fresh : b.n_free;
    b.head += reused;
    b.n_free -= reused;
    b.high += fresh - reused;
    b.live += fresh;
    return b;
}

// ---- which table words name an id ----

// A thread-count entry (PSThread): the value of an entry whose owner word is taken, whatever its count — an entry
// without its exit still counts a running call of that value.
SG_VDS_FN bool vd_thread_names_id(unsigned long long owner) { return owner != 0; }

// A block-log row (BlogSlot): a published tag (bit 63; no writer is in flight after the drain) means a row not yet
// fetched; its app word is a dictionary id for kinds SG_BLOCK_APP_VALUE (3) and SG_BLOCK_APP_LABEL (6).
SG_VDS_FN bool vd_blog_names_id(uint64_t tag, uint32_t kind) { return (tag >> 63) != 0 && (kind == 3u || kind == 6u); }

// A server-log slot (SlogSlot): published the same way; only the param family (kSlogParam = 1) carries a value id.
SG_VDS_FN bool vd_slog_names_id(uint64_t tag, uint32_t family) { return (tag >> 63) != 0 && family == 1u; }

}  // namespace sg
