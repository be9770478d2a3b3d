// api.cpp — the C ABI of libsentinel_gpu.so (include/sentinel_gpu.h): handle, rule tables, batch
// driver. Device work is in the .hip files; device and pinned memory is owned through devmem.h's types.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <thread>
#include <tuple>
#include <vector>

#include "devmem.h"
#include "engine.h"
#include "table_grow.h"
#include "vdict_sweep.h"

using namespace sg;

bool sg::DevAlloc::alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }
void sg::DevAlloc::free(void* p) { (void)hipFree(p); }
bool sg::PinnedAlloc::alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes) == hipSuccess; }
void sg::PinnedAlloc::free(void* p) { (void)hipHostFree(p); }
using Stream = UniqueHandle<hipStream_t, hipError_t, hipStreamDestroy>;
using Event = UniqueHandle<hipEvent_t, hipError_t, hipEventDestroy>;

// Host-path staging of a handle or a node: device copies of a _host entry point's inputs (slots 0, 2, 3) and of its
// output (slot 1). The _host entry points are synchronous and none calls another while its staged data is live, so
// they share the slots; each slot grows to its largest use.
struct Staging {
    DevBuf<uint8_t> slot[4];
    template <class T>
    bool get(int i, uint64_t n, T*& p) {
        if (!slot[i].reserve(n * sizeof(T))) return false;
        p = reinterpret_cast<T*>(slot[i].get());
        return true;
    }
};

constexpr int kAsyncSlots = 3;  // batches of one handle in flight on the host pipeline
constexpr int kDevSlots = 4;    // device-buffer batches of one handle in flight (sg_flow_enqueue)

struct sg_handle {
    ~sg_handle();  // makes `device` current and drains the handle's streams before the members free their memory
    int device = 0;
    sg_config cfg{};
    std::string err;

    std::vector<sg_namespace> ns;
    std::vector<sg_flow_rule> rules;  // as loaded (current rule per key)
    std::vector<Rule> rule_tab;       // device image
    uint32_t K = 0;
    int stride = 0;                   // buckets per flowId
    int n_wl = 0;
    int32_t wl[kMaxWl]{};

    DevBuf<Rule> d_rules;
    DevBuf<Bucket> d_ring;
    DevBuf<BucketHot> d_hot;          // start / PASS / WAITING of every bucket (the short walkers' gather)
    DevBuf<Occ> d_occ;
    // binned front half (engine.hip k_bin_sort): the hot flowIds of the previous batch
    DevBuf<uint32_t> d_hot_key;       // [kBinHot] flowId per hot slot, then the table [kHotTab] {flowId, slot}
    uint64_t hot_gen = ~0ull;         // rules_gen the hot set was reset for
    uint64_t rules_gen = 0;           // flow rule loads so far (a reload renumbers flowIds: the hot set restarts)
    int bin_mode = 1;                 // env SG_BIN: 0 off, 1 on for >= 2^14 flowIds, 2 on whenever the records allow
    int prep_tiles = 4;               // env SG_PREP_TILES: sort tiles per k_prep block on the binned path

    // A flow batch's workspace (flow_ws_alloc: sized for cfg.max_batch; seg_end for the loaded rules). Workspace 0
    // serves every synchronous batch and every other pipelined one; the limiter, cparam, local, pace and node paths
    // borrow its buffers. Workspace 1 is allocated on the first pipelined batch (pipe_setup).
    struct FlowWs {
        DevBuf<uint64_t> rec;
        DevBuf<uint64_t> rec_sorted;
        DevBuf<uint32_t> hist;        // radix sort histogram workspace
        DevBuf<uint32_t> bnd;
        DevBuf<int64_t> p0;
        DevBuf<uint32_t> np;
        DevBuf<int> err;
        DevBuf<uint32_t> long_list;
        DevBuf<uint32_t> long_key;    // flowId of each long_list entry (cluster flow path)
        DevBuf<uint32_t> long_end;    // segment end of each long_list entry (cluster flow path)
        DevBuf<uint32_t> long_pend;   // [kLongTab][kLongPeriods] period ends of the long segments
        DevBuf<uint32_t> short_list;
        DevBuf<uint32_t> short_key;   // flowId of each short_list entry (cluster flow path)
        DevBuf<uint32_t> short_end;   // segment end of each short_list entry (cluster flow path)
        DevBuf<uint32_t> counts;      // [1 + kClasses]: long count, short counts per class
        DevBuf<uint4> skips;
        DevBuf<uint32_t> skip_count;
        DevBuf<uint32_t> seg_end;     // [2 * seg_cap] end, then start (k_seg_mark) of each flowId's segment in the
        uint32_t seg_cap = 0;         // sorted records; seg_cap > K flowIds each (flow_seg_alloc), 0 without rules
        uint32_t* seg_start = nullptr;  // seg_end + seg_cap, all 0xFFFFFFFF between batches
        DevBuf<uint64_t> bin_buf;     // binned front half: the regular bins after the scatter (max_batch records)
    };
    FlowWs ws[2];
    uint64_t* last_sorted = nullptr;  // whichever of ws[0].rec / ws[0].rec_sorted holds the last sort result
    uint64_t last_rec4_n = 0;         // > 0: that batch (of this many requests) left 4-byte sorted records (BatchArgs::rec4)
    DevBuf<int64_t> d_last_ts;        // {last_ts, front_ts}
    int64_t* d_front_ts = nullptr;    // d_last_ts + 1. Pipelined limiter batches: last timestamp of the latest accepted front half
    DevBuf<FidSlot> d_fid;            // flowId → rule index (wire codec), 2^k slots
    uint64_t fid_mask = 0;
    uint64_t class_off[kClasses]{};
    DevBuf<unsigned long long> d_dbg;      // [128] debug counters (SG_DEBUG & 64)
    PinnedBuf<int> h_err;
    PinnedBuf<uint32_t> h_long;       // long segment count, skipped range count

    Staging stage;                    // the _host entry points' device copies (host_batch)

    // namespace QPS limiters (GlobalRequestLimiter): slot per namespace, device rings and scratch
    std::vector<int> ns_slot;
    int n_lim = 0;
    double lim_qps[kMaxLim]{};
    int lim_wl_idx = -1;
    DevBuf<LimRing> d_lim_ring;
    DevBuf<uint8_t> d_rule_lim;
    DevBuf<uint8_t> d_lim_slot;
    DevBuf<uint32_t> d_lim_tile;      // tile totals then tile offsets
    DevBuf<uint32_t> d_lim_period;    // arrivals, prefix, quota

    // hot-parameter flow control
    std::vector<sg_param_rule> prules;
    std::vector<PRule> ptab;
    DevBuf<PRule> d_prules;
    DevBuf<sg_param_hot_item> d_phot;
    DevBuf<PSlot> d_ptable;
    uint64_t ptotal = 0;             // slots over all rule sub-tables
    DevBuf<int64_t> d_plast_ts;

    // pace controller (RateLimiterController per FlowRule)
    std::vector<PaceRule> pace_tab;
    DevBuf<PaceRule> d_pace_rules;
    DevBuf<int64_t> d_pace_latest;
    DevBuf<int64_t> d_pace_last_ts;

    // cluster hot-parameter tokens
    std::vector<sg_cparam_rule> cprules;
    std::vector<CPRule> cptab;
    DevBuf<CPRule> d_cprules;
    DevBuf<sg_param_hot_item> d_cphot;
    DevBuf<uint64_t> d_cpkeys;
    DevBuf<CPBucket> d_cpring;
    uint64_t cptotal = 0;
    int cpstride = 1;
    DevBuf<int64_t> d_cplast_ts;
    // one-pipeline batch scratch (value-position records, fixed point over multi-value requests)
    DevBuf<uint32_t> d_cp_owner;
    DevBuf<uint32_t> d_cp_pslot;
    DevBuf<uint32_t> d_cp_long;       // segment lists over the value records (capacity cp_val_cap)
    DevBuf<uint32_t> d_cp_short;
    uint64_t cp_class_off[kClasses]{};
    DevBuf<uint32_t> d_p_msb;         // hot-parameter batch: first request index of each millisecond
    DevBuf<int64_t> d_p_mt;           // its first timestamp, then the millisecond count (uint32)
    DevBuf<uint16_t> d_p_mbk;         // pace: the millisecond of every kPcBuckets-th request
    std::vector<int32_t> cp_wls;      // distinct window lengths of the cluster param rules (CPRule::wl_idx)
    DevBuf<uint32_t> d_cp_bnd;        // [kMaxWl][kMaxPeriods] the batch's period tables (request index -> period)
    DevBuf<int64_t> d_cp_p0;
    DevBuf<uint32_t> d_cp_np;
    DevBuf<uint32_t> d_cp_slot_item;     // [cptotal] work item of each touched slot (k_cp_items)
    DevBuf<uint32_t> d_cp_items;      // [4 * cp_val_cap] per work item: re-walk flag, segment start; re-walk lists x2
    DevBuf<uint32_t> d_cp_counts;     // [6]: re-walk list counts (2 buffers x {long, short}), multi-value count
    DevBuf<uint32_t> d_cp_mlist;      // [max_batch] multi-value requests
    DevBuf<uint8_t> d_cp_chk;
    DevBuf<uint8_t> d_cp_assume;
    DevBuf<uint64_t> d_cp_rec;
    DevBuf<uint64_t> d_cp_rec2;
    DevBuf<uint32_t> d_cp_hist;
    uint64_t cp_val_cap = 0;          // value positions the scratch above is laid out for (cp_class_off follows it)
    DevBuf<CPBucket> d_cp_save;
    DevBuf<CPBucket> d_cp_ckpt;       // hot-slot ring checkpoints, one per window period of the batch
    DevBuf<uint2> d_cp_skips;         // saturated ranges of the hot-slot walker (k_cp_skipfill), [size()]
    DevBuf<uint32_t> d_cp_skip_count;
    DevBuf<int> d_cp_changed;
    DevBuf<uint8_t> d_cp_rule_lim;    // [cparam rules] limiter slot of the rule's namespace (0xFF none)
    std::vector<uint8_t> cp_rule_lim_host;
    bool cp_any_lim = false;          // some cluster param rule's namespace has a limiter
    uint32_t cp_rounds = 0;           // fixed-point rounds of the last batch (stats / tests)
    uint32_t cp_max_rounds = 64;      // env SG_CP_MAX_ROUNDS overrides (tests force the serial fallback)

    // param-flow wire codec: flowId → cluster param rule index, and the value dictionary (pcodec.hip)
    DevBuf<FidSlot> d_cpfid;
    uint64_t cpfid_mask = 0;
    struct VDict {
        bool on = false;
        uint64_t capacity = 0, arena_bytes = 0, max_batch = 0;
        uint64_t count = 0, arena_used = 0;   // the device state's size: every batch ends with the host knowing it
        // sg_vdict_sweep gives ids back: every id in [1, high] is live (count of them) or free, high = count + n_free
        uint64_t high = 0;                    // the largest id ever handed out
        DevBuf<uint32_t> free_ids;            // the last sweep's dead ids, ascending
        uint64_t free_head = 0, n_free = 0;   // entries batches have taken since; entries left
        DevBuf<uint64_t> tab;
        uint64_t tab_mask = 0;
        DevBuf<VEntry> entries;
        DevBuf<uint8_t> arena;
        DevBuf<VDesc> desc;                   // batch scratch, max_batch values
        DevBuf<uint64_t> hash;
        DevBuf<uint32_t> slot_of;
        DevBuf<uint32_t> dedupe;              // dedupe_slots >= 2 * max_batch
        uint64_t dedupe_slots = 0;
        DevBuf<uint64_t> scan;
        DevBuf<uint64_t> sums;                // scan workspace for max(max_batch values, cfg.max_batch frames)
        DevBuf<uint64_t> cnt;                 // [cfg.max_batch] values per frame / value_begin
        DevBuf<uint64_t> totals;              // [2] device: scan total, miss count
    } vd;

    // GatewayFlowSlot: the converted rules and the parser's tables (gateway_rules.h, gateway.hip)
    struct Gateway {
        bool on = false;
        GwConverted conv;                     // host copy: sg_gateway_converted, sg_gateway_param_rule_count
        uint64_t nm_id = 0, d_id = 0;         // "$NM", "$D"
        DevBuf<GwRes> res;
        DevBuf<GwItemRule> rules;
        DevBuf<uint8_t> patterns;
        DevBuf<uint64_t> cnt;                 // batch scratch, grown on demand: [n + 1]
        DevBuf<uint64_t> item_map;            // [n_items]
        DevBuf<uint64_t> sums;                // scan workspace for n + 1
        DevBuf<uint32_t> err;                 // [1]
    } gw;

    // Gateway API definitions and the expansion's view of the gateway rules (gateway_api.h, gateway_api.hip)
    struct GatewayApi {
        bool on = false;
        GwaTables t;                          // host copy: sg_gateway_verdict_ids
        uint32_t default_context = 0;
        DevBuf<GwaSlot> exact, bucket;
        DevBuf<uint32_t> exact_list, vid_begin, vid_apis, api_res;
        DevBuf<GwaPred> ant, wild;
        DevBuf<uint8_t> patterns;
        // per item rule of gw.conv.items, rebuilt by either load (the verdict ids) and sg_gateway_set_item_fields
        std::vector<uint32_t> item_source;    // the gateway rule behind it
        std::vector<uint32_t> vid_rule;       // verdict id - n API verdict ids → gateway rule index
        uint32_t n_rules = 0;                 // the rule count of the last sg_gateway_load_rules
        bool fields_set = false;
        DevBuf<uint32_t> item_field, item_vid;
        DevBuf<uint64_t> cnt, sums;           // batch scratch, grown on demand: 2 x [n + 1], the scan's workspace
        DevBuf<uint32_t> err;                 // [1]
    } gwa;

    // local slot chain
    sg_local_config lcfg{2, 1000, 500, 0};
    std::vector<LRule> ltab;          // [K] the resources (sg_local_load_rules), origin nodes not included
    uint32_t l_nodes = 0;             // node arrays: the resources, then the pool (l_pool_cap nodes)
    int32_t l_n_origins = 0;
    bool l_has_cx = false;
    std::vector<int64_t> l_rule_slot; // loaded flow rule i → its LCtl index, -2 stateless fast-path rule, -1 ignored
    DevBuf<LFlowRule> d_lfrules;
    DevBuf<LCtl> d_lctl;
    DevBuf<LAuth> d_lauth;            // [K] AuthoritySlot's rule of each resource, null = no authority rule kept
    DevBuf<int32_t> d_lauth_ids;      // its lists' origin ids above 64
    DevBuf<int64_t> d_llast_fetch;    // [K] StatisticNode.lastFetchTime
    DevBuf<LRule> d_lrules;
    DevBuf<LHead> d_lhead;
    DevBuf<LBucket> d_lsec;
    DevBuf<LFuture> d_lbor;
    DevBuf<LBucket> d_lmin;
    DevBuf<int64_t> d_llast_ts;
    int l_n_wl = 0, l_wsec = 0, l_wmin = 0;
    int32_t l_wl[kMaxWl]{};
    struct LocalWs {                  // the local path's own batch buffers of a pipeline workspace (0: every local
        DevBuf<int> flags;            // batch; 1: every other sg_local_enqueue batch), sized for max_batch
        DevBuf<uint32_t> exit_pos;
        DevBuf<uint32_t> exit_cnt;
        DevBuf<LSkip> skips;
        DevBuf<uint32_t> skip_count;
        DevBuf<uint64_t> pslot;       // [max_batch] LArgs::pslot (param rules loaded and the cx wave walker on)
        DevBuf<CxSide> cxside;        // [max_batch] LArgs::cxside (with pslot)
        DevBuf<uint32_t> cxw_next;    // LArgs::cxw_next
        DevBuf<uint32_t> cx_list;     // [max_batch + 1] LArgs::cx_list, then cx_count (cx resources loaded)
        DevBuf<uint8_t> auth_rej;     // [max_batch] LArgs::auth_rej (authority rules loaded)
    };
    LocalWs lws[2];
    // node pool (origin nodes, context DefaultNodes; created by the batches, kept across flow-rule reloads)
    uint32_t l_pool_cap = 0, l_pool_used = 0;
    DevBuf<uint64_t> d_lnkeys;        // map (resource, kind, id) → node, size() slots (a power of two)
    DevBuf<uint32_t> d_lnvals;
    DevBuf<uint32_t> d_lnode_new;     // pool nodes a batch created
    PinnedBuf<uint32_t> h_lnode_new;  // pinned
    DevBuf<uint2> d_lev_node;         // [max_batch] map slots of each event's nodes
    DevBuf<uint32_t> d_ldyn;          // [K] batch epoch of each resource's last origin event
    uint32_t l_epoch = 0;
    uint64_t l_batches = 0;           // local batches decided since sg_local_load_rules
    int32_t l_n_contexts = 0;
    int32_t l_cluster_state = SG_CLUSTER_NOT_STARTED;
    bool l_cluster_rules = false;     // some loaded flow rule is in cluster mode
    std::vector<uint8_t> l_base_cx;   // per resource: walked by the cx walker whatever the key groups
    std::vector<std::pair<uint32_t, uint32_t>> l_relate;        // RELATE (resource, referenced resource)
    std::vector<std::pair<uint32_t, uint32_t>> l_cluster_refs;  // cluster-mode rules: (resource, cluster_key)
    bool l_groups_stale = false;      // cluster rules / namespaces / cluster state changed: regroup before a batch
    DevBuf<uint32_t> d_lgkey;         // [K] RELATE key groups (record key of each resource), null without groups
    uint64_t l_ps_applied = 0;        // ps_gen whose param flags d_lrules carries (0: none)
    bool l_has_cx_ps = false;         // some resource is cx because of param rules
    DevBuf<uint8_t> d_linbound;       // [K] EntryType.IN resources (sg_local_set_entry_types), null = none
    std::vector<uint8_t> l_inbound;   // the same on the host (the system image's key group)
    // SystemSlot (sg_local_load_system_rules): ENTRY_NODE tracking, the thresholds, the system image
    bool l_sys_track = false;         // ENTRY_NODE is tracked (from the first system-rule load to sg_local_load_rules)
    LSysConf l_sys_conf = system_defaults();
    double l_sys_load = -1, l_sys_cpu = -1;  // SystemStatusListener's values
    DevBuf<LSys> d_lsys;              // thresholds, status, curThreadNum, scan verdict, apply scratch
    DevBuf<LBucket> d_lsys_sec;       // [S] ENTRY_NODE's second window
    DevBuf<unsigned long long> d_lsys_lastp;  // [S] LSys::lastp
    DevBuf<int64_t> d_lsys_acc;       // [S][8] LSys::acc
    DevBuf<int64_t> d_lsys_pb;        // [3][kMaxPeriods] SysArgs::pb
    DevBuf<LRule> d_lrules_sys;       // the system image: d_lrules with every inbound resource in one key group
    DevBuf<uint32_t> d_lgkey_sys;     // ... and its record keys
    bool l_sys_image = false;         // the system image is current (tracking on and some resource inbound)
    int l_sys_force = 0;              // env SG_SYS_SERIAL=1: every tracked batch takes the serial path
    uint32_t l_sys_path = 0;          // sg_local_system_last_path
    uint32_t l_sys_first = 0xFFFFFFFFu;  // the last scan's first unproven entry
    PinnedBuf<uint32_t> h_lsys_verdict;  // pinned {unproven, first_unproven}
    DevBuf<LBucket> d_lentry_acc;     // [60] the ENTRY_NODE's buckets, summed per metric call
    DevBuf<unsigned long long> d_lm_cnt;     // the metric passes' row counter
    DevBuf<int64_t> d_lentry_fetch;   // the ENTRY_NODE's lastFetchTime
    // LogSlot's rollup (sg_local_block_log_enable; null d_blog: off)
    DevBuf<BlogSlot> d_blog;          // the table, 2^blog_log2 slots; outlives every rule reload
    int32_t blog_log2 = 0;
    DevBuf<unsigned long long> d_blog_ctr;  // {lost entries, lost count, rows taken, rows kept}
    DevBuf<sg_block_row> d_blog_rows, d_blog_keep;  // [slots] the fetch's complete rows / survivors
    DevBuf<int32_t> d_blog_app;       // [max_batch] LArgs::blog_app
    DevBuf<int32_t> d_lres_app;       // [K] LArgs::res_app
    std::vector<int32_t> l_res_app;   // its host copy (blocklog_rules.h), kept whether or not the log is on
    // the token server's stat log (sg_server_log_enable; null d_slog: off)
    DevBuf<SlogSlot> d_slog;          // the table, 2^slog_log2 slots; outlives every rule reload
    int32_t slog_log2 = 0;
    DevBuf<unsigned long long> d_slog_ctr;  // {lost decisions, lost count, rows / slots taken, slots kept}
    DevBuf<SlogSlot> d_slog_rows, d_slog_keep;  // [slots] the fetch's complete slots / survivors
    DevBuf<int64_t> d_slog_fid;       // [K] SlogArgs::fid, uploaded with the rules while the log is on
    DevBuf<int64_t> d_slog_cpfid;     // [cluster param rules] SlogArgs::cpfid, the same way
    DevBuf<uint32_t> d_slog_blk;      // [max_batch] CPBatch::slog_blk, from the first cluster param batch with the log on
    DevBuf<int32_t> d_slog_rel;       // [max_batch] ConcArgs::slog_rel, from the first concurrent batch with the log on
    bool slog_rls = false;            // SlogArgs::rls: set by sg_rls_should_rate_limit for the duration of its batch

    int kbits = 0, ibits = 0, abits = 0;
    int32_t shard_rank = 0, shard_world = 1;  // sg_set_shard: this handle's share of a node's flowIds
    // sg_lim_exchange: the node's gathered per-millisecond limiter arrivals for the next flow batch of a shard
    DevBuf<uint32_t> d_xg_ws[2];         // the gathered arrivals a pipelined batch of workspace x reads (copied at enqueue)
    DevBuf<int> d_limx_err;           // sg_lim_arrivals' own error word (the pipelined batches keep theirs)
    PinnedBuf<int> h_limx_err;        // pinned
    const uint32_t* lim_xg = nullptr;
    int64_t lim_xt = 0;
    uint32_t lim_xn = 0;
    bool lim_x_armed = false;
    // ParamFlowSlot chain (sg_pslot_*)
    uint32_t ps_nres = 0;
    bool ps_loaded = false;
    DevBuf<uint32_t> d_ps_begin;
    DevBuf<uint32_t> d_ps_rules;
    DevBuf<int32_t> d_ps_grade;
    DevBuf<int32_t> d_ps_idx;
    DevBuf<int32_t> d_ps_init;
    DevBuf<PSThread> d_ps_tc;
    uint64_t ps_tc_slots = 0;
    DevBuf<int64_t> d_ps_last_ts;
    std::vector<uint32_t> ps_res_rules;  // param rules per resource
    uint64_t ps_gen = 0;              // sg_pslot_load_rules calls so far
    DevBuf<int32_t> d_ps_cmode;       // per rule: SG_CLUSTER_MODE_*
    DevBuf<uint32_t> d_ps_ckey;       // per rule: its flowId's cluster param rule index (embedded server)
    bool ps_cluster = false;          // some loaded param rule is a cluster-mode QPS rule
    std::vector<std::pair<uint32_t, uint32_t>> ps_cluster_refs;  // (resource, cluster_key) of those rules
    DevBuf<uint32_t> d_ps_gkey;       // [n_res] key groups of sg_pslot_decide_batch on an embedded server, or null
    bool ps_groups_stale = true;      // param rules / cluster param rules / namespaces / state changed
    // concurrent cluster tokens (sg_conc_*)
    DevBuf<int32_t> d_cnow;           // nowCalls per rule
    DevBuf<double> d_cthr;
    DevBuf<int64_t> d_coff;
    DevBuf<int64_t> d_cres;
    DevBuf<int64_t> d_cfid;
    DevBuf<CTok> d_ctok;
    uint64_t ctok_slots = 0, ctok_used = 0;  // table size; slots taken since the last rehash (upper bound)
    DevBuf<uint8_t> d_calive;
    DevBuf<int64_t> d_clast_ts;
    uint64_t conc_seq = 0;            // requests decided so far (token ids)
    bool conc_dirty = true;           // rules / namespaces / timeouts changed since the last upload
    bool cnow_pending = false;        // cnow_host holds the remapped counters of a rule reload
    std::vector<int32_t> cnow_host;
    std::vector<int64_t> c_off, c_res;
    // asynchronous host pipeline (sg_flow_submit): H2D / compute / D2H streams, kAsyncSlots batches in flight
    struct Slot {
        uint64_t ticket = 0;            // 0 = free
        DevBuf<sg_req> d_req;
        DevBuf<sg_result> d_out;
        PinnedBuf<int> h_err;           // pinned: the batch's error flags
        Event h2d, comp, d2h;
    };
    Slot slots[kAsyncSlots];
    Stream s_in, s_comp, s_out;
    uint64_t next_ticket = 1;
    std::unordered_map<uint64_t, int> finished;  // tickets completed while making room, not yet collected
    bool stats_on = false;
    uint32_t short_max = kShortMax;   // default walker split (env SG_SHORT_MAX overrides, for tuning)
    bool short_max_env = false;
    // lane / wave walker splits of the other walkers, read once in sg_create (tuning)
    uint32_t param_short_max = 64;    // hot-parameter walkers (env SG_PARAM_SHORT_MAX; r04: 64 < 32 by 2%)
    uint32_t pace_short_max = 128;    // pace walkers (env SG_PACE_SHORT_MAX; 1M rules, 16M canPass: 32 → 1.31,
                                      // 64 → 1.24, 96..256 → 1.21-1.22, 512 → 1.34 ms/step)
    uint32_t cparam_short_max = 64;   // cluster param walkers (env SG_CPARAM_SHORT_MAX; r04: 64 < 32 by 5%)
    int dbg = 0;                      // env SG_DEBUG: see BatchArgs::dbg
    int l_cxw = 1;                    // env SG_CXW=0: long cx segments on the lane walker too (LArgs::cxw)
    uint32_t l_cxw_min = 0xFFFFFFFFu;          // env SG_CXW_MIN: shortest cx segment class the wave walker takes (LArgs::cxw_cls)
    bool wide_seen = false;           // some loaded rule allowed bucket counts >= 2^30 (sticky: the ring keeps them)
    Event ev[5];
    sg_batch_stats stats{};
    Stream aux;        // second stream: the long-segment walker runs beside the short one
    Event fork, join;
    // Pipelined flow batches (sg_flow_enqueue, sg_flow_submit): the front half of a batch (validation, sort,
    // segments) runs on s_front while the previous batch's walkers run on s_back. The workspaces ws[0] / ws[1] alternate.
    Stream s_front, s_back, s_aux2;
    Stream s_xcopy;    // the sharded limiter exchange's copy into a pipeline workspace
    Event xcopy_done;
    Event front_done[2], back_done[2], pfork, pjoin;
    Event lm_in, lm_done;  // sg_local_metrics_raw_enqueue: the caller's stream <-> s_back
    DevBuf<int> d_lm_gate;                           // its capacity gate (count <= cap)
    uint64_t pipe_seq = 0;            // batches put on the pipeline so far (workspace = seq % 2)
    int front_sixteenths = 8;         // CU partition of the pipeline streams (pipe_setup; round 6: the binned front half
                                      // (k_bin_sort) takes 4/8, -2.5 % against 3/8; the two-pass sort measures the same at 3 or 4)
    bool rec4 = true;                 // env SG_REC4=0: 8-byte front records on the binned path too (BatchArgs::rec4)
    int walk_cus = 0;                 // CUs of the walkers' streams when partitioned (0 = all)
    struct DevTicket {                // sg_flow_enqueue batches in flight
        uint64_t ticket = 0;
        PinnedBuf<int> h_err;         // pinned
        Event done;
        bool local = false;           // an sg_local_enqueue batch (its error flags map through local_status)
    };
    DevTicket dev[kDevSlots];
    bool front_only = false;          // a node handle's front (validation + namespace limiter): no flow state
};

namespace {
PSArgs pslot_args(sg_handle* h);          // below: the ParamFlowSlot state's device arguments
int pslot_embed(sg_handle* h, PSArgs& s, hipStream_t stream);  // below: its embedded token server (SERVER)
int ensure_layout(sg_handle* h);          // below: record layout of the loaded rules
int flow_status(sg_handle* h, int err);   // below: batch error flags -> SG_E_*
int drain_async(sg_handle* h);  // below: completes the handle's in-flight host-pipeline batches
int local_apply_groups(sg_handle* h);  // below: key groups of the local chain
int local_sys_image(sg_handle* h);     // below: SystemSlot's rule image (after any change of the normal one)
void local_sys_drop(sg_handle* h);
}

extern "C" {
static int upload_fid_table(sg_handle* h);  // flowId → rule index for the wire codec (defined below)
static int upload_cp_fid_table(sg_handle* h, const sg_cparam_rule* rules, uint32_t n);  // the same for param rules
}

namespace {

int fail(sg_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                        \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail((h), SG_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(_e));     \
    } while (0)

// A _host entry point after its argument checks, for a handle or a node `o` (device: where its staging lives):
// n requests up, call(d_req, d_out) on the staged copies, n results down.
template <class O, class Req, class Out, class Call>
int host_batch(O* o, int device, const Req* req, uint64_t n, Out* out, Call call) {
    auto bad = [&](int code, const std::string& msg) {
        o->err = msg;
        return code;
    };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bad(SG_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    Req* d_req = nullptr;
    Out* d_out = nullptr;
    if (!o->stage.get(0, o->cfg.max_batch, d_req) || !o->stage.get(1, o->cfg.max_batch, d_out))
        return bad(SG_E_NOMEM, "host-path buffers");
    e = hipMemcpy(d_req, req, sizeof(Req) * n, hipMemcpyHostToDevice);
    if (e != hipSuccess) return bad(SG_E_DEVICE, std::string("host-path upload: ") + hipGetErrorString(e));
    const int rc = call(d_req, d_out);
    if (rc) return rc;
    e = hipMemcpy(out, d_out, sizeof(Out) * n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return bad(SG_E_DEVICE, std::string("host-path download: ") + hipGetErrorString(e));
    return SG_OK;
}

int bits_for(uint64_t v) {  // bits needed to represent v (v >= 1)
    int b = 0;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

// calcGlobalThreshold(rule) * exceedCount (ClusterFlowChecker.java:38-48, :68)
double global_threshold(const sg_handle* h, const sg_flow_rule& r) {
    double base;
    if (r.threshold_type == SG_THRESHOLD_GLOBAL) {
        base = r.count;
    } else {
        int connected = 0;
        if (r.namespace_id >= 0 && (size_t)r.namespace_id < h->ns.size()) connected = h->ns[r.namespace_id].connected_count;
        base = r.count * connected;
    }
    return base * h->cfg.exceed_count;
}


int layout_records(sg_handle* h) {
    h->kbits = bits_for((uint64_t)h->K);  // must hold K itself (sentinel key of rejected requests)
    if (h->kbits < 1) h->kbits = 1;
    h->ibits = bits_for(h->cfg.max_batch > 1 ? h->cfg.max_batch - 1 : 1);
    // acquire field: 7 bits + prio (larger acquireCounts escape to the request), so that {idx, acode} fit the
    // low 32 bits whenever ibits <= 24 (the short walker's compact LDS records)
    h->abits = std::min(8, 64 - h->kbits - h->ibits);
    if (h->abits < 3) return fail(h, SG_E_UNSUPPORTED, "rule count x max_batch too large for 64-bit records");
    return SG_OK;
}

// Distinct window lengths of the loaded flows (+ the limiter's 100 ms when a limiter is on).
int rebuild_wl_table(sg_handle* h) {
    int n_wl = 0;
    int32_t wl[kMaxWl]{};
    auto index_of = [&](int32_t v) -> int {
        for (int w = 0; w < n_wl; ++w)
            if (wl[w] == v) return w;
        if (n_wl == kMaxWl) return -1;
        wl[n_wl] = v;
        return n_wl++;
    };
    for (uint32_t k = 0; k < h->K; ++k) {
        const int w = index_of(h->rule_tab[k].wl);
        if (w < 0) return fail(h, SG_E_UNSUPPORTED, "more than 8 distinct window lengths");
        h->rule_tab[k].wl_idx = w;
    }
    h->lim_wl_idx = -1;
    if (h->n_lim > 0) {
        h->lim_wl_idx = index_of(kLimWindowMs);
        if (h->lim_wl_idx < 0) return fail(h, SG_E_UNSUPPORTED, "more than 8 distinct window lengths");
    }
    h->n_wl = n_wl;
    std::memcpy(h->wl, wl, sizeof(wl));
    return SG_OK;
}

int upload_rule_table(sg_handle* h) {
    h->l_groups_stale = true;  // an embedded token server's key groups follow the cluster rules / namespaces
    h->ps_groups_stale = true;
    int rc = rebuild_wl_table(h);
    if (rc) return rc;
    // Bucket counts stay below thr * (2 + isec) * (2 + maxOccupyRatio): a pass needs PASS sum <= thr * isec,
    // an occupy acquire + occupied <= thr + head and WAITING sum <= ratio * thr * isec before it adds acquire.
    // Below 2^30 the short walker may hold PASS / WAITING in int32 (BatchArgs::narrow).
    const double ratio = h->cfg.max_occupy_ratio > 0 ? h->cfg.max_occupy_ratio : 0.0;
    for (uint32_t k = 0; k < h->K; ++k) {
        Rule& R = h->rule_tab[k];
        R.thr = global_threshold(h, h->rules[k]);
        const double bound = (R.thr > 0 ? R.thr : 0.0) * (2.0 + R.isec) * (2.0 + ratio);
        if (!(bound < 1073741824.0)) h->wide_seen = true;
    }
    if (h->K) HIP_TRY(h, hipMemcpy(h->d_rules, h->rule_tab.data(), sizeof(Rule) * h->K, hipMemcpyHostToDevice));
    // limiter slot of each rule's namespace
    h->d_rule_lim.reset();
    if (h->K) {
        std::vector<uint8_t> rl(h->K, 0xFF);
        for (uint32_t k = 0; k < h->K; ++k) {
            const int ns = h->rules[k].namespace_id;
            if (ns >= 0 && (size_t)ns < h->ns_slot.size() && h->ns_slot[ns] >= 0) rl[k] = (uint8_t)h->ns_slot[ns];
        }
        if (!h->d_rule_lim.alloc_bytes(h->K)) return fail(h, SG_E_NOMEM, "rule limiter table");
        HIP_TRY(h, hipMemcpy(h->d_rule_lim, rl.data(), h->K, hipMemcpyHostToDevice));
    }
    return SG_OK;
}

// A flow workspace's batch buffers for cfg.max_batch requests (class_off set): everything but seg_end, which follows
// the loaded rules (flow_seg_alloc), and bin_buf (bin_setup, on the first binned batch).
bool flow_ws_alloc(sg_handle* h, sg_handle::FlowWs& w) {
    const uint64_t n = h->cfg.max_batch;
    const uint64_t short_words = h->class_off[kClasses - 1] + n / (kClassMax[kClasses - 2] + 1) + 1;
    // + kRecW records of slack: the short walker stages record windows past a segment's end unclamped
    return w.rec.alloc(n + kRecW) && w.rec_sorted.alloc(n + kRecW) && w.hist.alloc(radix_hist_words(n)) &&
           w.bnd.alloc((size_t)kMaxWl * kMaxPeriods) && w.p0.alloc(kMaxWl) && w.np.alloc(kMaxWl) && w.err.alloc(1) &&
           w.long_list.alloc(n + 1) && w.long_key.alloc(n + 1) && w.long_end.alloc(n + 1) &&
           w.long_pend.alloc((size_t)kLongTab * kLongPeriods) && w.short_list.alloc(short_words) &&
           w.short_key.alloc(short_words) && w.short_end.alloc(short_words) && w.counts.alloc(1 + kClasses) &&
           w.skips.alloc(2 * n / kSkipMin + 1) && w.skip_count.alloc(1);
}

// Segment marks for K flowIds: [K + 1] ends (none marked: 0), then [K + 1] starts (none marked: 0xFFFFFFFF).
int flow_seg_alloc(sg_handle* h, DevBuf<uint32_t>& seg, uint32_t K) {
    const size_t cap = (size_t)K + 1;
    if (!seg.alloc(2 * cap)) return fail(h, SG_E_NOMEM, "segment marks");
    HIP_TRY(h, hipMemset(seg, 0, sizeof(uint32_t) * cap));
    HIP_TRY(h, hipMemset(seg + cap, 0xFF, sizeof(uint32_t) * cap));
    return SG_OK;
}

// A device copy of v (one element at least, so that no table pointer is null).
template <class T>
static bool gwa_upload(DevBuf<T>& d, const std::vector<T>& v) {
    if (!d.alloc(v.empty() ? 1 : v.size())) return false;
    return v.empty() || hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) == hipSuccess;
}

// The gateway rules' verdict ids behind those of the API predicates: after either load. The rules' tables are in
// force by then; a failure here leaves the expansion refusing (fields unset, no ids) until the next load.
static int gwa_renumber(sg_handle* h) {
    auto& a = h->gwa;
    if (!h->gw.on) return SG_OK;
    const std::vector<uint32_t> vid =
        gwa_item_vids(h->gw.conv, a.item_source, a.on ? (uint32_t)a.t.vid_pred.size() : 0u, a.vid_rule);
    if (!gwa_upload(a.item_vid, vid)) return fail(h, SG_E_NOMEM, "gateway verdict ids");
    if (!a.fields_set && !gwa_upload(a.item_field, std::vector<uint32_t>(vid.size(), 0u)))
        return fail(h, SG_E_NOMEM, "gateway item fields");
    return SG_OK;
}

}  // namespace

extern "C" {

const char* sg_build_info(void) {
    return "sentinel_gpu: cluster flow-decision engine, HIP for gfx950 (MI355X)";
}

int sg_create(const sg_config* cfg, sg_handle** out) {
    if (!cfg || !out) return SG_E_INVAL;
    *out = nullptr;
    if (cfg->max_batch == 0 || cfg->max_batch > (1ull << 32)) return SG_E_INVAL;
    if (!(cfg->exceed_count >= 0) || !(cfg->max_occupy_ratio >= 0)) return SG_E_INVAL;
    sg_handle* h = new sg_handle();
    h->cfg = *cfg;
    h->device = cfg->device;
    auto bail = [&](int rc) {
        delete h;
        return rc;
    };
    if (hipSetDevice(h->device) != hipSuccess) return bail(SG_E_DEVICE);
    const uint64_t n = cfg->max_batch;
    {  // short-segment class slices: class c holds segments longer than kClassMax[c-1], so at most n/(that+1)
        uint64_t off = 0;
        for (int c = 0; c < kClasses; ++c) {
            h->class_off[c] = off;
            off += (c == 0 ? n : n / (kClassMax[c - 1] + 1)) + 1;
        }
    }
    if (!flow_ws_alloc(h, h->ws[0])) return bail(SG_E_NOMEM);
    {
        const uint64_t tiles = n / 4096 + 1;
        if (!h->d_lim_ring.alloc(kMaxLim) || !h->d_lim_slot.alloc(n) || !h->d_lim_tile.alloc(tiles * kMaxLim * 2) ||
            !h->d_lim_period.alloc((size_t)kMaxLim * kMaxPeriods * 3))
            return bail(SG_E_NOMEM);
    }
    if (!h->d_last_ts.alloc(2)) return bail(SG_E_NOMEM);  // + front_ts
    if (!h->d_dbg.alloc(128) || hipMemset(h->d_dbg, 0, 128 * 8) != hipSuccess) return bail(SG_E_NOMEM);
    if (!h->h_err.alloc_bytes(sizeof(int))) return bail(SG_E_NOMEM);
    if (!h->h_long.alloc_bytes(2 * sizeof(uint32_t))) return bail(SG_E_NOMEM);
    int64_t neg = -1;
    if (hipMemcpy(h->d_last_ts, &neg, sizeof(neg), hipMemcpyHostToDevice) != hipSuccess) return bail(SG_E_DEVICE);
    h->d_front_ts = h->d_last_ts + 1;
    if (hipMemcpy(h->d_front_ts, &neg, sizeof(neg), hipMemcpyHostToDevice) != hipSuccess) return bail(SG_E_DEVICE);
    if (!h->d_plast_ts.alloc_bytes(sizeof(int64_t))) return bail(SG_E_NOMEM);
    if (hipMemcpy(h->d_plast_ts, &neg, sizeof(neg), hipMemcpyHostToDevice) != hipSuccess) return bail(SG_E_DEVICE);
    for (auto& e : h->ev)
        if (hipEventCreate(e.put()) != hipSuccess) return bail(SG_E_DEVICE);
    // the auxiliary stream carries the wave walkers beside the lane walkers (pace, hot params, cluster params)
    if (hipStreamCreateWithPriority(h->aux.put(), hipStreamNonBlocking, 0) != hipSuccess ||
        hipEventCreateWithFlags(h->fork.put(), hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(h->join.put(), hipEventDisableTiming) != hipSuccess)
        return bail(SG_E_DEVICE);
    if (const char* d = std::getenv("SG_DEBUG")) h->dbg = std::atoi(d);
    if (const char* d = std::getenv("SG_CXW")) h->l_cxw = std::atoi(d) != 0 ? 1 : 0;
    if (const char* d = std::getenv("SG_SYS_SERIAL")) h->l_sys_force = std::atoi(d) != 0 ? 1 : 0;
    if (const char* d = std::getenv("SG_CXW_MIN")) h->l_cxw_min = (uint32_t)std::strtoul(d, nullptr, 10);
    if (const char* d = std::getenv("SG_BIN")) h->bin_mode = std::atoi(d);
    if (const char* d = std::getenv("SG_FRONT_SIXTEENTHS")) h->front_sixteenths = std::atoi(d);
    if (const char* d = std::getenv("SG_REC4")) h->rec4 = std::atoi(d) != 0;
    if (const char* d = std::getenv("SG_PREP_TILES")) h->prep_tiles = std::max(1, std::min(64, std::atoi(d)));
    if (const char* sm = std::getenv("SG_SHORT_MAX")) {
        h->short_max = (uint32_t)std::strtoul(sm, nullptr, 10);
        h->short_max_env = true;
    }
    if (const char* d = std::getenv("SG_PARAM_SHORT_MAX")) h->param_short_max = (uint32_t)std::strtoul(d, nullptr, 10);
    if (const char* d = std::getenv("SG_PACE_SHORT_MAX")) h->pace_short_max = (uint32_t)std::strtoul(d, nullptr, 10);
    if (const char* d = std::getenv("SG_CPARAM_SHORT_MAX")) h->cparam_short_max = (uint32_t)std::strtoul(d, nullptr, 10);
    if (const char* mr = std::getenv("SG_CP_MAX_ROUNDS")) h->cp_max_rounds = (uint32_t)std::strtoul(mr, nullptr, 10);
    // default namespace 0, no limiter, 1 connection
    sg_namespace d0{0, 1, 30000.0};
    h->ns.push_back(d0);
    *out = h;
    return SG_OK;
}

void sg_destroy(sg_handle* h) { delete h; }

const char* sg_last_error(const sg_handle* h) { return h ? h->err.c_str() : "null handle"; }

int sg_set_shard(sg_handle* h, int32_t rank, int32_t world) {
    if (h) drain_async(h);
    if (!h || world < 1 || rank < 0 || rank >= world) return SG_E_INVAL;
    h->shard_rank = rank;
    h->shard_world = world;
    return SG_OK;
}

int sg_lim_slots(const sg_handle* h, uint32_t* n_lim) {
    if (!h || !n_lim) return SG_E_INVAL;
    *n_lim = (uint32_t)h->n_lim;
    return SG_OK;
}

int sg_lim_arrivals(sg_handle* h, const sg_req* req, uint64_t n, int64_t t_base, uint32_t n_ms, uint32_t* counts_out,
                    uint64_t counts_words, void* stream_) {
    if (!h || (!req && n) || !counts_out) return SG_E_INVAL;
    if (t_base < 0 || n_ms == 0 || n_ms > kMaxPeriods) return fail(h, SG_E_INVAL, "exchange range: t_base >= 0, 1 <= n_ms <= 65536");
    if (counts_words != (uint64_t)h->n_lim * n_ms)
        return fail(h, SG_E_INVAL, "counts buffer must hold n_lim * n_ms words (sg_lim_slots)");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipSetDevice(h->device));
    // reads only the request batch and the rule → limiter table: batches in flight on the pipeline go on
    int rc = ensure_layout(h);
    if (rc) return rc;
    if (!h->d_limx_err && (!h->d_limx_err.alloc_bytes(sizeof(int)) ||
                           !h->h_limx_err.alloc_bytes(sizeof(int))))
        return fail(h, SG_E_NOMEM, "exchange error word");
    HIP_TRY(h, hipMemsetAsync(counts_out, 0, sizeof(uint32_t) * (size_t)h->n_lim * n_ms, stream));
    HIP_TRY(h, hipMemsetAsync(h->d_limx_err, 0, sizeof(int), stream));
    if (h->n_lim > 0)
        HIP_TRY(h, launch_lim_arrivals(req, n, h->K, h->d_rule_lim, t_base, n_ms, counts_out, h->d_limx_err, stream));
    HIP_TRY(h, hipMemcpyAsync(h->h_limx_err, h->d_limx_err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return flow_status(h, *h->h_limx_err);
}

namespace {
int cp_rule_limiters(sg_handle* h, hipStream_t stream);
}

int sg_lim_arrivals_param(sg_handle* h, const sg_cparam_req* req, uint64_t n, int64_t t_base, uint32_t n_ms,
                          uint32_t* counts_out, uint64_t counts_words, void* stream_) {
    if (!h || (!req && n) || !counts_out) return SG_E_INVAL;
    if (t_base < 0 || n_ms == 0 || n_ms > kMaxPeriods) return fail(h, SG_E_INVAL, "exchange range: t_base >= 0, 1 <= n_ms <= 65536");
    if (counts_words != (uint64_t)h->n_lim * n_ms)
        return fail(h, SG_E_INVAL, "counts buffer must hold n_lim * n_ms words (sg_lim_slots)");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = cp_rule_limiters(h, stream);
    if (rc) return rc;
    if (!h->d_limx_err && (!h->d_limx_err.alloc_bytes(sizeof(int)) ||
                           !h->h_limx_err.alloc_bytes(sizeof(int))))
        return fail(h, SG_E_NOMEM, "exchange error word");
    HIP_TRY(h, hipMemsetAsync(counts_out, 0, sizeof(uint32_t) * (size_t)h->n_lim * n_ms, stream));
    HIP_TRY(h, hipMemsetAsync(h->d_limx_err, 0, sizeof(int), stream));
    if (h->n_lim > 0 && h->d_cp_rule_lim)
        HIP_TRY(h, launch_lim_arrivals_param(req, n, (uint32_t)h->cprules.size(), h->d_cp_rule_lim, t_base, n_ms,
                                             counts_out, h->d_limx_err, stream));
    HIP_TRY(h, hipMemcpyAsync(h->h_limx_err, h->d_limx_err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return flow_status(h, *h->h_limx_err);
}

int sg_lim_exchange(sg_handle* h, const uint32_t* gathered, uint64_t gathered_words, int64_t t_base, uint32_t n_ms) {
    if (!h || !gathered) return SG_E_INVAL;
    if (t_base < 0 || n_ms == 0 || n_ms > kMaxPeriods) return fail(h, SG_E_INVAL, "exchange range: t_base >= 0, 1 <= n_ms <= 65536");
    if (gathered_words != (uint64_t)h->shard_world * (uint64_t)h->n_lim * n_ms)
        return fail(h, SG_E_INVAL, "gathered buffer must hold world * n_lim * n_ms words (sg_lim_slots)");
    h->lim_xg = gathered;
    h->lim_xt = t_base;
    h->lim_xn = n_ms;
    h->lim_x_armed = true;
    return SG_OK;
}

int sg_set_namespaces(sg_handle* h, const sg_namespace* ns, uint32_t n) {
    if (!h || (!ns && n)) return SG_E_INVAL;
    int want = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (ns[i].limiter_enabled) {
            if (!(ns[i].max_allowed_qps >= 0)) return fail(h, SG_E_INVAL, "max allowed QPS should >= 0");
            ++want;
        }
    }
    if (want > kMaxLim) return fail(h, SG_E_UNSUPPORTED, "more than 8 namespaces with a QPS limiter");
    h->conc_dirty = true;  // AVG_LOCAL concurrency thresholds read connectedCount
    for (const auto& r : h->rules)
        if (r.namespace_id < 0 || (uint32_t)r.namespace_id >= n)
            return fail(h, SG_E_INVAL, "a loaded rule refers to a namespace that would disappear");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    // A namespace that keeps its limiter keeps its window (GlobalRequestLimiter.initIfAbsent :32-37,
    // applyMaxQpsChange :73-80); a newly enabled one starts empty.
    LimRing old[kMaxLim], nw[kMaxLim];
    if (h->n_lim) HIP_TRY(h, hipMemcpy(old, h->d_lim_ring, sizeof(LimRing) * kMaxLim, hipMemcpyDeviceToHost));
    std::vector<int> slot(n, -1);
    int n_lim = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!ns[i].limiter_enabled) continue;
        const int s_new = n_lim++;
        slot[i] = s_new;
        h->lim_qps[s_new] = ns[i].max_allowed_qps;
        const int s_old = (i < h->ns_slot.size()) ? h->ns_slot[i] : -1;
        if (s_old >= 0) {
            nw[s_new] = old[s_old];
        } else {
            for (int j = 0; j < kLimSamples; ++j) {
                nw[s_new].start[j] = INT64_MIN;
                nw[s_new].count[j] = 0;
            }
        }
    }
    if (n_lim) HIP_TRY(h, hipMemcpy(h->d_lim_ring, nw, sizeof(LimRing) * n_lim, hipMemcpyHostToDevice));
    h->ns.assign(ns, ns + n);
    h->ns_slot = slot;
    h->n_lim = n_lim;
    if (!h->cptab.empty()) {  // AVG_LOCAL param thresholds follow the connected counts
        for (size_t i = 0; i < h->cptab.size(); ++i) {
            const int nsi = h->cprules[i].namespace_id;
            h->cptab[i].connected = (nsi >= 0 && (uint32_t)nsi < n) ? ns[nsi].connected_count : 0;
        }
        HIP_TRY(h, hipMemcpy(h->d_cprules, h->cptab.data(), sizeof(CPRule) * h->cptab.size(), hipMemcpyHostToDevice));
    }
    return upload_rule_table(h);
}

namespace {

// The stat log's flowId of every flow rule (SlogArgs::fid), uploaded when the log is enabled and with every rule load
// while it is on. The caller has drained the pipelines: no batch in flight reads the array it replaces.
int slog_sync_fids(sg_handle* h) {
    if (!h->d_slog) return SG_OK;
    std::vector<int64_t> fid(std::max<uint32_t>(h->K, 1u), 0);
    for (uint32_t k = 0; k < h->K; ++k) fid[k] = h->rules[k].flow_id;
    std::vector<int64_t> cpfid(std::max<size_t>(h->cprules.size(), 1), 0);
    for (size_t k = 0; k < h->cprules.size(); ++k) cpfid[k] = h->cprules[k].flow_id;
    DevBuf<int64_t> d, dc;  // both built before either replaces the live one: a failure leaves the pair as it was
    if (!d.alloc(fid.size()) || !dc.alloc(cpfid.size())) return fail(h, SG_E_NOMEM, "server log flowIds");
    HIP_TRY(h, hipMemcpy(d, fid.data(), sizeof(int64_t) * fid.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(dc, cpfid.data(), sizeof(int64_t) * cpfid.size(), hipMemcpyHostToDevice));
    h->d_slog_fid = std::move(d);
    h->d_slog_cpfid = std::move(dc);
    return SG_OK;
}

SlogArgs slog_args(sg_handle* h) {
    SlogArgs s{};
    s.tab = h->d_slog;
    s.mask = h->d_slog.size() - 1;
    s.lost = h->d_slog_ctr;
    s.fid = h->d_slog_fid;
    s.cpfid = h->d_slog_cpfid;
    s.rls = h->slog_rls ? 1 : 0;
    return s;
}

// The stat log's add for the decided flow batch a (flow_back, a node shard's back half): behind launch_skip_apply,
// where the results of the wave walker's skipped ranges exist, and before the workspace's next user.
int slog_add_flow(sg_handle* h, const BatchArgs& a, hipStream_t stream, uint64_t n_req = 0) {
    SlogArgs s = slog_args(h);
    s.n_req = n_req;
    s.drop = a.rec4 ? a.bin_tot + kBinDrop : nullptr;
    HIP_TRY(h, launch_slog_add_flow(a, s, stream));
    return SG_OK;
}

}  // namespace

namespace {

// Every check sg_load_flow_rules makes before it changes anything (FlowRuleUtil.isValidRule / checkClusterField,
// FlowRuleUtil.java:167-229, and the device path's limits: sampleCount <= 64 for a surviving metric's window shape
// too, <= 8 distinct window lengths with the limiter's 100 ms): after SG_OK only allocation or device errors remain.
int flow_rules_validate(sg_handle* h, const sg_flow_rule* rules, uint32_t n) {
    if (n >= SG_KEY_BAD) return fail(h, SG_E_INVAL, "too many rules");
    std::unordered_map<int64_t, uint32_t> seen, old_index;
    for (uint32_t k = 0; k < h->K; ++k) old_index.emplace(h->rules[k].flow_id, k);
    std::vector<int32_t> wls;
    for (uint32_t i = 0; i < n; ++i) {
        const sg_flow_rule& r = rules[i];
        if (r.flow_id <= 0) return fail(h, SG_E_INVAL, "flowId must be > 0");
        if (!(r.count >= 0)) return fail(h, SG_E_INVAL, "count must be >= 0");
        if (r.sample_count <= 0 || r.window_interval_ms <= 0 || r.window_interval_ms % r.sample_count != 0)
            return fail(h, SG_E_INVAL, "invalid window config");
        if (r.namespace_id < 0 || (size_t)r.namespace_id >= h->ns.size())
            return fail(h, SG_E_INVAL, "unknown namespace");
        if (!seen.emplace(r.flow_id, i).second) return fail(h, SG_E_INVAL, "duplicate flowId");
        int S = r.sample_count, wl = r.window_interval_ms / r.sample_count;
        auto it = old_index.find(r.flow_id);
        if (it != old_index.end()) {
            S = h->rule_tab[it->second].S;
            wl = h->rule_tab[it->second].wl;
        }
        if (S > SG_MAX_SAMPLE_COUNT) return fail(h, SG_E_UNSUPPORTED, "sampleCount > 64 is not supported by the device path");
        if (std::find(wls.begin(), wls.end(), wl) == wls.end()) wls.push_back(wl);
    }
    if (h->n_lim > 0 && std::find(wls.begin(), wls.end(), (int32_t)kLimWindowMs) == wls.end()) wls.push_back(kLimWindowMs);
    if (wls.size() > (size_t)kMaxWl) return fail(h, SG_E_UNSUPPORTED, "more than 8 distinct window lengths");
    return SG_OK;
}

}  // namespace

namespace {

// The new rule set's device state, built beside the live one (which it only reads: surviving flowIds' rings and
// occupy counters are copied over), so that a failure leaves the handle as it was; flow_rules_commit swaps it in,
// flow_rules_abort frees it. The node handle prepares every shard before it commits any.
struct FlowLoad {
    std::vector<Rule> tab;
    std::vector<int32_t> src;
    int stride = 1;
    int n_wl = 0;
    int32_t wl[kMaxWl]{};
    DevBuf<Rule> d_rules;
    DevBuf<Bucket> d_ring;
    DevBuf<BucketHot> d_hot;
    DevBuf<Occ> d_occ;
    DevBuf<uint32_t> d_seg_end;       // flow_seg_alloc for the new rules: workspace 0's
};

void flow_rules_abort(FlowLoad& L) { L = FlowLoad{}; }  // under the device that prepared it

int flow_rules_prepare_impl(sg_handle* h, const sg_flow_rule* rules, uint32_t n, FlowLoad& L) {
    // old flowId → old index, to keep the metric of surviving flows (ClusterFlowRuleManager.java:361)
    std::unordered_map<int64_t, uint32_t> old_index;
    for (uint32_t k = 0; k < h->K; ++k) old_index.emplace(h->rules[k].flow_id, k);

    L.tab.assign(n, Rule{});
    L.src.assign(n, -1);
    std::vector<Rule>& tab = L.tab;
    std::vector<int32_t>& src = L.src;
    int& stride = L.stride;
    int& n_wl = L.n_wl;
    int32_t* wl = L.wl;
    for (uint32_t i = 0; i < n; ++i) {
        int S = rules[i].sample_count, interval = rules[i].window_interval_ms;
        auto it = old_index.find(rules[i].flow_id);
        if (it != old_index.end()) {  // the existing ClusterMetric keeps its window shape
            src[i] = (int32_t)it->second;
            S = h->rule_tab[it->second].S;
            interval = h->rule_tab[it->second].S * h->rule_tab[it->second].wl;
        }
        if (S > SG_MAX_SAMPLE_COUNT)
            return fail(h, SG_E_UNSUPPORTED, "sampleCount > 64 is not supported by the device path");
        Rule R{};
        R.S = S;
        R.wl = interval / S;
        R.isec = interval / 1000.0;
        R.wait_ms = 1000 / S;
        int w = 0;
        while (w < n_wl && wl[w] != R.wl) ++w;
        if (w == n_wl) {
            if (n_wl == kMaxWl) return fail(h, SG_E_UNSUPPORTED, "more than 8 distinct window lengths");
            wl[n_wl++] = R.wl;
        }
        R.wl_idx = w;  // final indices come from rebuild_wl_table (adds the limiter's 100 ms)
        stride = std::max(stride, S);
        tab[i] = R;
    }

    if (n && h->front_only) {  // a node's front: rule thresholds and limiter slots only
        if (!L.d_rules.alloc(n)) return fail(h, SG_E_NOMEM, "rule table");
    } else if (n) {
        DevBuf<int32_t> d_src;
        if (!L.d_rules.alloc(n) || !L.d_ring.alloc((size_t)n * stride) || !L.d_hot.alloc((size_t)n * stride) ||
            !L.d_occ.alloc(n) || !d_src.alloc(n))
            return fail(h, SG_E_NOMEM, "rule state allocation failed");
        const int rc = flow_seg_alloc(h, L.d_seg_end, n);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpy(d_src, src.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, launch_init_state(L.d_ring, L.d_occ, n, stride, d_src, h->d_ring, h->d_occ, h->stride, 0));
        HIP_TRY(h, launch_hot_sync(L.d_ring, L.d_hot, (uint64_t)n * stride, 0));
        HIP_TRY(h, hipDeviceSynchronize());
    }
    return SG_OK;
}

int flow_rules_prepare(sg_handle* h, const sg_flow_rule* rules, uint32_t n, FlowLoad& L) {
    const int rc = flow_rules_prepare_impl(h, rules, n, L);
    if (rc) flow_rules_abort(L);
    return rc;
}

int flow_rules_commit(sg_handle* h, const sg_flow_rule* rules, uint32_t n, FlowLoad& L) {
    std::vector<int32_t>& src = L.src;
    if (h->d_cnow) {  // CurrentConcurrencyManager: surviving flowIds keep nowCalls, new ones start at 0
        // the counters in the current rule order: a reload not yet uploaded (cnow_pending) already holds them
        // remapped to h->K / h->rules; d_cnow is still in the order of the rules before that reload
        std::vector<int32_t> old(h->K, 0);
        if (h->cnow_pending) {
            for (uint32_t k = 0; k < h->K && k < h->cnow_host.size(); ++k) old[k] = h->cnow_host[k];
        } else if (h->K) {
            HIP_TRY(h, hipMemcpy(old.data(), h->d_cnow, sizeof(int32_t) * h->K, hipMemcpyDeviceToHost));
        }
        h->cnow_host.assign(n, 0);
        for (uint32_t i = 0; i < n; ++i)
            if (src[i] >= 0) h->cnow_host[i] = old[src[i]];
        h->cnow_pending = true;
    }
    h->c_off.assign(n, 2000);  // ClusterFlowConfig.clientOfflineTime / resourceTimeout defaults
    h->c_res.assign(n, 2000);
    h->conc_dirty = true;
    h->d_rules = std::move(L.d_rules);
    h->d_ring = std::move(L.d_ring);
    h->d_hot = std::move(L.d_hot);
    h->d_occ = std::move(L.d_occ);
    sg_handle::FlowWs& w = h->ws[0];
    w.seg_end = std::move(L.d_seg_end);  // null without rules and on a node's front
    w.seg_cap = w.seg_end ? n + 1 : 0;
    w.seg_start = w.seg_end ? w.seg_end + w.seg_cap : nullptr;
    h->rules.assign(rules, rules + n);
    h->rule_tab = L.tab;
    h->K = n;
    ++h->rules_gen;
    h->stride = L.stride;
    h->n_wl = L.n_wl;
    std::memcpy(h->wl, L.wl, sizeof(L.wl));
    int rc = layout_records(h);
    if (rc) return rc;
    rc = upload_fid_table(h);
    if (rc) return rc;
    rc = slog_sync_fids(h);
    if (rc) return rc;
    return upload_rule_table(h);
}

}  // namespace

int sg_load_flow_rules(sg_handle* h, const sg_flow_rule* rules, uint32_t n) {
    if (h) drain_async(h);
    if (!h || (!rules && n)) return SG_E_INVAL;
    (void)hipSetDevice(h->device);
    const int vrc = flow_rules_validate(h, rules, n);
    if (vrc) return vrc;
    FlowLoad L;
    const int rc = flow_rules_prepare(h, rules, n, L);
    if (rc) return rc;
    return flow_rules_commit(h, rules, n, L);
}

// flowId → rule index for the wire codec: open addressing, linear probing, load factor <= 1/2 (the same
// splitmix64 finaliser as codec.hip's fid_hash). flowIds are > 0 and unique (validated above).
static uint64_t host_fid_hash(int64_t fid) { return mix64((uint64_t)fid); }

static int upload_fid_table(sg_handle* h) {
    uint64_t cap = 2;
    while (cap < 2ull * h->K) cap <<= 1;
    std::vector<FidSlot> tab(cap, FidSlot{0, 0, 0});
    for (uint32_t k = 0; k < h->K; ++k) {
        const int64_t fid = h->rules[k].flow_id;
        uint64_t p = host_fid_hash(fid) & (cap - 1);
        while (tab[p].fid != 0) p = (p + 1) & (cap - 1);
        tab[p] = FidSlot{fid, k, 0};
    }
    DevBuf<FidSlot> d;
    if (!d.alloc(cap)) return fail(h, SG_E_NOMEM, "flowId table");
    if (hipMemcpy(d, tab.data(), sizeof(FidSlot) * cap, hipMemcpyHostToDevice) != hipSuccess)
        return fail(h, SG_E_DEVICE, "flowId table upload");
    h->d_fid = std::move(d);
    h->fid_mask = cap - 1;
    return SG_OK;
}

int sg_codec_decode_flow(sg_handle* h, const uint8_t* payload, const uint32_t* offsets, const int64_t* ts_ms,
                         uint64_t n, sg_req* req_out, int32_t* xid_out, uint8_t* kind_out, void* stream) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!payload || !offsets || !ts_ms || !req_out || !xid_out || !kind_out) return fail(h, SG_E_INVAL, "null buffer");
    if (((uintptr_t)payload & 3u) != 0) return fail(h, SG_E_INVAL, "payload must be 4-byte aligned");
    if (!h->d_fid) {
        int rc = upload_fid_table(h);  // no rules loaded yet: every flowId is unknown
        if (rc) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    CodecArgs c{};
    c.n = n;
    c.payload = payload;
    c.offsets = offsets;
    c.ts = ts_ms;
    c.req = req_out;
    c.xid = xid_out;
    c.kind = kind_out;
    c.fid_tab = h->d_fid;
    c.fid_mask = h->fid_mask;
    HIP_TRY(h, launch_codec_decode(c, (hipStream_t)stream));
    return SG_OK;
}

int sg_codec_encode_flow(sg_handle* h, const int32_t* xid, const uint8_t* kind, const sg_result* res, uint64_t n,
                         uint8_t* frames_out, void* stream) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!xid || !kind || !res || !frames_out) return fail(h, SG_E_INVAL, "null buffer");
    if (((uintptr_t)frames_out & 15u) != 0) return fail(h, SG_E_INVAL, "frames_out must be 16-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    CodecArgs c{};
    c.n = n;
    c.xid_in = xid;
    c.kind_in = kind;
    c.res = res;
    c.frames = frames_out;
    HIP_TRY(h, launch_codec_encode(c, (hipStream_t)stream));
    return SG_OK;
}

// ------------------------------------------------- param-flow wire codec and the value dictionary (pcodec.hip)

static int upload_cp_fid_table(sg_handle* h, const sg_cparam_rule* rules, uint32_t n) {
    uint64_t cap = 2;
    while (cap < 2ull * n) cap <<= 1;
    std::vector<FidSlot> tab(cap, FidSlot{0, 0, 0});
    for (uint32_t k = 0; k < n; ++k) {  // flowIds are > 0 and unique (validated by sg_cparam_load_rules)
        uint64_t p = host_fid_hash(rules[k].flow_id) & (cap - 1);
        while (tab[p].fid != 0) p = (p + 1) & (cap - 1);
        tab[p] = FidSlot{rules[k].flow_id, k, 0};
    }
    DevBuf<FidSlot> d;
    if (!d.alloc(cap)) return fail(h, SG_E_NOMEM, "param flowId table");
    if (hipMemcpy(d, tab.data(), sizeof(FidSlot) * cap, hipMemcpyHostToDevice) != hipSuccess)
        return fail(h, SG_E_DEVICE, "param flowId table upload");
    h->d_cpfid = std::move(d);
    h->cpfid_mask = cap - 1;
    return SG_OK;
}

int sg_vdict_init(sg_handle* h, const sg_vdict_config* cfg) {
    if (!h || !cfg) return SG_E_INVAL;
    if (h->vd.on) return fail(h, SG_E_UNSUPPORTED, "the handle already has a value dictionary");
    if (cfg->capacity_log2 < 1 || cfg->capacity_log2 > 28) return fail(h, SG_E_INVAL, "capacity_log2 must be in [1, 28]");
    if (cfg->max_batch_values == 0 || cfg->max_batch_values >= (1ull << 31))
        return fail(h, SG_E_INVAL, "max_batch_values must be in [1, 2^31)");
    HIP_TRY(h, hipSetDevice(h->device));
    auto& v = h->vd;
    v.capacity = 1ull << cfg->capacity_log2;
    v.arena_bytes = cfg->arena_bytes;
    v.max_batch = cfg->max_batch_values;
    const uint64_t slots = 2 * v.capacity;  // at most half full: a probe always ends
    v.tab_mask = slots - 1;
    v.dedupe_slots = 64;
    while (v.dedupe_slots < 2 * v.max_batch) v.dedupe_slots <<= 1;
    const uint64_t frames = h->cfg.max_batch ? h->cfg.max_batch : 1;
    const uint64_t mb = v.max_batch;
    if (!v.tab.alloc_bytes(8 * slots) || !v.entries.alloc_bytes(sizeof(VEntry) * (v.capacity + 1)) ||
        !v.arena.alloc_bytes(v.arena_bytes ? v.arena_bytes : 1) ||
        !v.desc.alloc_bytes(sizeof(VDesc) * mb) || !v.hash.alloc_bytes(8 * mb) ||
        !v.slot_of.alloc_bytes(4 * mb) || !v.dedupe.alloc_bytes(4 * v.dedupe_slots) ||
        !v.scan.alloc_bytes(8 * mb) ||
        !v.sums.alloc_bytes(8 * (scan_blocks(std::max(mb, frames)) + 1)) ||
        !v.cnt.alloc_bytes(8 * frames) || !v.totals.alloc_bytes(16) ||
        hipMemset(v.tab, 0, 8 * slots) != hipSuccess) {
        v = sg_handle::VDict{};
        return fail(h, SG_E_NOMEM, "value dictionary allocation");
    }
    HIP_TRY(h, hipDeviceSynchronize());
    v.on = true;
    return SG_OK;
}

namespace {

VDictArgs vd_args(sg_handle* h, uint64_t m, const uint8_t* src, uint64_t* ids) {
    const auto& v = h->vd;
    VDictArgs a{};
    a.tab = v.tab;
    a.tab_mask = v.tab_mask;
    a.entries = v.entries;
    a.arena = v.arena;
    a.high = v.high;
    a.arena_used = v.arena_used;
    a.free_ids = v.free_ids.get() ? v.free_ids.get() + v.free_head : nullptr;
    a.n_free = v.n_free;
    a.m = m;
    a.src = src;
    a.desc = v.desc;
    a.hash = v.hash;
    a.ids = ids;
    a.slot_of = v.slot_of;
    a.dedupe = v.dedupe;
    a.dedupe_mask = v.dedupe_slots - 1;
    a.scan = v.scan;
    a.n_miss = reinterpret_cast<unsigned long long*>(v.totals + 1);
    return a;
}

// After the lookup pass of a batch of a.m values (ids 0 = miss, *a.n_miss counted): dedupe the misses, rank the
// first occurrences, check the capacity, then append and insert. Returns with the stream idle.
int vd_finish(sg_handle* h, VDictArgs a, hipStream_t stream) {
    auto& v = h->vd;
    uint64_t misses = 0;
    HIP_TRY(h, hipMemcpyAsync(&misses, v.totals + 1, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (misses == 0) return SG_OK;
    uint64_t slots = 64;
    while (slots < 2 * misses) slots <<= 1;  // <= dedupe_slots: misses <= m <= max_batch
    a.dedupe_mask = slots - 1;
    HIP_TRY(h, hipMemsetAsync(v.dedupe, 0xFF, 4 * slots, stream));
    HIP_TRY(h, launch_vd_dedupe(a, stream));
    HIP_TRY(h, launch_scan_u64(v.scan, a.m, v.sums, v.totals, stream));
    uint64_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, v.totals, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    const uint64_t fresh = total >> 32, bytes = total & 0xFFFFFFFFull;
    if (v.count + fresh > v.capacity) return fail(h, SG_E_CAPACITY, "value dictionary full");
    if (v.arena_used + bytes > v.arena_bytes) return fail(h, SG_E_CAPACITY, "value dictionary arena full");
    HIP_TRY(h, launch_vd_commit(a, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    const VdBook b = vd_after_batch(VdBook{v.free_head, v.n_free, v.high, v.count}, fresh);
    v.free_head = b.head;
    v.n_free = b.n_free;
    v.high = b.high;
    v.count = b.live;
    v.arena_used += bytes;
    return SG_OK;
}

constexpr uint32_t kParamTypeSize[8] = {4, 8, 1, 8, 4, 2, 1, 0};  // SG_PARAM_TYPE_* payload bytes (STRING: any)

}  // namespace

int sg_vdict_intern(sg_handle* h, const uint8_t* types, const uint32_t* offsets, const uint8_t* bytes, uint64_t n,
                    uint64_t* ids_out) {
    if (!h) return SG_E_INVAL;
    if (!h->vd.on) return fail(h, SG_E_INVAL, "sg_vdict_init first");
    if (n == 0) return SG_OK;
    if (!types || !offsets || !ids_out) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->vd.max_batch) return fail(h, SG_E_CAPACITY, "more values than max_batch_values");
    for (uint64_t j = 0; j < n; ++j) {
        if (types[j] > SG_PARAM_TYPE_STRING || offsets[j + 1] < offsets[j]) return fail(h, SG_E_INVAL, "bad value record");
        const uint32_t len = offsets[j + 1] - offsets[j];
        if (types[j] != SG_PARAM_TYPE_STRING && len != kParamTypeSize[types[j]])
            return fail(h, SG_E_INVAL, "payload size does not match the type");
        if (len >= (1u << 24)) return fail(h, SG_E_INVAL, "payload of 16 MiB or more");
    }
    const uint64_t nbytes = offsets[n];
    if (nbytes && !bytes) return fail(h, SG_E_INVAL, "null buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf<uint8_t> d_types, d_bytes;
    DevBuf<uint32_t> d_off;
    DevBuf<uint64_t> d_ids;
    int rc = SG_OK;
    auto run = [&]() -> int {
        if (!d_types.alloc_bytes(n) || !d_off.alloc_bytes(4 * (n + 1)) ||
            !d_bytes.alloc_bytes(nbytes ? nbytes : 1) || !d_ids.alloc_bytes(8 * n))
            return fail(h, SG_E_NOMEM, "intern buffers");
        HIP_TRY(h, hipMemcpy(d_types, types, n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(d_off, offsets, 4 * (n + 1), hipMemcpyHostToDevice));
        if (nbytes) HIP_TRY(h, hipMemcpy(d_bytes, bytes, nbytes, hipMemcpyHostToDevice));
        VDictArgs a = vd_args(h, n, d_bytes, d_ids);
        a.types = d_types;
        a.offsets = d_off;
        HIP_TRY(h, hipMemsetAsync(h->vd.totals, 0, 16, nullptr));
        HIP_TRY(h, launch_vd_host_lookup(a, nullptr));
        const int frc = vd_finish(h, a, nullptr);
        if (frc) return frc;
        HIP_TRY(h, hipMemcpy(ids_out, d_ids, 8 * n, hipMemcpyDeviceToHost));
        return SG_OK;
    };
    rc = run();
    (void)hipDeviceSynchronize();
    return rc;
}

int sg_vdict_lookup(sg_handle* h, const uint64_t* ids, uint64_t n, uint8_t* types_out, uint32_t* offsets_out,
                    uint8_t* bytes_out, uint64_t bytes_cap) {
    if (!h) return SG_E_INVAL;
    if (!h->vd.on) return fail(h, SG_E_INVAL, "sg_vdict_init first");
    if (!offsets_out) return fail(h, SG_E_INVAL, "null buffer");
    offsets_out[0] = 0;
    if (n == 0) return SG_OK;
    if (!ids || !types_out) return fail(h, SG_E_INVAL, "null buffer");
    for (uint64_t j = 0; j < n; ++j)
        if (!vd_id_in_range(ids[j], h->vd.high)) return fail(h, SG_E_INVAL, "unknown value id");
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf<uint64_t> d_ids;
    DevBuf<VEntry> d_e;
    DevBuf<uint32_t> d_off;
    DevBuf<uint8_t> d_bytes;
    std::vector<VEntry> e(n);
    auto run = [&]() -> int {
        if (!d_ids.alloc_bytes(8 * n) || !d_e.alloc_bytes(sizeof(VEntry) * n) ||
            !d_off.alloc_bytes(4 * (n + 1)))
            return fail(h, SG_E_NOMEM, "lookup buffers");
        HIP_TRY(h, hipMemcpy(d_ids, ids, 8 * n, hipMemcpyHostToDevice));
        HIP_TRY(h, launch_vd_gather(h->vd.entries, d_ids, n, d_e, nullptr));
        HIP_TRY(h, hipMemcpy(e.data(), d_e, sizeof(VEntry) * n, hipMemcpyDeviceToHost));
        for (uint64_t j = 0; j < n; ++j)  // an id a sweep gave back and no batch has taken since
            if (e[j].type == kVdTombType) return fail(h, SG_E_INVAL, "unknown value id");
        uint64_t total = 0;
        for (uint64_t j = 0; j < n; ++j) {
            types_out[j] = (uint8_t)e[j].type;
            total += e[j].len;
            if (total >= (1ull << 32)) return fail(h, SG_E_CAPACITY, "more than 2^32 payload bytes");
            offsets_out[j + 1] = (uint32_t)total;
        }
        if (total > bytes_cap) return fail(h, SG_E_CAPACITY, "bytes_out too small");
        if (total == 0) return SG_OK;
        if (!bytes_out) return fail(h, SG_E_INVAL, "null buffer");
        if (!d_bytes.alloc_bytes(total)) return fail(h, SG_E_NOMEM, "lookup buffers");
        HIP_TRY(h, hipMemcpy(d_off, offsets_out, 4 * (n + 1), hipMemcpyHostToDevice));
        HIP_TRY(h, launch_vd_bytes(d_e, d_off, n, h->vd.arena, d_bytes, nullptr));
        HIP_TRY(h, hipMemcpy(bytes_out, d_bytes, total, hipMemcpyDeviceToHost));
        return SG_OK;
    };
    const int rc = run();
    (void)hipDeviceSynchronize();
    return rc;
}

int sg_vdict_size(sg_handle* h, uint64_t* n_values, uint64_t* arena_used) {
    if (!h) return SG_E_INVAL;
    if (!h->vd.on) return fail(h, SG_E_INVAL, "sg_vdict_init first");
    if (n_values) *n_values = h->vd.count;
    if (arena_used) *arena_used = h->vd.arena_used;
    return SG_OK;
}

// The reference interns nothing: its maps hold the values themselves and grow. Entries [1, high] and the used arena
// bytes are copied into the larger arrays — ids are array positions, so none moves — and the main table is filled
// again from the entries that are no tombstones (pcodec.hip k_vd_rehash). The free list of the last sweep stays as it
// is: it only ever shrinks between sweeps. The per-batch scratch (max_batch_values) is not touched.
int sg_vdict_grow(sg_handle* h, int32_t capacity_log2, uint64_t arena_bytes) {
    if (!h) return SG_E_INVAL;
    auto& v = h->vd;
    const GrowPlan plan = grow_plan_vdict(v.on, v.capacity, v.arena_bytes, capacity_log2, arena_bytes);
    if (plan.code) return fail(h, plan.code, plan.why);
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const uint64_t capacity = plan.total, slots = 2 * capacity;  // at most half full: a probe always ends
    DevBuf<uint64_t> tab;
    DevBuf<VEntry> entries;
    DevBuf<uint8_t> arena;
    if (!tab.alloc_bytes(8 * slots) || !entries.alloc_bytes(sizeof(VEntry) * (capacity + 1)) ||
        !arena.alloc_bytes(arena_bytes ? arena_bytes : 1))
        return fail(h, SG_E_NOMEM, "grown value dictionary");
    HIP_TRY(h, hipMemsetAsync(tab, 0, 8 * slots, nullptr));
    HIP_TRY(h, hipMemcpyAsync(entries, v.entries, sizeof(VEntry) * (v.high + 1), hipMemcpyDeviceToDevice, nullptr));
    if (v.arena_used)
        HIP_TRY(h, hipMemcpyAsync(arena, v.arena, v.arena_used, hipMemcpyDeviceToDevice, nullptr));
    VDictArgs a{};
    a.tab = tab;
    a.tab_mask = slots - 1;
    a.entries = entries;
    a.arena = arena;
    a.high = v.high;
    HIP_TRY(h, launch_vd_rehash(a, nullptr));
    HIP_TRY(h, hipDeviceSynchronize());
    v.tab = std::move(tab);
    v.entries = std::move(entries);
    v.arena = std::move(arena);
    v.tab_mask = slots - 1;
    v.capacity = capacity;
    v.arena_bytes = arena_bytes;
    return SG_OK;
}

// The dictionary's own sweep, by the mechanism of the table sweeps: new entries, main table, arena and free list are
// built beside the ones in force (vdict_sweep.hip) from the ids that something still names, and swapped in at the end.
// Purely referential: no timestamp is read or raised. The sources are everything on this handle that holds a value
// id between calls — the value tables sg_param_sweep / sg_cparam_sweep read, the thread counts, the hot items of the
// rule sets in force, the gateway's two ids, the unfetched rows of both logs — and the caller's keep list.
int sg_vdict_sweep(sg_handle* h, const uint64_t* keep_ids, uint64_t n_keep, sg_vdict_sweep_stats* out) {
    if (!h) return SG_E_INVAL;
    auto& v = h->vd;
    VdsRefusal ref = vd_sweep_refusal(v.on, n_keep, keep_ids == nullptr, 0);
    if (ref.code) return fail(h, ref.code, ref.why);
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    HIP_TRY(h, hipDeviceSynchronize());  // batches on the caller's streams: their table writes are sources
    uint64_t bad = 0;
    for (uint64_t j = 0; j < n_keep; ++j) bad += !vd_id_in_range(keep_ids[j], v.high);
    ref = vd_sweep_refusal(true, n_keep, false, bad);
    if (ref.code) return fail(h, ref.code, ref.why);
    sg_vdict_sweep_stats st{};
    st.high = v.high;
    st.live = v.count;
    st.free_ids = v.n_free;
    st.arena_before = st.arena_after = v.arena_used;
    if (v.high == 0) {  // nothing was ever interned
        if (out) *out = st;
        return SG_OK;
    }
    const uint64_t high = v.high, words = (high >> 5) + 1, slots = 2 * v.capacity;
    const uint64_t gw_ids[2] = {h->gw.nm_id, h->gw.d_id};
    const uint64_t n_gw = h->gw.on ? 2 : 0;
    DevBuf<uint32_t> d_bits, d_free;
    DevBuf<uint64_t> d_dead, d_bytes, d_sums, d_tot, d_keep, tab;
    DevBuf<VEntry> entries;
    DevBuf<uint8_t> arena;
    if (!d_bits.alloc(words) || !d_dead.alloc(high) || !d_bytes.alloc(high) || !d_sums.alloc(scan_blocks(high) + 1) ||
        !d_tot.alloc(3) || !d_keep.alloc(n_keep + 2) || !tab.alloc(slots) || !entries.alloc(v.capacity + 1) ||
        !arena.alloc(v.arena_bytes ? v.arena_bytes : 1))
        return fail(h, SG_E_NOMEM, "swept value dictionary");
    HIP_TRY(h, hipMemsetAsync(d_bits, 0, 4 * words, nullptr));
    HIP_TRY(h, hipMemsetAsync(d_tot, 0, 24, nullptr));
    HIP_TRY(h, hipMemsetAsync(tab, 0, 8 * slots, nullptr));
    if (n_keep) HIP_TRY(h, hipMemcpy(d_keep, keep_ids, 8 * n_keep, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_keep + n_keep, gw_ids, 16, hipMemcpyHostToDevice));
    // the mark passes, one per kind of source; the extents are this handle's own sizes
    constexpr uint32_t kPSlotWords = sizeof(PSlot) / 8, kThreadWords = sizeof(PSThread) / 8, kHotWords = sizeof(sg_param_hot_item) / 8;
    static_assert(offsetof(PSlot, value) == 0 && offsetof(PSThread, owner) == 0 && offsetof(PSThread, value) == 8 &&
                      offsetof(sg_param_hot_item, value) == 0,
                  "word offsets of the strided mark pass");
    HIP_TRY(h, launch_vds_mark_words(d_bits, high, reinterpret_cast<const uint64_t*>(h->d_ptable.get()), h->ptotal,
                                     kPSlotWords, 0, -1, nullptr));
    HIP_TRY(h, launch_vds_mark_words(d_bits, high, h->d_cpkeys, h->cptotal, 1, 0, -1, nullptr));
    if (h->ps_loaded)
        HIP_TRY(h, launch_vds_mark_words(d_bits, high, reinterpret_cast<const uint64_t*>(h->d_ps_tc.get()), h->ps_tc_slots,
                                         kThreadWords, 1, 0, nullptr));
    HIP_TRY(h, launch_vds_mark_words(d_bits, high, reinterpret_cast<const uint64_t*>(h->d_phot.get()), h->d_phot.size(),
                                     kHotWords, 0, -1, nullptr));
    HIP_TRY(h, launch_vds_mark_words(d_bits, high, reinterpret_cast<const uint64_t*>(h->d_cphot.get()), h->d_cphot.size(),
                                     kHotWords, 0, -1, nullptr));
    HIP_TRY(h, launch_vds_mark_words(d_bits, high, d_keep + n_keep, n_gw, 1, 0, -1, nullptr));
    HIP_TRY(h, launch_vds_mark_blog(d_bits, high, h->d_blog, h->d_blog.size(), nullptr));
    HIP_TRY(h, launch_vds_mark_slog(d_bits, high, h->d_slog, h->d_slog.size(), nullptr));
    HIP_TRY(h, launch_vds_mark_keep(d_bits, high, d_keep, n_keep, v.entries, reinterpret_cast<unsigned long long*>(d_tot + 2),
                                    nullptr));
    VdSweepArgs a{};
    a.entries = v.entries;
    a.arena = v.arena;
    a.high = high;
    a.bits = d_bits;
    a.dead = d_dead;
    a.bytes = d_bytes;
    HIP_TRY(h, launch_vds_flags(a, nullptr));
    HIP_TRY(h, launch_scan_u64(d_dead, high, d_sums, d_tot, nullptr));
    HIP_TRY(h, launch_scan_u64(d_bytes, high, d_sums, d_tot + 1, nullptr));
    uint64_t tot[3] = {0, 0, 0};  // dead ids, live arena bytes, bad keep entries
    HIP_TRY(h, hipMemcpy(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost));
    ref = vd_sweep_refusal(true, n_keep, false, tot[2]);
    if (ref.code) return fail(h, ref.code, ref.why);
    if (!d_free.alloc(tot[0] ? tot[0] : 1)) return fail(h, SG_E_NOMEM, "swept value dictionary");
    a.n_entries = entries;
    a.n_tab = tab;
    a.n_tab_mask = slots - 1;
    a.n_arena = arena;
    a.n_free_ids = d_free;
    HIP_TRY(h, launch_vds_move(a, nullptr));
    HIP_TRY(h, hipDeviceSynchronize());
    st.removed = tot[0] - v.n_free;  // the ids free before are dead again: they are not removed twice
    st.live = high - tot[0];
    st.free_ids = tot[0];
    st.arena_after = tot[1];
    v.tab = std::move(tab);
    v.entries = std::move(entries);
    v.arena = std::move(arena);
    v.free_ids = std::move(d_free);
    v.free_head = 0;
    v.n_free = tot[0];
    v.count = st.live;
    v.arena_used = tot[1];
    if (out) *out = st;
    return SG_OK;
}

int sg_codec_decode_param(sg_handle* h, const uint8_t* payload, const uint32_t* offsets, const int64_t* ts_ms,
                          uint64_t n, sg_cparam_req* req_out, uint64_t* values_out, uint64_t values_cap,
                          uint64_t* n_values, int32_t* xid_out, uint8_t* kind_out, void* stream) {
    if (!h) return SG_E_INVAL;
    if (!n_values) return fail(h, SG_E_INVAL, "null buffer");
    *n_values = 0;
    if (!h->vd.on) return fail(h, SG_E_INVAL, "sg_vdict_init first");
    if (n == 0) return SG_OK;
    if (!payload || !offsets || !ts_ms || !req_out || !xid_out || !kind_out || (!values_out && values_cap))
        return fail(h, SG_E_INVAL, "null buffer");
    if (((uintptr_t)payload & 3u) != 0) return fail(h, SG_E_INVAL, "payload must be 4-byte aligned");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "more frames than max_batch");
    if (!h->d_cpfid) {
        int rc = upload_cp_fid_table(h, nullptr, 0);  // no param rules loaded yet: every flowId is unknown
        if (rc) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    auto& v = h->vd;
    PCodecArgs c{};
    c.n = n;
    c.payload = payload;
    c.offsets = offsets;
    c.ts = ts_ms;
    c.req = req_out;
    c.xid = xid_out;
    c.kind = kind_out;
    c.fid_tab = h->d_cpfid;
    c.fid_mask = h->cpfid_mask;
    c.cnt = v.cnt;
    HIP_TRY(h, launch_pcodec_count(c, st));
    HIP_TRY(h, launch_scan_u64(v.cnt, n, v.sums, v.totals, st));
    HIP_TRY(h, hipMemsetAsync(v.totals + 1, 0, 8, st));
    uint64_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, v.totals, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    *n_values = total;
    if (total > values_cap) return fail(h, SG_E_CAPACITY, "values_out too small");
    if (total > v.max_batch) return fail(h, SG_E_CAPACITY, "more values than max_batch_values");
    c.vd = vd_args(h, total, payload, values_out);
    HIP_TRY(h, launch_pcodec_emit(c, st));
    return vd_finish(h, c.vd, st);
}

int sg_codec_encode_param(sg_handle* h, const int32_t* xid, const uint8_t* kind, const sg_result* res, uint64_t n,
                          uint8_t* frames_out, void* stream) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!xid || !kind || !res || !frames_out) return fail(h, SG_E_INVAL, "null buffer");
    if (((uintptr_t)frames_out & 15u) != 0) return fail(h, SG_E_INVAL, "frames_out must be 16-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    PCodecArgs c{};
    c.n = n;
    c.xid_in = xid;
    c.kind_in = kind;
    c.res = res;
    c.frames = frames_out;
    HIP_TRY(h, launch_pcodec_encode(c, (hipStream_t)stream));
    return SG_OK;
}

// ------------------------------------------------- GatewayFlowSlot: rules and the param parser (gateway.hip)

int sg_gateway_load_rules(sg_handle* h, const sg_gateway_rule* rules, uint32_t n, const uint8_t* pattern_bytes,
                          uint64_t n_pattern_bytes, uint32_t n_resources) {
    if (!h) return SG_E_INVAL;
    if (!h->vd.on) return fail(h, SG_E_INVAL, "sg_vdict_init first");
    if ((n && !rules) || (n_pattern_bytes && !pattern_bytes)) return fail(h, SG_E_INVAL, "null buffer");
    if (n_pattern_bytes >= (1ull << 32)) return fail(h, SG_E_INVAL, "pattern blob of 4 GiB or more");
    if (!gw_ranges_ok(rules, n, n_pattern_bytes, n_resources))
        return fail(h, SG_E_INVAL, "gateway rule: resource >= n_resources or pattern outside the blob");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    // "$NM" then "$D": a known string keeps its id, so a reload (or a header value that came first) moves nothing
    static const uint8_t types[2] = {SG_PARAM_TYPE_STRING, SG_PARAM_TYPE_STRING};
    static const uint32_t offsets[3] = {0, 3, 5};
    static const uint8_t bytes[5] = {'$', 'N', 'M', '$', 'D'};
    uint64_t ids[2] = {0, 0};
    const int irc = sg_vdict_intern(h, types, offsets, bytes, 2, ids);
    if (irc) return irc;
    GwConverted conv = gw_convert(rules, n, n_resources, ids[0]);
    DevBuf<GwRes> d_res;
    DevBuf<GwItemRule> d_rules;
    DevBuf<uint8_t> d_pat;
    DevBuf<uint32_t> d_err;
    if (!d_res.alloc(conv.res.size() ? conv.res.size() : 1) || !d_rules.alloc(conv.items.size() ? conv.items.size() : 1) ||
        !d_pat.alloc(n_pattern_bytes ? n_pattern_bytes : 1) || !d_err.alloc(1))
        return fail(h, SG_E_NOMEM, "gateway parser tables");
    if (!conv.res.empty())
        HIP_TRY(h, hipMemcpy(d_res, conv.res.data(), sizeof(GwRes) * conv.res.size(), hipMemcpyHostToDevice));
    if (!conv.items.empty())
        HIP_TRY(h, hipMemcpy(d_rules, conv.items.data(), sizeof(GwItemRule) * conv.items.size(), hipMemcpyHostToDevice));
    if (n_pattern_bytes) HIP_TRY(h, hipMemcpy(d_pat, pattern_bytes, n_pattern_bytes, hipMemcpyHostToDevice));
    auto& g = h->gw;
    g.conv = std::move(conv);
    g.nm_id = ids[0];
    g.d_id = ids[1];
    g.res = std::move(d_res);
    g.rules = std::move(d_rules);
    g.patterns = std::move(d_pat);
    g.err = std::move(d_err);
    g.on = true;
    h->gwa.n_rules = n;
    h->gwa.fields_set = false;  // the field ids belonged to the rules before
    h->gwa.item_source = gwa_item_sources(g.conv);
    return gwa_renumber(h);
}

int sg_gateway_converted(sg_handle* h, sg_pslot_rule* rules_out, uint32_t cap, uint32_t* n_rules,
                         sg_param_hot_item* hot_out, uint32_t hot_cap, uint32_t* n_hot, uint32_t* source_out) {
    if (!h) return SG_E_INVAL;
    if (!h->gw.on) return fail(h, SG_E_INVAL, "sg_gateway_load_rules first");
    if (!n_rules || !n_hot) return fail(h, SG_E_INVAL, "null buffer");
    const GwConverted& c = h->gw.conv;
    *n_rules = (uint32_t)c.rules.size();
    *n_hot = (uint32_t)c.hot.size();
    if (c.rules.size() > cap || c.hot.size() > hot_cap) return fail(h, SG_E_CAPACITY, "converted rule buffers too small");
    if ((!c.rules.empty() && !rules_out) || (!c.hot.empty() && !hot_out)) return fail(h, SG_E_INVAL, "null buffer");
    std::copy(c.rules.begin(), c.rules.end(), rules_out);
    std::copy(c.hot.begin(), c.hot.end(), hot_out);
    if (source_out) std::copy(c.source.begin(), c.source.end(), source_out);
    return SG_OK;
}

int sg_gateway_param_rule_count(sg_handle* h, uint32_t resource, uint32_t* n_item_rules, int32_t* has_item_less) {
    if (!h) return SG_E_INVAL;
    if (!h->gw.on) return fail(h, SG_E_INVAL, "sg_gateway_load_rules first");
    const auto& res = h->gw.conv.res;
    const GwRes r = resource < res.size() ? res[resource] : GwRes{0, 0, 0, 0};
    if (n_item_rules) *n_item_rules = r.n_items;
    if (has_item_less) *has_item_less = (int32_t)r.has_item_less;
    return SG_OK;
}

int sg_gateway_parse_batch(sg_handle* h, const sg_gateway_req* req, uint64_t n, const sg_gateway_item* items,
                           uint64_t n_items, const uint8_t* bytes, uint64_t n_bytes, sg_pslot_arg* args_out,
                           uint64_t args_cap, uint64_t* values_out, uint64_t values_cap, sg_slot_ext* ext_inout,
                           sg_pslot_event* pev_inout, uint64_t* n_args, uint64_t* n_values, void* stream) {
    if (!h) return SG_E_INVAL;
    if (!n_args || !n_values) return fail(h, SG_E_INVAL, "null buffer");
    *n_args = 0;
    *n_values = 0;
    if (!h->vd.on) return fail(h, SG_E_INVAL, "sg_vdict_init first");
    auto& gw = h->gw;
    if (!gw.on) return fail(h, SG_E_INVAL, "sg_gateway_load_rules first");
    if (n == 0) return SG_OK;
    if (!req || (n_items && !items) || (n_bytes && !bytes) || (args_cap && !args_out) || (values_cap && !values_out))
        return fail(h, SG_E_INVAL, "null buffer");
    if (((uintptr_t)bytes & 3u) != 0) return fail(h, SG_E_INVAL, "bytes must be 4-byte aligned");
    if (n_items >= (1ull << 31) || n_bytes >= (1ull << 32))  // args and values (<= n_items + n) fit 32 bits each
        return fail(h, SG_E_INVAL, "2^31 items or 2^32 bytes, or more");
    auto& v = h->vd;
    if (n > v.max_batch) return fail(h, SG_E_CAPACITY, "more requests than max_batch_values");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (!gw.cnt.reserve(n + 1) || !gw.item_map.reserve(n_items ? n_items : 1) || !gw.sums.reserve(scan_blocks(n + 1) + 1))
        return fail(h, SG_E_NOMEM, "gateway batch buffers");
    GwArgs g{};
    g.n = n;
    g.req = req;
    g.items = items;
    g.n_items = n_items;
    g.bytes = bytes;
    g.n_bytes = n_bytes;
    g.res = gw.res;
    g.n_resources = (uint32_t)gw.conv.res.size();
    g.rules = gw.rules;
    g.patterns = gw.patterns;
    g.nm_id = gw.nm_id;
    g.d_id = gw.d_id;
    g.cnt = gw.cnt;
    g.item_map = gw.item_map;
    g.err = gw.err;
    g.args = args_out;
    g.ext = ext_inout;
    g.pev = pev_inout;
    HIP_TRY(h, hipMemsetAsync(gw.err, 0, 4, st));
    if (n_items) HIP_TRY(h, hipMemsetAsync(gw.item_map, 0, 8 * n_items, st));
    HIP_TRY(h, launch_gw_count(g, st));
    HIP_TRY(h, launch_scan_u64(gw.cnt, n + 1, gw.sums, v.totals, st));
    HIP_TRY(h, hipMemsetAsync(v.totals + 1, 0, 8, st));
    uint64_t total = 0;
    uint32_t err = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, v.totals, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(&err, gw.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (err & kGwErrItemCount) return fail(h, SG_E_INVAL, "item_count differs from the resource's item-rule count");
    if (err & kGwErrRange) return fail(h, SG_E_INVAL, "item range or byte range out of bounds, or a string of 16 MiB or more");
    if (err & kGwErrShared) return fail(h, SG_E_INVAL, "an item belongs to two requests");
    const uint64_t na = total >> 32, nv = total & 0xFFFFFFFFull;
    *n_args = na;
    *n_values = nv;
    if (na > args_cap) return fail(h, SG_E_CAPACITY, "args_out too small");
    if (nv > values_cap) return fail(h, SG_E_CAPACITY, "values_out too small");
    if (nv > v.max_batch) return fail(h, SG_E_CAPACITY, "more values than max_batch_values");
    if (nv) {
        g.vd = vd_args(h, nv, bytes, values_out);
        HIP_TRY(h, launch_gw_match(g, st));
        const int frc = vd_finish(h, g.vd, st);
        if (frc) return frc;
    }
    HIP_TRY(h, launch_gw_emit(g, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return SG_OK;
}

// ------------------------------------------------- Gateway API definitions and request expansion (gateway_api.hip)

int sg_gateway_load_apis(sg_handle* h, const sg_gateway_api* apis, uint32_t n_apis, const sg_gateway_api_pred* preds,
                         uint32_t n_preds, const uint8_t* pattern_bytes, uint64_t n_pattern_bytes, uint32_t n_resources,
                         uint32_t default_context) {
    if (!h) return SG_E_INVAL;
    if ((n_apis && !apis) || (n_preds && !preds) || (n_pattern_bytes && !pattern_bytes))
        return fail(h, SG_E_INVAL, "null buffer");
    if (n_pattern_bytes >= (1ull << 32)) return fail(h, SG_E_INVAL, "pattern blob of 4 GiB or more");
    if (!gwa_ranges_ok(apis, n_apis, preds, n_preds, n_pattern_bytes, n_resources))
        return fail(h, SG_E_INVAL, "API definition: resource >= n_resources, predicates outside preds or pattern outside the blob");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    static const uint8_t none = 0;
    GwaTables t = gwa_build(apis, n_apis, preds, n_preds, pattern_bytes ? pattern_bytes : &none);
    sg_handle::GatewayApi d;  // the new tables, moved in only when all of them are up
    const std::vector<uint8_t> blob(pattern_bytes, pattern_bytes + n_pattern_bytes);
    if (!gwa_upload(d.exact, t.exact) || !gwa_upload(d.bucket, t.bucket) || !gwa_upload(d.exact_list, t.exact_list) ||
        !gwa_upload(d.vid_begin, t.vid_begin) || !gwa_upload(d.vid_apis, t.vid_apis) || !gwa_upload(d.api_res, t.api_res) ||
        !gwa_upload(d.ant, t.ant) || !gwa_upload(d.wild, t.wild) || !gwa_upload(d.patterns, blob) || !d.err.alloc(1))
        return fail(h, SG_E_NOMEM, "API definition tables");
    auto& a = h->gwa;
    a.t = std::move(t);
    a.default_context = default_context;
    a.exact = std::move(d.exact);
    a.bucket = std::move(d.bucket);
    a.exact_list = std::move(d.exact_list);
    a.vid_begin = std::move(d.vid_begin);
    a.vid_apis = std::move(d.vid_apis);
    a.api_res = std::move(d.api_res);
    a.ant = std::move(d.ant);
    a.wild = std::move(d.wild);
    a.patterns = std::move(d.patterns);
    a.err = std::move(d.err);
    a.on = true;
    return gwa_renumber(h);
}

int sg_gateway_verdict_ids(sg_handle* h, uint8_t* kind_out, uint32_t* index_out, uint32_t cap, uint32_t* n) {
    if (!h) return SG_E_INVAL;
    if (!n) return fail(h, SG_E_INVAL, "null buffer");
    const auto& a = h->gwa;
    const size_t n_api = a.on ? a.t.vid_pred.size() : 0, n_rule = h->gw.on ? a.vid_rule.size() : 0;
    *n = (uint32_t)(n_api + n_rule);
    if (n_api + n_rule > cap) return fail(h, SG_E_CAPACITY, "verdict id buffers too small");
    if ((n_api + n_rule) && (!kind_out || !index_out)) return fail(h, SG_E_INVAL, "null buffer");
    for (size_t i = 0; i < n_api + n_rule; ++i) {
        kind_out[i] = i < n_api ? 0 : 1;
        index_out[i] = i < n_api ? a.t.vid_pred[i] : a.vid_rule[i - n_api];
    }
    return SG_OK;
}

int sg_gateway_set_item_fields(sg_handle* h, const uint32_t* field_id, uint32_t n) {
    if (!h) return SG_E_INVAL;
    if (!h->gw.on) return fail(h, SG_E_INVAL, "sg_gateway_load_rules first");
    auto& a = h->gwa;
    if (n != a.n_rules) return fail(h, SG_E_INVAL, "n differs from the rule count of the last sg_gateway_load_rules");
    if (n && !field_id) return fail(h, SG_E_INVAL, "null buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    std::vector<uint32_t> f(a.item_source.size());
    for (size_t j = 0; j < f.size(); ++j) f[j] = field_id[a.item_source[j]];
    DevBuf<uint32_t> d;
    if (!gwa_upload(d, f)) return fail(h, SG_E_NOMEM, "gateway item fields");
    a.item_field = std::move(d);
    a.fields_set = true;
    return SG_OK;
}

int sg_gateway_expand_batch(sg_handle* h, const sg_gateway_http_req* req, uint64_t n, const sg_gateway_field* fields,
                            uint64_t n_fields, const uint32_t* verdicts, uint64_t n_verdicts, const uint8_t* bytes,
                            uint64_t n_bytes, sg_gateway_req* req_out, uint64_t req_cap, sg_gateway_item* items_out,
                            uint64_t items_cap, uint32_t* src_out, sg_local_event* ev_out, sg_slot_ext* ext_out,
                            uint64_t* n_req, uint64_t* n_items, void* stream) {
    if (!h) return SG_E_INVAL;
    if (!n_req || !n_items) return fail(h, SG_E_INVAL, "null buffer");
    *n_req = 0;
    *n_items = 0;
    auto& a = h->gwa;
    auto& gw = h->gw;
    if (!a.on || !gw.on) return fail(h, SG_E_INVAL, "sg_gateway_load_apis and sg_gateway_load_rules first");
    if (a.item_vid.size() < std::max<size_t>(gw.conv.items.size(), 1) || a.item_field.size() < std::max<size_t>(gw.conv.items.size(), 1))
        return fail(h, SG_E_INVAL, "the gateway rules' verdict ids are not in place: load again");
    if (n == 0) return SG_OK;
    if (!req || (n_fields && !fields) || (n_verdicts && !verdicts) || (n_bytes && !bytes) ||
        (req_cap && (!req_out || !src_out || !ev_out || !ext_out)) || (items_cap && !items_out))
        return fail(h, SG_E_INVAL, "null buffer");
    if (((uintptr_t)bytes & 3u) != 0) return fail(h, SG_E_INVAL, "bytes must be 4-byte aligned");
    if (n_fields >= (1ull << 32) || n_verdicts >= (1ull << 32) || n_bytes >= (1ull << 32))
        return fail(h, SG_E_INVAL, "2^32 fields, verdicts or bytes, or more");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (!a.cnt.reserve(2 * (n + 1)) || !a.sums.reserve(scan_blocks(n + 1) + 4)) return fail(h, SG_E_NOMEM, "gateway batch buffers");
    GwxArgs g{};
    g.n = n;
    g.req = req;
    g.fields = fields;
    g.n_fields = n_fields;
    g.verdicts = verdicts;
    g.n_verdicts = n_verdicts;
    g.bytes = bytes;
    g.n_bytes = n_bytes;
    g.exact = a.exact;
    g.exact_list = a.exact_list;
    g.bucket = a.bucket;
    g.ant = a.ant;
    g.wild = a.wild;
    g.vid_begin = a.vid_begin;
    g.vid_apis = a.vid_apis;
    g.api_res = a.api_res;
    g.patterns = a.patterns;
    g.exact_mask = (uint32_t)a.t.exact.size() - 1;
    g.bucket_mask = (uint32_t)a.t.bucket.size() - 1;
    g.n_wild = (uint32_t)a.t.wild.size();
    g.n_api_vids = (uint32_t)a.t.vid_pred.size();
    g.n_vids = g.n_api_vids + (uint32_t)a.vid_rule.size();
    g.default_context = a.default_context;
    g.res = gw.res;
    g.rules = gw.rules;
    g.item_field = a.item_field;
    g.item_vid = a.item_vid;
    g.n_resources = (uint32_t)gw.conv.res.size();
    g.fields_set = a.fields_set ? 1u : 0u;
    g.cnt = a.cnt;
    g.cnt_items = a.cnt + (n + 1);
    g.err = a.err;
    g.req_out = req_out;
    g.items_out = items_out;
    g.src_out = src_out;
    g.ev_out = ev_out;
    g.ext_out = ext_out;
    uint64_t* d_total = a.sums + scan_blocks(n + 1) + 1;  // [2] behind the scan's workspace: entries, items
    HIP_TRY(h, hipMemsetAsync(a.err, 0, 4, st));
    HIP_TRY(h, launch_gwx_count(g, st));
    HIP_TRY(h, launch_scan_u64(g.cnt, n + 1, a.sums, d_total, st));
    HIP_TRY(h, launch_scan_u64(g.cnt_items, n + 1, a.sums, d_total + 1, st));
    uint64_t total[2] = {0, 0};
    uint32_t err = 0;
    HIP_TRY(h, hipMemcpyAsync(total, d_total, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (err & kGwxErrRange) return fail(h, SG_E_INVAL, "a path, field or verdict range out of bounds");
    if (err & kGwxErrVerdict) return fail(h, SG_E_INVAL, "a verdict slice not ascending, or a verdict id out of range");
    const uint64_t ne = total[0], ni = total[1];
    *n_req = ne;
    *n_items = ni;
    if (ne >= (1ull << 32) || ni >= (1ull << 32)) return fail(h, SG_E_CAPACITY, "the batch expands to 2^32 entries or items, or more");
    if (ne > req_cap) return fail(h, SG_E_CAPACITY, "req_out too small");
    if (ni > items_cap) return fail(h, SG_E_CAPACITY, "items_out too small");
    if (ne) HIP_TRY(h, launch_gwx_emit(g, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return SG_OK;
}

int sg_enable_stats(sg_handle* h, int on) {
    if (!h) return SG_E_INVAL;
    h->stats_on = on != 0;
    return SG_OK;
}

int sg_get_stats(const sg_handle* h, sg_batch_stats* out) {
    if (!h || !out) return SG_E_INVAL;
    *out = h->stats;
    return SG_OK;
}

namespace {

// The batch's error flags → return code (the batch is rejected as a whole; no state changed).
int flow_status(sg_handle* h, int err) {
    if (err & kErrTime)
        return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    if (err & kErrPeriods) return fail(h, SG_E_UNSUPPORTED, "batch spans more than 65536 window periods");
    if (err & kErrInternal) return fail(h, SG_E_DEVICE, "internal walker error");
    if (err & kErrExchange)
        return fail(h, SG_E_INVAL, "a request of a limited namespace lies outside the limiter exchange's time range");
    return SG_OK;
}

// A local batch's error flags → return code (rejected as a whole; no state changed).
int local_status(sg_handle* h, int err) {
    if (err & kErrTime)
        return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    if (err & kErrPeriods) return fail(h, SG_E_UNSUPPORTED, "batch spans more than 65536 window periods");
    if (err & kErrBounds)
        return fail(h, SG_E_INVAL, "an event's origin id (0..n_origins), context id (0..n_contexts-1) or arguments "
                                   "(the arg / value arrays) are out of range");
    if (err & kErrTableFull) return fail(h, SG_E_CAPACITY, "a param value or thread-count table is full");
    if (err & kErrInternal) return fail(h, SG_E_DEVICE, "internal walker error");
    return SG_OK;
}

int ticket_status(sg_handle* h, const sg_handle::DevTicket& d) {
    if (!d.local) return flow_status(h, *d.h_err);
    const int rc = local_status(h, *d.h_err);
    // a refused pipelined batch (e.g. its first timestamp behind the previous batch's, found by the back half)
    // decided nothing: it does not count as a batch seen (enqueue_local_pipelined counted it)
    if (rc != SG_OK && h->l_batches > 0) --h->l_batches;
    return rc;
}

// Workspace 1 and the pipeline's streams / events, allocated on first pipelined batch (seg_end grows with K).
int pipe_setup(sg_handle* h) {
    auto& w = h->ws[1];
    if (!w.rec) {
        if (!flow_ws_alloc(h, w)) return fail(h, SG_E_NOMEM, "pipeline workspace");
        // CU partition between the halves (env SG_FRONT_SIXTEENTHS = k: the front half gets the CUs whose sixteenth
        // 2 * (i % 8) + (i / 8) % 2 is below k, the walkers the rest; 0 = no masks, both halves on every CU). An even
        // k takes the CUs with i % 8 < k / 2; an odd k adds every other CU of the next eighth.
        int cus = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
        const int k16 = h->front_sixteenths;
        if (k16 > 0 && k16 < 16 && cus >= 8) {
            std::vector<uint32_t> fm((cus + 31) / 32, 0u), bm((cus + 31) / 32, 0u);
            int nb = 0;
            for (int i = 0; i < cus; ++i) {
                if (2 * (i % 8) + (i / 8) % 2 < k16) fm[i / 32] |= 1u << (i % 32);
                else {
                    bm[i / 32] |= 1u << (i % 32);
                    ++nb;
                }
            }
            HIP_TRY(h, hipExtStreamCreateWithCUMask(h->s_front.put(), (uint32_t)fm.size(), fm.data()));
            HIP_TRY(h, hipExtStreamCreateWithCUMask(h->s_back.put(), (uint32_t)bm.size(), bm.data()));
            HIP_TRY(h, hipExtStreamCreateWithCUMask(h->s_aux2.put(), (uint32_t)bm.size(), bm.data()));
            h->walk_cus = nb;
        } else {
            HIP_TRY(h, hipStreamCreateWithFlags(h->s_front.put(), hipStreamNonBlocking));
            HIP_TRY(h, hipStreamCreateWithFlags(h->s_back.put(), hipStreamNonBlocking));
            HIP_TRY(h, hipStreamCreateWithFlags(h->s_aux2.put(), hipStreamNonBlocking));
        }
        for (int x = 0; x < 2; ++x) {
            HIP_TRY(h, hipEventCreateWithFlags(h->front_done[x].put(), hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(h->back_done[x].put(), hipEventDisableTiming));
        }
        HIP_TRY(h, hipEventCreateWithFlags(h->pfork.put(), hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(h->pjoin.put(), hipEventDisableTiming));
    }
    if (w.seg_cap < h->K) {  // grows with K; a reload to no more rules keeps it (all marks are reset between batches)
        w.seg_cap = 0;
        w.seg_start = nullptr;
        const int rc = flow_seg_alloc(h, w.seg_end, h->K);
        if (rc) return rc;
        w.seg_cap = h->K + 1;
    }
    w.seg_start = w.seg_end + w.seg_cap;
    return SG_OK;
}

BatchArgs flow_args(sg_handle* h, const sg_handle::FlowWs& w, const sg_req* req, uint64_t n, sg_result* out) {
    BatchArgs a{};
    a.req = req;
    a.out = out;
    a.n = n;
    a.rec = w.rec;
    a.rec_sorted = w.rec_sorted;
    a.hist0 = h->n_lim > 0 ? nullptr : w.hist;  // the limiter pre-pass rewrites records after k_prep
    a.hist0_bits = radix_digit_bits(h->kbits);
    a.kshift = 64 - h->kbits;
    a.hist0_shift = a.kshift;
    a.abits = h->abits;
    a.imask = (h->ibits >= 64) ? ~0ull : ((1ull << h->ibits) - 1);
    a.amask = (1ull << h->abits) - 1;
    a.aesc = (1ull << (h->abits - 1)) - 1;
    a.K = h->K;
    a.rules = h->d_rules;
    a.ring = h->d_ring;
    a.hot = h->d_hot;
    a.occ = h->d_occ;
    a.seg_end = w.seg_end;
    a.seg_start = w.seg_start;
    a.short_end = w.short_end;
    a.stride = h->stride;
    a.max_occ_ratio = h->cfg.max_occupy_ratio;
    a.n_wl = h->n_wl;
    std::memcpy(a.wl, h->wl, sizeof(a.wl));
    a.bnd = w.bnd;
    a.p0 = w.p0;
    a.np = w.np;
    a.err = w.err;
    a.last_ts = h->d_last_ts;
    a.check_last = 1;
    a.walk_cus = 0;
    a.long_list = w.long_list;
    a.long_count = w.counts;
    a.short_list = w.short_list;
    a.short_key = w.short_key;
    a.long_key = w.long_key;
    a.long_end = w.long_end;
    a.long_pend = w.long_pend;
    a.short_count = w.counts + 1;
    for (int c = 0; c < kClasses; ++c) a.class_off[c] = h->class_off[c];
    a.skips = w.skips;
    a.skip_count = w.skip_count;
    a.dbg = h->dbg;
    a.generic_walker = (h->cfg.flags & SG_FLAG_RING_REREAD) != 0;
    a.narrow = h->wide_seen ? 0 : 1;
    a.dbg_ctr = h->d_dbg;
    a.skip_cap = (uint32_t)(2 * h->cfg.max_batch / kSkipMin + 1);
    a.short_max = (h->cfg.flags & SG_FLAG_WAVE_ONLY) ? 0u
                  : (h->cfg.flags & SG_FLAG_SERIAL_ONLY) ? 0xFFFFFFFFu : h->short_max;
    return a;
}

// Front half of a batch on `stream`: validation and packed records (k_prep), the namespace limiter pre-pass,
// the stable sort by flowId and the segment lists. Touches only the workspace, the caller's output (default
// results) and the limiter state.
// The namespace limiter pre-pass over a batch's records (after k_prep): TOO_MANY_REQUEST results, sentinel records.
int flow_limiter(sg_handle* h, BatchArgs& a, hipStream_t stream) {
    if (h->n_lim > 0) {
        LimArgs L{};
        L.n_lim = h->n_lim;
        L.wl_idx = h->lim_wl_idx;
        std::memcpy(L.qps, h->lim_qps, sizeof(L.qps));
        L.rule_lim = h->d_rule_lim;
        L.slot = h->d_lim_slot;
        const uint64_t tiles = a.n / 4096 + 1;
        L.tile_tot = h->d_lim_tile;
        L.tile_off = h->d_lim_tile + tiles * kMaxLim;
        L.arrivals = h->d_lim_period;
        L.prefix = h->d_lim_period + (size_t)kMaxLim * kMaxPeriods;
        L.quota = h->d_lim_period + (size_t)2 * kMaxLim * kMaxPeriods;
        L.ring = h->d_lim_ring;
        if (h->lim_x_armed) {
            L.xg = h->lim_xg;
            L.ts = &a.req[0].ts_ms;
            L.ts_stride = sizeof(sg_req) / sizeof(int64_t);
            L.t_base = h->lim_xt;
            L.n_ms = h->lim_xn;
            L.world = h->shard_world;
            L.rank = h->shard_rank;
        }
        HIP_TRY(h, launch_limiter(a, L, stream));
    }
    return SG_OK;
}

// The binned front half (engine.hip k_bin_sort) for a flow batch of workspace w when the handle's records allow it:
// >= 2^14 flowIds (SG_BIN=2: any), at most 2^20 (a regular bin holds <= 2048 flowIds), kBinDigit free middle bits,
// no namespace limiter (its pre-pass rewrites records after k_prep). Sets a's bin fields; false: the two-pass sort.
bool bin_setup(sg_handle* h, sg_handle::FlowWs& w, BatchArgs& a, hipStream_t stream) {
    if (h->bin_mode == 0 || h->n_lim > 0 || !a.hist0 || a.n == 0 || h->K == 0) return false;
    if (h->bin_mode == 1 && h->K < (1u << 14)) return false;
    if (64 - h->kbits - h->ibits - h->abits < kBinDigit) return false;
    const int kb = h->K > 1 ? bits_for((uint64_t)h->K - 1) : 1;
    const int bsh = std::max(0, kb - 9);
    if (bsh > kBinMaxBsh || (((h->K - 1) >> bsh) + 1) > kBinRegular) return false;
    if (!h->d_hot_key) {
        if (!h->d_hot_key.alloc_bytes(sizeof(uint32_t) * (kBinHot + 1) + sizeof(uint2) * kHotTab))
            return false;
        h->hot_gen = ~0ull;
    }
    uint2* tab = reinterpret_cast<uint2*>(h->d_hot_key + kBinHot + 1);
    if (!w.bin_buf) {
        if (!w.bin_buf.alloc(h->cfg.max_batch + kRecW)) return false;
    }
    if (h->hot_gen != h->rules_gen) {  // flowIds renumbered: no hot flowIds yet (stream-ordered before k_prep)
        if (launch_hot_reset(tab, stream) != hipSuccess) return false;
        h->hot_gen = h->rules_gen;
    }
    a.bin_on = 1;
    a.prep_tiles = h->prep_tiles;
    a.bin_dshift = h->abits + h->ibits;
    a.bin_bsh = bsh;
    a.bin_R = ((h->K - 1) >> bsh) + 1;
    a.hot_tab = tab;
    a.hot_key = h->d_hot_key;
    a.bin_buf = w.bin_buf;
    a.hist0_bits = kBinDigit;
    a.hist0_shift = a.bin_dshift;
    a.rec4 = (h->rec4 && h->abits == kRec4Abits && h->ibits <= 24) ? 1 : 0;
    return true;
}

int flow_front(sg_handle* h, BatchArgs& a, uint32_t* hist, hipStream_t stream, bool stats) {
    if (stats) HIP_TRY(h, hipEventRecord(h->ev[0], stream));
    HIP_TRY(h, hipMemsetAsync(a.err, 0, sizeof(int), stream));
    HIP_TRY(h, hipMemsetAsync(a.long_count, 0, (1 + kClasses) * sizeof(uint32_t), stream));
    HIP_TRY(h, hipMemsetAsync(a.skip_count, 0, sizeof(uint32_t), stream));
    a.csum0 = nullptr;
    if (a.hist0 && radix_csum_atomic()) {
        a.csum0 = radix_csum(a.hist0, a.n, a.hist0_bits);
        HIP_TRY(h, hipMemsetAsync(a.csum0, 0, radix_csum_bytes(a.n, a.hist0_bits), stream));
    }
    HIP_TRY(h, launch_prep(a, stream));
    const int lrc = flow_limiter(h, a, stream);
    if (lrc) return lrc;
    if (a.front_ts) HIP_TRY(h, launch_front_ts(a, stream));
    if (stats) HIP_TRY(h, hipEventRecord(h->ev[1], stream));
    if (a.bin_on) {  // one scatter pass by bin digit, the regular bins sorted and every segment listed in LDS
        HIP_TRY(h, launch_bin_front(a, hist, true, a.csum0 != nullptr, stream));
        a.bin_tot = radix_tot(hist, a.n, kBinDigit);  // the stat log's add reads the rejected requests' total
        if (stats) HIP_TRY(h, hipEventRecord(h->ev[2], stream));
        return SG_OK;
    }
    {
        uint64_t* sorted = nullptr;
        HIP_TRY(h, radix_sort_records(a.rec, a.rec_sorted, a.n, a.kshift, hist, &sorted, stream, 64, a.hist0 != nullptr,
                                      a.csum0 != nullptr));
        a.rec_sorted = sorted;
    }
    if (stats) HIP_TRY(h, hipEventRecord(h->ev[2], stream));
    HIP_TRY(h, launch_seg_flow(a, stream));
    return SG_OK;
}

// Back half on `stream` (after the front half and after the previous batch's back half): the cross-batch time
// check (when the front half skipped it), both walkers (long segments on `aux`), skipped BLOCK counts, the
// handle's last timestamp; the error word lands in the pinned err_dst.
int flow_back(sg_handle* h, const BatchArgs& a, hipStream_t stream, hipStream_t aux, hipEvent_t fork, hipEvent_t join,
              int* err_dst, bool stats) {
    if (!a.check_last) HIP_TRY(h, launch_check_last(a, stream));
    if (h->dbg & 2) {
        HIP_TRY(h, launch_walk_long(a, stream));
        HIP_TRY(h, launch_walk_short(a, stream));
    } else {
        HIP_TRY(h, hipEventRecord(fork, stream));
        HIP_TRY(h, hipStreamWaitEvent(aux, fork, 0));
        HIP_TRY(h, launch_walk_long(a, aux));
        HIP_TRY(h, launch_walk_short(a, stream));
        HIP_TRY(h, hipEventRecord(join, aux));
        HIP_TRY(h, hipStreamWaitEvent(stream, join, 0));
    }
    HIP_TRY(h, launch_skip_apply(a, stream));
    if (stats) HIP_TRY(h, hipEventRecord(h->ev[3], stream));
    if (h->d_slog) {  // the token server's stat log, behind the decisions
        const int src = slog_add_flow(h, a, stream);
        if (src) return src;
    }
    HIP_TRY(h, launch_finish(a, stream));
    HIP_TRY(h, hipMemcpyAsync(err_dst, a.err, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (stats) {
        HIP_TRY(h, hipMemcpyAsync(h->h_long, a.long_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipMemcpyAsync(h->h_long + 1, a.skip_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipEventRecord(h->ev[4], stream));
    }
    return SG_OK;
}

int ensure_layout(sg_handle* h) {
    if (h->K == 0 && h->kbits == 0) return layout_records(h);
    return SG_OK;
}

// Enqueue one batch's whole pipeline on `stream` with workspace 0 (req/out device-resident); its error flags
// land in the pinned word err_dst when the stream reaches the end. Stats events only for the synchronous call.
int enqueue_flow(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, hipStream_t stream, int* err_dst,
                 bool stats) {
    int rc = ensure_layout(h);
    if (rc) return rc;
    sg_handle::FlowWs& w = h->ws[0];
    BatchArgs a = flow_args(h, w, req, n, out);
    bin_setup(h, w, a, stream);
    rc = flow_front(h, a, w.hist, stream, stats);
    if (rc) return rc;
    h->last_sorted = a.rec_sorted;
    h->last_rec4_n = a.rec4 ? n : 0;
    return flow_back(h, a, stream, h->aux, h->fork, h->join, err_dst, stats);
}

// Enqueue one batch on the pipeline: its front half waits for `after` (its input's arrival, may be null) and for
// the walkers of the batch two back (same workspace); its back half follows its front half and the previous
// batch's back half. With namespace limiters the cross-batch time check stays in k_prep, against front_ts (the
// limiter pre-pass must see only accepted batches). Returns the event that marks the batch's completion through
// *done (the back half's end, recorded on s_back).
int enqueue_flow_pipelined(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, hipEvent_t after, int* err_dst,
                           hipEvent_t done) {
    int rc = ensure_layout(h);
    if (rc) return rc;
    rc = pipe_setup(h);
    if (rc) return rc;
    const int x = (int)(h->pipe_seq & 1);
    sg_handle::FlowWs& w = h->ws[x];
    // sharded namespace limiter: the armed exchange is copied into workspace x's own buffer now (the caller's
    // buffer is free again when this returns); the batch two back, which read that buffer, has finished its
    // front half by then
    const bool xshard = h->shard_world > 1 && h->n_lim > 0;
    if (xshard) {
        const uint64_t words = (uint64_t)h->shard_world * h->n_lim * h->lim_xn;
        if (words > h->d_xg_ws[0].size() || words > h->d_xg_ws[1].size()) {
            (void)hipDeviceSynchronize();
            if (!h->d_xg_ws[0].reserve(words) || !h->d_xg_ws[1].reserve(words))
                return fail(h, SG_E_NOMEM, "exchange buffers");
        } else if (h->pipe_seq >= 2) {
            HIP_TRY(h, hipEventSynchronize(h->front_done[x]));
        }
        // complete before returning (the caller may free or refill its buffer then): a device-to-device hipMemcpy
        // may return before the copy has run, and the front half on s_front could read a half-copied exchange
        if (!h->s_xcopy) {
            HIP_TRY(h, hipStreamCreateWithFlags(h->s_xcopy.put(), hipStreamNonBlocking));
            HIP_TRY(h, hipEventCreateWithFlags(h->xcopy_done.put(), hipEventDisableTiming));
        }
        HIP_TRY(h, hipMemcpyAsync(h->d_xg_ws[x], h->lim_xg, 4 * words, hipMemcpyDeviceToDevice, h->s_xcopy));
        HIP_TRY(h, hipEventRecord(h->xcopy_done, h->s_xcopy));
        HIP_TRY(h, hipEventSynchronize(h->xcopy_done));
    }
    BatchArgs a = flow_args(h, w, req, n, out);
    bin_setup(h, w, a, h->s_front);
    if (after) HIP_TRY(h, hipStreamWaitEvent(h->s_front, after, 0));
    if (h->pipe_seq >= 2) HIP_TRY(h, hipStreamWaitEvent(h->s_front, h->back_done[x], 0));
    if (h->n_lim > 0) {
        // the limiter pre-pass must see only accepted batches: k_prep checks the time order against the previous
        // front half's last timestamp (front_ts, advanced once a batch passed validation) as well as last_ts, so
        // this front half need not wait for the previous batch's walkers.
        // A batch the back half later refuses has still advanced front_ts: the next batch is checked against its
        // timestamps too (a batch must be time-ordered after every batch submitted before it, accepted or not).
        a.front_ts = h->d_front_ts;
    } else {
        a.check_last = 0;  // checked by the back half, after the previous batch has advanced last_ts
    }
    if (xshard) {
        h->lim_xg = h->d_xg_ws[x];
        h->lim_x_armed = true;  // read by flow_front
    }
    rc = flow_front(h, a, w.hist, h->s_front, false);
    h->lim_x_armed = false;
    if (rc) return rc;
    if (x == 0) {
        h->last_sorted = a.rec_sorted;
        h->last_rec4_n = a.rec4 ? n : 0;
    }
    HIP_TRY(h, hipEventRecord(h->front_done[x], h->s_front));
    HIP_TRY(h, hipStreamWaitEvent(h->s_back, h->front_done[x], 0));
    a.walk_cus = h->walk_cus;
    rc = flow_back(h, a, h->s_back, h->s_aux2, h->pfork, h->pjoin, err_dst, false);
    if (rc) return rc;
    HIP_TRY(h, hipEventRecord(h->back_done[x], h->s_back));
    if (done) HIP_TRY(h, hipEventRecord(done, h->s_back));
    h->pipe_seq++;
    return SG_OK;
}

// Completes every batch of the host pipeline (their statuses are kept for sg_flow_poll / sg_flow_wait): the
// synchronous entry points and every state-changing call start from a drained handle.
int drain_async(sg_handle* h) {
    for (auto& sl : h->slots) {
        if (!sl.ticket) continue;
        hipError_t e = hipEventSynchronize(sl.d2h);
        h->finished[sl.ticket] = e != hipSuccess ? fail(h, SG_E_DEVICE, hipGetErrorString(e)) : flow_status(h, *sl.h_err);
        sl.ticket = 0;
    }
    for (auto& d : h->dev) {
        if (!d.ticket) continue;
        hipError_t e = hipEventSynchronize(d.done);
        h->finished[d.ticket] = e != hipSuccess ? fail(h, SG_E_DEVICE, hipGetErrorString(e)) : ticket_status(h, d);
        d.ticket = 0;
    }
    if (h->s_back) (void)hipStreamSynchronize(h->s_back);  // workspace 0 is the synchronous path's too
    return SG_OK;
}

}  // namespace

sg_handle::~sg_handle() {
    (void)hipSetDevice(device);
    drain_async(this);
}

namespace {

// The sharded limiter's plan over the armed exchange alone (no local batch): every shard's replica of the namespace
// windows walks the same node arrivals.
int lim_plan_only(sg_handle* h, hipStream_t stream) {
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    int rc = ensure_layout(h);
    if (rc) return rc;
    BatchArgs a{};
    a.err = h->ws[0].err;
    LimArgs L{};
    L.n_lim = h->n_lim;
    std::memcpy(L.qps, h->lim_qps, sizeof(L.qps));
    L.arrivals = h->d_lim_period;
    L.prefix = h->d_lim_period + (size_t)kMaxLim * kMaxPeriods;
    L.quota = h->d_lim_period + (size_t)2 * kMaxLim * kMaxPeriods;
    L.ring = h->d_lim_ring;
    L.xg = h->lim_xg;
    L.t_base = h->lim_xt;
    L.n_ms = h->lim_xn;
    L.world = h->shard_world;
    L.rank = h->shard_rank;
    HIP_TRY(h, hipMemsetAsync(a.err, 0, sizeof(int), stream));
    HIP_TRY(h, launch_limiter_plan_only(a, L, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return SG_OK;
}

}  // namespace

int sg_flow_decide_batch(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, void* stream_) {
    if (!h) return SG_E_INVAL;
    const bool xshard = h->shard_world > 1 && h->n_lim > 0;
    if (xshard && !h->lim_x_armed)
        return fail(h, SG_E_UNSUPPORTED, "sharded namespace limiter: sg_lim_exchange must precede every flow batch");
    const bool armed = h->lim_x_armed;
    h->lim_x_armed = false;  // the exchange is consumed by this call, whatever its outcome
    if (n == 0 && !armed) return SG_OK;
    hipStream_t stream = (hipStream_t)stream_;
    // no requests on this shard, or a batch rejected before the device sees it: the shard's replica of the
    // namespace windows still walks the node's gathered arrivals (the other shards charge them too)
    const char* early = n == 0 ? "" : (!req || !out) ? "null buffer" : n > h->cfg.max_batch ? "batch larger than max_batch" : nullptr;
    if (early) {
        if (armed) {
            int rc = lim_plan_only(h, stream);
            if (rc) return rc;
        }
        if (n == 0) return SG_OK;
        return fail(h, (!req || !out) ? SG_E_INVAL : SG_E_CAPACITY, early);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    h->lim_x_armed = armed;  // read by flow_front
    int rc = enqueue_flow(h, req, n, out, stream, h->h_err, h->stats_on);
    h->lim_x_armed = false;
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (h->stats_on) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[4]);
        h->stats.total_ms = ms;
        (void)hipEventElapsedTime(&ms, h->ev[1], h->ev[2]);
        h->stats.sort_ms = ms;
        (void)hipEventElapsedTime(&ms, h->ev[2], h->ev[3]);
        h->stats.walk_ms = ms;
        h->stats.long_segments = h->h_long[0];
        h->stats.skipped_ranges = h->h_long[1];
    }
    return flow_status(h, *h->h_err);
}

void* sg_host_alloc(sg_handle* h, uint64_t bytes) {
    if (!h || bytes == 0) return nullptr;
    if (hipSetDevice(h->device) != hipSuccess) return nullptr;
    void* p = nullptr;  // the caller's from here on (sg_host_free)
    if (!PinnedAlloc::alloc(&p, bytes)) {
        fail(h, SG_E_NOMEM, "pinned host allocation");
        return nullptr;
    }
    return p;
}

void sg_host_free(sg_handle* h, void* p) {
    if (!h || !p) return;
    (void)hipSetDevice(h->device);
    PinnedAlloc::free(p);
}

// A pipelined batch of a shard with a namespace limiter consumes the armed exchange (sg_lim_exchange before every
// batch, as for sg_flow_decide_batch); an empty or refused batch walks it at once (the replica advances).
static int xshard_gate(sg_handle* h, uint64_t n, const char* early) {
    if (!(h->shard_world > 1 && h->n_lim > 0)) return early ? (n == 0 ? 1 : fail(h, SG_E_INVAL, early)) : SG_OK;
    if (!h->lim_x_armed)
        return fail(h, SG_E_UNSUPPORTED, "sharded namespace limiter: sg_lim_exchange must precede every flow batch");
    if (!early) return SG_OK;
    h->lim_x_armed = false;
    int rc = lim_plan_only(h, nullptr);
    if (rc) return rc;
    return n == 0 ? 1 : fail(h, n > h->cfg.max_batch ? SG_E_CAPACITY : SG_E_INVAL, early);
}

int sg_flow_submit(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, uint64_t* ticket) {
    if (!h || !ticket) return SG_E_INVAL;
    *ticket = 0;
    {
        const char* early = n == 0 ? "" : (!req || !out) ? "null buffer"
                            : n > h->cfg.max_batch ? "batch larger than max_batch" : nullptr;
        const int g = xshard_gate(h, n, early);
        if (g) return g == 1 ? SG_OK : g;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->s_comp) {  // first use: streams, per-slot device buffers, events, pinned error words
        HIP_TRY(h, hipStreamCreateWithFlags(h->s_in.put(), hipStreamNonBlocking));
        HIP_TRY(h, hipStreamCreateWithFlags(h->s_comp.put(), hipStreamNonBlocking));
        HIP_TRY(h, hipStreamCreateWithFlags(h->s_out.put(), hipStreamNonBlocking));
        for (auto& sl : h->slots) {
            if (!sl.d_req.alloc_bytes(sizeof(sg_req) * h->cfg.max_batch) ||
                !sl.d_out.alloc_bytes(sizeof(sg_result) * h->cfg.max_batch) ||
                !sl.h_err.alloc_bytes(sizeof(int)))
                return fail(h, SG_E_NOMEM, "host pipeline buffers");
            HIP_TRY(h, hipEventCreateWithFlags(sl.h2d.put(), hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(sl.comp.put(), hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(sl.d2h.put(), hipEventDisableTiming));
        }
    }
    sg_handle::Slot& sl = h->slots[h->next_ticket % kAsyncSlots];
    if (sl.ticket) {  // all slots in flight: complete the oldest (its status waits in `finished`)
        hipError_t e = hipEventSynchronize(sl.d2h);
        h->finished[sl.ticket] = e != hipSuccess ? fail(h, SG_E_DEVICE, hipGetErrorString(e)) : flow_status(h, *sl.h_err);
        sl.ticket = 0;
    }
    // H2D of this batch overlaps the previous batches' compute; the batch's front half (sort) overlaps the
    // previous batch's walkers, the walkers stay in submission order (the batches are time-ordered and share the
    // window state); D2H overlaps the next batch's compute
    HIP_TRY(h, hipMemcpyAsync(sl.d_req, req, sizeof(sg_req) * n, hipMemcpyHostToDevice, h->s_in));
    HIP_TRY(h, hipEventRecord(sl.h2d, h->s_in));
    int rc = enqueue_flow_pipelined(h, sl.d_req, n, sl.d_out, sl.h2d, sl.h_err, sl.comp);
    if (rc) return rc;
    HIP_TRY(h, hipStreamWaitEvent(h->s_out, sl.comp, 0));
    // results back on the copy engine (both directions of the link overlap: H2D of the next batch on s_in; a copy
    // kernel measured slower end to end, 2.45 vs 2.64 G decisions/s)
    HIP_TRY(h, hipMemcpyAsync(out, sl.d_out, sizeof(sg_result) * n, hipMemcpyDeviceToHost, h->s_out));
    HIP_TRY(h, hipEventRecord(sl.d2h, h->s_out));
    // (a slot is reused only after its batch completed: above, or when its ticket was collected)
    sl.ticket = h->next_ticket++;
    *ticket = sl.ticket;
    return SG_OK;
}

int sg_flow_enqueue(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, uint64_t* ticket) {
    if (!h || !ticket) return SG_E_INVAL;
    *ticket = 0;
    {
        const char* early = n == 0 ? "" : (!req || !out) ? "null buffer"
                            : n > h->cfg.max_batch ? "batch larger than max_batch" : nullptr;
        const int g = xshard_gate(h, n, early);
        if (g) return g == 1 ? SG_OK : g;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    sg_handle::DevTicket& d = h->dev[h->next_ticket % kDevSlots];
    if (!d.done) {
        if (!d.h_err.alloc_bytes(sizeof(int))) return fail(h, SG_E_NOMEM, "pinned error word");
        HIP_TRY(h, hipEventCreateWithFlags(d.done.put(), hipEventDisableTiming));
    }
    if (d.ticket) {  // every slot in flight: complete the oldest (its status waits in `finished`)
        hipError_t e = hipEventSynchronize(d.done);
        h->finished[d.ticket] = e != hipSuccess ? fail(h, SG_E_DEVICE, hipGetErrorString(e)) : ticket_status(h, d);
        d.ticket = 0;
    }
    int rc = enqueue_flow_pipelined(h, req, n, out, nullptr, d.h_err, d.done);
    if (rc) return rc;
    d.local = false;
    d.ticket = h->next_ticket++;
    *ticket = d.ticket;
    return SG_OK;
}

static int collect(sg_handle* h, uint64_t ticket, bool block) {
    if (!h) return SG_E_INVAL;
    if (ticket == 0) return 1;
    auto it = h->finished.find(ticket);
    if (it != h->finished.end()) {
        const int st = it->second;
        h->finished.erase(it);
        return st == SG_OK ? 1 : st;
    }
    for (auto& sl : h->slots) {
        if (sl.ticket != ticket) continue;
        hipError_t e = block ? hipEventSynchronize(sl.d2h) : hipEventQuery(sl.d2h);
        if (e == hipErrorNotReady) return 0;
        sl.ticket = 0;
        if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
        const int st = flow_status(h, *sl.h_err);
        return st == SG_OK ? 1 : st;
    }
    for (auto& d : h->dev) {
        if (d.ticket != ticket) continue;
        hipError_t e = block ? hipEventSynchronize(d.done) : hipEventQuery(d.done);
        if (e == hipErrorNotReady) return 0;
        d.ticket = 0;
        if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
        const int st = ticket_status(h, d);
        return st == SG_OK ? 1 : st;
    }
    return fail(h, SG_E_INVAL, "unknown or already collected ticket");
}

int sg_flow_poll(sg_handle* h, uint64_t ticket) { return collect(h, ticket, false); }

int sg_flow_wait(sg_handle* h, uint64_t ticket) {
    const int r = collect(h, ticket, true);
    return r == 1 ? SG_OK : r;
}

int sg_flow_decide_batch_host(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out) {
    if (!h) return SG_E_INVAL;
    // empty or refused before the device: the device entry point answers (and walks an armed exchange)
    if (n == 0 || n > h->cfg.max_batch || !req || !out) return sg_flow_decide_batch(h, n ? req : nullptr, n, out, nullptr);
    return host_batch(h, h->device, req, n, out,
                      [&](sg_req* d_req, sg_result* d_out) { return sg_flow_decide_batch(h, d_req, n, d_out, nullptr); });
}

// Envoy RLS (SentinelEnvoyRlsServiceImpl.shouldRateLimit, service/v3/SentinelEnvoyRlsServiceImpl.java:34-85): every
// descriptor of the batch one token request of one device batch (at most max_batch of them), then the per-request codes.
int sg_rls_should_rate_limit(sg_handle* h, const sg_rls_request* req, uint32_t n, const int32_t* desc_rule,
                             uint64_t n_desc, int32_t* overall, sg_rls_status* status) {
    if (!h) return SG_E_INVAL;
    if (n && (!req || !overall)) return fail(h, SG_E_INVAL, "null buffer");
    if (n_desc && (!desc_rule || !status)) return fail(h, SG_E_INVAL, "null buffer");
    for (uint32_t j = 0; j < n; ++j)
        if ((uint64_t)req[j].desc_begin + req[j].desc_count > n_desc)
            return fail(h, SG_E_INVAL, "a request's descriptors lie outside desc_rule");
    // SimpleClusterFlowChecker (flow/SimpleClusterFlowChecker.java:33-65) reads count * exceedCount and has neither a
    // namespace limiter nor AVG_LOCAL thresholds: refuse rules the cluster path would treat differently, and a batch
    // that would need several device batches (no partial commit), before any state changes
    uint64_t n_tok = 0;
    for (uint32_t j = 0; j < n; ++j) {
        if (req[j].hits_addend < 0) continue;
        n_tok += req[j].desc_count;
        for (uint32_t x = 0; x < req[j].desc_count; ++x) {
            const int32_t r = desc_rule[(uint64_t)req[j].desc_begin + x];
            if (r < 0 || (uint32_t)r >= h->K) continue;
            const sg_flow_rule& fr = h->rules[r];
            const int ns = fr.namespace_id;
            if (fr.threshold_type != SG_THRESHOLD_GLOBAL ||
                (ns >= 0 && (size_t)ns < h->ns_slot.size() && h->ns_slot[ns] >= 0))
                return fail(h, SG_E_UNSUPPORTED, "RLS rules are loaded GLOBAL in namespaces without a limiter "
                                                 "(SimpleClusterFlowChecker reads count * exceedCount only)");
        }
    }
    if (n_tok > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "more descriptors than max_batch");
    std::vector<sg_req> batch;
    std::vector<uint64_t> owner;  // descriptor of each token request
    batch.reserve(n_desc);
    owner.reserve(n_desc);
    for (uint64_t d = 0; d < n_desc; ++d) status[d] = sg_rls_status{0, 0, 0, 0};
    for (uint32_t j = 0; j < n; ++j) {
        const sg_rls_request& q = req[j];
        if (q.hits_addend < 0) {  // "acquireCount should be positive": onError, no token requests (:36-40)
            overall[j] = SG_RLS_ERROR;
            continue;
        }
        overall[j] = SG_RLS_OK;
        const int32_t acquire = q.hits_addend == 0 ? 1 : q.hits_addend;  // :41-44
        for (uint32_t x = 0; x < q.desc_count; ++x) {
            const uint64_t d = (uint64_t)q.desc_begin + x;
            const int32_t r = desc_rule[d];
            sg_req t{};
            t.ts_ms = q.ts_ms;
            t.key = (r < 0 || (uint32_t)r >= h->K) ? SG_KEY_NO_RULE : (uint32_t)r;  // checkToken: no rule
            t.acquire = acquire;
            batch.push_back(t);
            owner.push_back(d);
        }
    }
    std::vector<sg_result> res(batch.size());
    if (!batch.empty()) {
        h->slog_rls = true;  // SimpleClusterFlowChecker's log calls for this batch (the stat log's add reads it)
        const int rc = sg_flow_decide_batch_host(h, batch.data(), batch.size(), res.data());
        h->slog_rls = false;
        if (rc) return rc;
    }
    for (uint64_t x = 0; x < batch.size(); ++x) {
        const uint64_t d = owner[x];
        int32_t st = res[x].status;
        if (st == SG_STATUS_NO_RULE_EXISTS) st = SG_STATUS_OK;  // a descriptor without a rule passes (:55-58)
        sg_rls_status& o = status[d];
        o.code = st == SG_STATUS_OK ? SG_RLS_OK : SG_RLS_OVER_LIMIT;
        if (batch[x].key != SG_KEY_NO_RULE) {
            const double c = h->rules[batch[x].key].count;  // (int) rule.getCount(), JLS narrowing
            o.requests_per_unit = c >= 2147483647.0 ? INT32_MAX : (int32_t)c;
            o.limit_remaining = res[x].remaining;
            o.has_rule = 1;
        }
    }
    for (uint32_t j = 0; j < n; ++j) {
        if (overall[j] == SG_RLS_ERROR) continue;
        for (uint32_t x = 0; x < req[j].desc_count; ++x)
            if (status[(uint64_t)req[j].desc_begin + x].code != SG_RLS_OK) overall[j] = SG_RLS_OVER_LIMIT;
    }
    return SG_OK;
}

int sg_flow_read_state(sg_handle* h, uint32_t key, int64_t* starts, int64_t* counters, int64_t* occupy) {
    if (!h || key >= h->K || !starts || !counters || !occupy) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const int S = h->rule_tab[key].S;
    std::vector<Bucket> b(S);
    HIP_TRY(h, hipMemcpy(b.data(), h->d_ring + (size_t)key * h->stride, sizeof(Bucket) * S, hipMemcpyDeviceToHost));
    Occ o;
    HIP_TRY(h, hipMemcpy(&o, h->d_occ + key, sizeof(Occ), hipMemcpyDeviceToHost));
    for (int j = 0; j < S; ++j) {
        starts[j] = b[j].start;
        for (int e = 0; e < SG_NUM_EVENTS; ++e) counters[j * SG_NUM_EVENTS + e] = b[j].start == INT64_MIN ? 0 : b[j].c[e];
    }
    occupy[0] = o.pass;
    occupy[1] = o.pass_req;
    return SG_OK;
}

int sg_flow_export_state(sg_handle* h, int64_t* ring, uint64_t ring_words, int64_t* occ, uint64_t occ_words,
                         int32_t* stride) {
    if (!h || !stride) return SG_E_INVAL;
    *stride = h->stride;
    if (!ring) return SG_OK;
    const uint64_t rw = (uint64_t)h->K * h->stride * 8, ow = 2ull * h->K;
    if (ring_words < rw || !occ || occ_words < ow) return fail(h, SG_E_INVAL, "export buffers too small");
    if (h->K == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    static_assert(sizeof(Bucket) == 64 && sizeof(Occ) == 16, "export layout");
    HIP_TRY(h, hipMemcpy(ring, h->d_ring, rw * 8, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(occ, h->d_occ, ow * 8, hipMemcpyDeviceToHost));
    return SG_OK;
}

int sg_flow_import_state(sg_handle* h, const int64_t* ring, uint64_t ring_words, const int64_t* occ,
                         uint64_t occ_words) {
    if (!h || !ring || !occ) return SG_E_INVAL;
    const uint64_t rw = (uint64_t)h->K * h->stride * 8, ow = 2ull * h->K;
    if (ring_words != rw || occ_words != ow) return fail(h, SG_E_INVAL, "import size does not match the loaded rules");
    if (h->K == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    HIP_TRY(h, hipMemcpy(h->d_ring, ring, rw * 8, hipMemcpyHostToDevice));
    HIP_TRY(h, launch_hot_sync(h->d_ring, h->d_hot, (uint64_t)h->K * h->stride, 0));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->d_occ, occ, ow * 8, hipMemcpyHostToDevice));
    return SG_OK;
}

int sg_snapshot_metrics(sg_handle* h, int64_t now_ms, double* out, uint64_t cap) {
    if (!h || !out || cap < 2ull * h->K) return SG_E_INVAL;
    if (h->K == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    DevBuf<double> d_out;
    if (!d_out.alloc(2 * (size_t)h->K)) return fail(h, SG_E_DEVICE, "snapshot buffer: out of memory");
    hipError_t e1 = launch_snapshot(h->d_rules, h->d_ring, h->d_occ, h->K, h->stride, now_ms, d_out, 0);
    hipError_t e2 = e1 == hipSuccess ? hipMemcpy(out, d_out, sizeof(double) * 2 * h->K, hipMemcpyDeviceToHost) : e1;
    if (e2 != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e2));
    return SG_OK;
}

int sg_snapshot_metrics_device(sg_handle* h, int64_t now_ms, double* out_dev, uint64_t cap, void* stream) {
    if (!h || !out_dev || cap < 2ull * h->K) return SG_E_INVAL;
    if (h->K == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    HIP_TRY(h, launch_snapshot(h->d_rules, h->d_ring, h->d_occ, h->K, h->stride, now_ms, out_dev, (hipStream_t)stream));
    return SG_OK;
}

// The same snapshot ordered on the pipeline after every batch enqueued so far (sg_flow_enqueue / submit): the
// node-wide rollup of one simulated second can run while the next second's batches are being decided.
int sg_snapshot_metrics_enqueue(sg_handle* h, int64_t now_ms, double* out_dev, uint64_t cap, uint64_t* ticket) {
    if (!h || !out_dev || !ticket || cap < 2ull * h->K) return SG_E_INVAL;
    *ticket = 0;
    if (h->K == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = pipe_setup(h);
    if (rc) return rc;
    sg_handle::DevTicket& d = h->dev[h->next_ticket % kDevSlots];
    if (!d.done) {
        if (!d.h_err.alloc_bytes(sizeof(int))) return fail(h, SG_E_NOMEM, "pinned error word");
        HIP_TRY(h, hipEventCreateWithFlags(d.done.put(), hipEventDisableTiming));
    }
    if (d.ticket) {
        hipError_t e = hipEventSynchronize(d.done);
        h->finished[d.ticket] = e != hipSuccess ? fail(h, SG_E_DEVICE, hipGetErrorString(e)) : ticket_status(h, d);
        d.ticket = 0;
    }
    *d.h_err = 0;
    HIP_TRY(h, launch_snapshot(h->d_rules, h->d_ring, h->d_occ, h->K, h->stride, now_ms, out_dev, h->s_back));
    HIP_TRY(h, hipEventRecord(d.done, h->s_back));
    d.local = false;
    d.ticket = h->next_ticket++;
    *ticket = d.ticket;
    return SG_OK;
}

// A refused batch changes no state, table capacity included: the value slots its prep kernel claimed before the
// verdict (k_pprep, k_local_prep) hold no counter and are given back by rebuilding the sub-tables from a copy. On
// the refusal path only; the copy lives for this call. The refusal's code stands unless the device fails here: when
// there is no memory for the copy the claims stay (they cost free slots, never an answer) and the caller reports
// what it refused the batch for.
static int param_release_claims(sg_handle* h, hipStream_t stream) {
    if (!h->ptotal || h->ptab.empty()) return SG_OK;
    DevBuf<PSlot> old;
    if (!old.alloc(h->ptotal)) return SG_OK;
    HIP_TRY(h, hipMemcpyAsync(old, h->d_ptable, sizeof(PSlot) * h->ptotal, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(h, launch_param_rebuild(h->d_prules, (uint32_t)h->ptab.size(), h->d_ptable, old, h->ptotal, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return SG_OK;
}

// ParamFlowRuleManager.loadRules (…/param/ParamFlowRuleManager.java) → fresh ParameterMetric maps.
int sg_param_load_rules(sg_handle* h, const sg_param_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                        uint32_t n_hot) {
    if (!h || (!rules && n) || (!hot && n_hot)) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<PRule> tab(n);
    std::vector<sg_param_hot_item> hot_sorted(hot, hot + n_hot);
    uint64_t base = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const sg_param_rule& r = rules[i];
        if (!(r.count >= 0) || r.duration_sec <= 0) return fail(h, SG_E_INVAL, "invalid param rule");
        if ((uint64_t)r.hot_begin + r.hot_count > n_hot) return fail(h, SG_E_INVAL, "hot item range out of bounds");
        const int lg = r.capacity_log2 ? r.capacity_log2 : 20;
        if (lg < 1 || lg > 30) return fail(h, SG_E_INVAL, "capacity_log2 must be in [1, 30]");
        PRule& R = tab[i];
        R.token_count = (int64_t)r.count;  // (long) rule.getCount(); count is finite and >= 0 here
        if (r.count >= 9.2e18) R.token_count = INT64_MAX;
        R.duration_sec = r.duration_sec;
        R.burst = r.burst;
        R.behavior = r.behavior;
        R.max_queueing_ms = r.max_queueing_ms;
        R.hot_begin = r.hot_begin;
        R.hot_count = r.hot_count;
        R.table_base = base;
        R.table_mask = (1ull << lg) - 1;
        base += (1ull << lg) + 1;  // + the side slot for the value ~0
        std::sort(hot_sorted.begin() + r.hot_begin, hot_sorted.begin() + r.hot_begin + r.hot_count,
                  [](const sg_param_hot_item& x, const sg_param_hot_item& y) { return x.value < y.value; });
    }
    if (base >= (1ull << 32)) return fail(h, SG_E_UNSUPPORTED, "param tables larger than 2^32 slots");
    h->d_prules.reset();
    h->d_phot.reset();
    h->d_ptable.reset();
    h->ptotal = 0;
    if (n) {
        if (!h->d_prules.alloc_bytes(sizeof(PRule) * n) ||
            !h->d_ptable.alloc_bytes(sizeof(PSlot) * base))
            return fail(h, SG_E_NOMEM, "param table allocation");
        if (n_hot && !h->d_phot.alloc_bytes(sizeof(sg_param_hot_item) * n_hot))
            return fail(h, SG_E_NOMEM, "param hot items");
        HIP_TRY(h, hipMemcpy(h->d_prules, tab.data(), sizeof(PRule) * n, hipMemcpyHostToDevice));
        if (n_hot)
            HIP_TRY(h, hipMemcpy(h->d_phot, hot_sorted.data(), sizeof(sg_param_hot_item) * n_hot, hipMemcpyHostToDevice));
        HIP_TRY(h, launch_param_clear(h->d_ptable, base, 0));
        HIP_TRY(h, hipDeviceSynchronize());
    }
    h->prules.assign(rules, rules + n);
    h->ptab = tab;
    h->ptotal = base;
    return SG_OK;
}

// The handle's millisecond table for a batch of n requests, allocated at the first call. The hot-parameter and the
// pace batch share it: both are synchronous calls of this handle. False: out of device memory.
static bool ms_table_for(sg_handle* h, uint64_t n, MsTable* m) {
    if (!h->d_p_msb && (!h->d_p_msb.alloc_bytes(sizeof(uint32_t) * kMaxPeriods) ||
                        !h->d_p_mt.alloc_bytes(2 * sizeof(int64_t))))  // {t0, {np, zero word}}
        return false;
    if (!h->d_p_mbk && !h->d_p_mbk.alloc_bytes(sizeof(uint16_t) * kPcBuckets)) return false;
    m->msb = h->d_p_msb;
    m->mt0 = h->d_p_mt;
    m->mnp = reinterpret_cast<uint32_t*>(h->d_p_mt + 1);
    m->mbk = h->d_p_mbk;
    m->bshift = 0;
    while (((n - 1) >> m->bshift) >= kPcBuckets) ++m->bshift;
    return true;
}

int sg_param_decide_batch(sg_handle* h, const sg_param_req* req, uint64_t n, int32_t* pass, void* stream_) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !pass) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);  // the main workspace's segment lists may belong to an enqueued flow batch
    PArgs p{};
    p.req = req;
    p.out = pass;
    p.n = n;
    p.rec = h->ws[0].rec;
    p.rec_sorted = h->ws[0].rec_sorted;
    p.ibits = bits_for(h->cfg.max_batch > 1 ? h->cfg.max_batch - 1 : 1);
    p.imask = (1ull << p.ibits) - 1;
    p.rules = h->d_prules;
    p.n_rules = (uint32_t)h->ptab.size();
    p.hot = h->d_phot;
    p.table = h->d_ptable;
    p.total_slots = h->ptotal;
    p.err = h->ws[0].err;
    p.last_ts = h->d_plast_ts;
    p.long_list = h->ws[0].long_list;
    p.long_count = h->ws[0].counts;
    p.short_max = (h->cfg.flags & SG_FLAG_WAVE_ONLY) ? 0u
                  : (h->cfg.flags & SG_FLAG_SERIAL_ONLY) ? 0xFFFFFFFFu : h->param_short_max;
    const int gbits = bits_for(h->ptotal + 1);
    p.gshift = p.ibits + 8;  // {slot | acquire code : 8 | request index}
    if (p.gshift + gbits > 64) return fail(h, SG_E_UNSUPPORTED, "param tables x max_batch too large for 64-bit records");
    if (!ms_table_for(h, n, &p.ms)) return fail(h, SG_E_NOMEM, "param millisecond table");
    BatchArgs sg{};  // k_seg's lists in the main workspace; its error word: a zero word (the param flags are no errors)
    sg.err = reinterpret_cast<int*>(h->d_p_mt.get()) + 3;
    sg.short_list = h->ws[0].short_list;
    sg.short_count = h->ws[0].counts + 1;
    for (int c = 0; c < kClasses; ++c) sg.class_off[c] = h->class_off[c];
    HIP_TRY(h, hipMemsetAsync(h->ws[0].err, 0, sizeof(int), stream));
    HIP_TRY(h, hipMemsetAsync(h->ws[0].counts, 0, (1 + kClasses) * sizeof(uint32_t), stream));
    HIP_TRY(h, hipMemsetAsync(sg.err, 0, sizeof(int), stream));
    uint64_t* sorted = nullptr;
    HIP_TRY(h, launch_param_batch(p, sg, h->ws[0].rec, h->ws[0].rec_sorted, h->ws[0].hist, p.gshift, p.gshift + gbits, &sorted, stream,
                                  h->aux, h->fork, h->join));
    h->last_sorted = sorted;
    h->last_rec4_n = 0;
    HIP_TRY(h, hipMemcpyAsync(h->h_err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    const int err = *h->h_err & ~kErrNonPositive;
    if (err) {  // no walker ran: what k_pprep claimed goes back
        const int rc = param_release_claims(h, stream);
        if (rc) return rc;  // SG_E_DEVICE only
    }
    if (err & kErrTime)
        return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    if (err & kErrTableFull) return fail(h, SG_E_CAPACITY, "a param rule's value table is full");
    return SG_OK;
}

int sg_param_decide_batch_host(sg_handle* h, const sg_param_req* req, uint64_t n, int32_t* pass) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    return host_batch(h, h->device, req, n, pass,
                      [&](sg_param_req* d_req, int32_t* d_out) { return sg_param_decide_batch(h, d_req, n, d_out, nullptr); });
}

int sg_param_read_state(sg_handle* h, uint32_t rule, uint64_t value, int64_t* last_time, int64_t* tokens) {
    if (!h || rule >= h->ptab.size() || !last_time || !tokens) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    const PRule& R = h->ptab[rule];
    PSlot found{};
    bool hit = false;
    if (value == ~0ull) {  // the side slot
        HIP_TRY(h, hipMemcpy(&found, h->d_ptable + R.table_base + R.table_mask + 1, sizeof(PSlot), hipMemcpyDeviceToHost));
        hit = true;
    } else {
        // the probe sequence of param_slot, read in chunks of 64 slots
        uint64_t i = table_home(value, R.table_mask), seen = 0;
        PSlot chunk[64];
        while (!hit && seen <= R.table_mask) {
            const uint64_t m = std::min<uint64_t>(64, R.table_mask + 1 - i);  // up to the table's end
            HIP_TRY(h, hipMemcpy(chunk, h->d_ptable + R.table_base + i, sizeof(PSlot) * m, hipMemcpyDeviceToHost));
            bool empty = false;
            for (uint64_t j = 0; j < m && !hit && !empty; ++j) {
                if (chunk[j].value == value) {
                    found = chunk[j];
                    hit = true;
                } else if (chunk[j].value == ~0ull) {
                    empty = true;
                }
            }
            if (empty) break;
            seen += m;
            i = (i + m) & R.table_mask;
        }
    }
    if (!hit || !found.flags) return 0;
    *last_time = found.time;
    *tokens = found.tokens;
    return (int)found.flags;
}

// The reference's CacheMaps simply grow. Here the grown tables are allocated and filled beside the ones in force
// (grow.hip k_pgrow: every counted entry re-inserted under its rule's new mask, the side slots carried over) and
// swapped in at the end, so any refusal leaves the handle as it was. Every batch builds its arguments from
// d_prules / d_ptable / ptab / ptotal when it is called (sg_param_decide_batch, pslot_args for sg_pslot_* and the slot
// chain): once the enqueued work has drained nothing else holds the old tables.
int sg_param_resize(sg_handle* h, const int32_t* capacity_log2, uint32_t n) {
    if (!h) return SG_E_INVAL;
    std::vector<uint64_t> cur(h->ptab.size());
    for (size_t i = 0; i < cur.size(); ++i) cur[i] = h->ptab[i].table_mask;
    const GrowPlan plan = grow_plan_param(cur, capacity_log2, n, h->cfg.max_batch, h->ps_loaded);
    if (plan.code) return fail(h, plan.code, plan.why);
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    std::vector<PRule> tab = h->ptab;
    for (uint32_t i = 0; i < n; ++i) {
        tab[i].table_base = plan.base[i];
        tab[i].table_mask = plan.mask[i];
    }
    DevBuf<PRule> d_rules;
    DevBuf<PSlot> d_table;
    if (!d_rules.alloc(n) || !d_table.alloc(plan.total)) return fail(h, SG_E_NOMEM, "grown param tables");
    HIP_TRY(h, hipMemcpy(d_rules, tab.data(), sizeof(PRule) * n, hipMemcpyHostToDevice));
    HIP_TRY(h, launch_param_grow(h->d_prules, h->d_ptable, h->ptotal, d_rules, n, d_table, plan.total, 0));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_prules = std::move(d_rules);
    h->d_ptable = std::move(d_table);
    h->ptab = tab;
    h->ptotal = plan.total;
    for (uint32_t i = 0; i < n; ++i)
        if (capacity_log2[i]) h->prules[i].capacity_log2 = capacity_log2[i];
    return SG_OK;
}

int sg_param_table_used(sg_handle* h, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity) {
    if (!h || rule >= h->ptab.size()) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const PRule& R = h->ptab[rule];
    DevBuf<unsigned long long> d;
    if (!d.alloc(2)) return fail(h, SG_E_NOMEM, "table count buffer");
    unsigned long long got[2] = {0, 0};
    HIP_TRY(h, launch_param_used(h->d_ptable, R.table_base, R.table_mask + 1, d, 0));
    HIP_TRY(h, hipMemcpy(got, d, sizeof(got), hipMemcpyDeviceToHost));
    if (used) *used = got[0];
    if (live) *live = got[1];
    if (capacity) *capacity = R.table_mask + 1;
    return SG_OK;
}

namespace {

// The time order of a sweep at now_ms against the last timestamps `ts` (device words; null: that path is not set up)
// of the paths that read the swept tables. check: SG_E_TIME when one of them lies after now_ms; raise: each becomes
// max(itself, now_ms), so a later batch that starts before now_ms is refused as any out-of-order batch is. The raise
// comes before the swap: swept tables under a timestamp left behind could answer an older batch differently, while
// a raised timestamp over unswept tables (a copy that fails midway: SG_E_DEVICE) only refuses more.
int sweep_time_check(sg_handle* h, int64_t now_ms, int64_t* const* ts, int n) {
    if (now_ms < 0) return fail(h, SG_E_TIME, "now_ms must be >= 0");
    for (int k = 0; k < n; ++k) {
        if (!ts[k]) continue;
        int64_t last = -1;
        HIP_TRY(h, hipMemcpy(&last, ts[k], sizeof(last), hipMemcpyDeviceToHost));
        if (now_ms < last) return fail(h, SG_E_TIME, "now_ms lies before a batch that read the swept tables");
    }
    return SG_OK;
}

int sweep_time_raise(sg_handle* h, int64_t now_ms, int64_t* const* ts, int n) {
    for (int k = 0; k < n; ++k) {
        if (!ts[k]) continue;
        int64_t last = -1;
        HIP_TRY(h, hipMemcpy(&last, ts[k], sizeof(last), hipMemcpyDeviceToHost));
        if (last < now_ms) HIP_TRY(h, hipMemcpy(ts[k], &now_ms, sizeof(now_ms), hipMemcpyHostToDevice));
    }
    return SG_OK;
}

void sweep_stats_out(sg_sweep_stats* out, const unsigned long long* cnt) {
    if (!out) return;
    out->values_removed = cnt[0];
    out->claims_dropped = cnt[1];
    out->threads_removed = cnt[2];
    out->values_kept = cnt[3];
}

}  // namespace

// The other direction of sg_param_resize, by its mechanism: fresh tables of the same size beside the ones in force,
// filled by grow.hip's sweep kernels with every entry that is not idle at now_ms (table_sweep.h), and swapped in at the
// end. The thread counts of the ParamFlowSlot chain (when loaded) are rehashed the same way, entries at 0 left out.
int sg_param_sweep(sg_handle* h, int64_t now_ms, sg_sweep_stats* out) {
    if (!h) return SG_E_INVAL;
    if (h->ptab.empty()) return fail(h, SG_E_INVAL, "no param rules loaded");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    // sg_param_*, sg_pslot_* and the slot chain (its param lookups go through the same tables once pslot rules are in)
    int64_t* const ts[3] = {h->d_plast_ts.get(), h->d_ps_last_ts.get(), h->ps_loaded ? h->d_llast_ts.get() : nullptr};
    int rc = sweep_time_check(h, now_ms, ts, 3);
    if (rc) return rc;
    const uint32_t n = (uint32_t)h->ptab.size();
    const bool threads = h->ps_loaded && h->d_ps_tc;
    DevBuf<PSlot> d_table;
    DevBuf<PSThread> d_tc;
    DevBuf<unsigned long long> d_cnt;
    if (!d_table.alloc(h->ptotal) || (threads && !d_tc.alloc(h->ps_tc_slots)) || !d_cnt.alloc(4))
        return fail(h, SG_E_NOMEM, "swept param tables");
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIP_TRY(h, hipMemset(d_cnt, 0, sizeof(cnt)));
    HIP_TRY(h, launch_param_sweep(h->d_prules, n, h->d_phot, h->d_ptable, d_table, h->ptotal, now_ms, d_cnt, 0));
    if (threads) HIP_TRY(h, launch_tc_sweep(h->d_ps_tc, d_tc, h->ps_tc_slots, d_cnt, 0));
    HIP_TRY(h, hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipDeviceSynchronize());
    rc = sweep_time_raise(h, now_ms, ts, 3);
    if (rc) return rc;  // SG_E_DEVICE only; the tables in force are untouched, some timestamps may be raised
    h->d_ptable = std::move(d_table);
    if (threads) h->d_ps_tc = std::move(d_tc);
    sweep_stats_out(out, cnt);
    return SG_OK;
}

// --------------------------------------------------------------------- pace controller
// FlowRuleUtil.generateRater (core/.../flow/FlowRuleUtil.java:132-145) builds one RateLimiterController per
// CONTROL_BEHAVIOR_RATE_LIMITER rule; a rebuild starts every latestPassedTime at -1
// (RateLimiterController.java:33). FlowRuleUtil.isValidRule (:167-175) requires count >= 0.
int sg_pace_load_rules(sg_handle* h, const sg_pace_rule* rules, uint32_t n) {
    if (!h || (!rules && n)) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<PaceRule> tab(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!(rules[i].count >= 0)) return fail(h, SG_E_INVAL, "invalid pace rule: count must be >= 0");
        tab[i].count = rules[i].count;
        tab[i].max_queueing_ms = rules[i].max_queueing_ms;
        tab[i].pad = 0;
    }
    h->d_pace_rules.reset();
    h->d_pace_latest.reset();
    h->pace_tab.clear();
    if (!h->d_pace_last_ts) {
        const int64_t neg = INT64_MIN;
        if (!h->d_pace_last_ts.alloc_bytes(sizeof(int64_t))) return fail(h, SG_E_NOMEM, "pace state");
        HIP_TRY(h, hipMemcpy(h->d_pace_last_ts, &neg, sizeof(neg), hipMemcpyHostToDevice));
    }
    if (n) {
        if (!h->d_pace_rules.alloc_bytes(sizeof(PaceRule) * n) ||
            !h->d_pace_latest.alloc_bytes(sizeof(int64_t) * n))
            return fail(h, SG_E_NOMEM, "pace rule allocation");
        std::vector<int64_t> init(n, -1);
        HIP_TRY(h, hipMemcpy(h->d_pace_rules, tab.data(), sizeof(PaceRule) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_pace_latest, init.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
    }
    h->pace_tab = tab;
    return SG_OK;
}

int sg_pace_decide_batch(sg_handle* h, const sg_pace_req* req, uint64_t n, int32_t* wait, void* stream_) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !wait) return fail(h, SG_E_INVAL, "null buffer");
    if (!h->d_pace_last_ts) return fail(h, SG_E_INVAL, "sg_pace_load_rules first");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipSetDevice(h->device));
    PaceArgs p{};
    p.req = req;
    p.out = wait;
    p.n = n;
    p.rec = h->ws[0].rec;
    p.rec_sorted = h->ws[0].rec_sorted;
    p.ibits = bits_for(h->cfg.max_batch > 1 ? h->cfg.max_batch - 1 : 1);
    p.imask = (1ull << p.ibits) - 1;
    p.rules = h->d_pace_rules;
    p.n_rules = (uint32_t)h->pace_tab.size();
    p.latest = h->d_pace_latest;
    p.err = h->ws[0].err;
    p.last_ts = h->d_pace_last_ts;
    p.long_list = h->ws[0].long_list;
    p.long_count = h->ws[0].counts;
    p.short_list = h->ws[0].short_list;
    p.short_max = (h->cfg.flags & SG_FLAG_WAVE_ONLY) ? 0u
                  : (h->cfg.flags & SG_FLAG_SERIAL_ONLY) ? 0xFFFFFFFFu : h->pace_short_max;
    const int gbits = bits_for((uint64_t)p.n_rules + 1);
    p.gshift = p.ibits + 8;  // {rule | acquire code : 8 | request index}
    if (p.gshift + gbits > 64) return fail(h, SG_E_UNSUPPORTED, "pace rules x max_batch too large for 64-bit records");
    if (!ms_table_for(h, n, &p.ms)) return fail(h, SG_E_NOMEM, "pace millisecond table");
    HIP_TRY(h, hipMemsetAsync(h->ws[0].err, 0, sizeof(int), stream));
    for (int c = 0; c < kClasses; ++c) p.class_off[c] = h->class_off[c];
    HIP_TRY(h, hipMemsetAsync(h->ws[0].counts, 0, (1 + kClasses) * sizeof(uint32_t), stream));
    uint64_t* sorted = nullptr;
    HIP_TRY(h, launch_pace_batch(p, h->ws[0].rec, h->ws[0].rec_sorted, h->ws[0].hist, p.gshift, p.gshift + gbits, &sorted, stream,
                                 h->aux, h->fork, h->join));
    h->last_sorted = sorted;
    h->last_rec4_n = 0;
    HIP_TRY(h, hipMemcpyAsync(h->h_err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (*h->h_err & kErrTime)
        return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    return SG_OK;
}

int sg_pace_decide_batch_host(sg_handle* h, const sg_pace_req* req, uint64_t n, int32_t* wait) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !wait) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    return host_batch(h, h->device, req, n, wait,
                      [&](sg_pace_req* d_req, int32_t* d_out) { return sg_pace_decide_batch(h, d_req, n, d_out, nullptr); });
}

int sg_pace_read_state(sg_handle* h, uint32_t rule, int64_t* latest_passed_time) {
    if (!h || rule >= h->pace_tab.size() || !latest_passed_time) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(latest_passed_time, h->d_pace_latest + rule, sizeof(int64_t), hipMemcpyDeviceToHost));
    return SG_OK;
}

// --------------------------------------------------------------------- cluster hot-parameter tokens

// ClusterParamFlowRuleManager.loadRules → applyClusterParamRules (…/ClusterParamFlowRuleManager.java:337-360):
// a flowId that survives keeps its metric (and its window shape), the others start empty.
int sg_cparam_load_rules(sg_handle* h, const sg_cparam_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                         uint32_t n_hot, int32_t capacity_log2) {
    if (!h || (!rules && n) || (!hot && n_hot)) return SG_E_INVAL;
    if (n >= SG_KEY_BAD) return fail(h, SG_E_INVAL, "too many rules");
    const int lg = capacity_log2 ? capacity_log2 : 16;
    if (lg < 1 || lg > 28) return fail(h, SG_E_INVAL, "capacity_log2 must be in [1, 28]");
    HIP_TRY(h, hipSetDevice(h->device));
    std::unordered_map<int64_t, uint32_t> seen, old_index;
    for (uint32_t k = 0; k < h->cprules.size(); ++k) old_index.emplace(h->cprules[k].flow_id, k);
    std::vector<CPRule> tab(n);
    std::vector<int32_t> wls;  // distinct window lengths (the batch's period tables)
    std::vector<sg_param_hot_item> hs(hot, hot + n_hot);
    int stride = 1;
    uint64_t base = 0;
    const uint64_t per = (1ull << lg) + 1;  // + the side slot
    for (uint32_t i = 0; i < n; ++i) {
        const sg_cparam_rule& r = rules[i];
        if (r.flow_id <= 0 || !(r.count >= 0)) return fail(h, SG_E_INVAL, "invalid param rule");
        if (r.sample_count <= 0 || r.window_interval_ms <= 0 || r.window_interval_ms % r.sample_count != 0)
            return fail(h, SG_E_INVAL, "invalid window config");
        if (r.namespace_id < 0 || (size_t)r.namespace_id >= h->ns.size()) return fail(h, SG_E_INVAL, "unknown namespace");
        if ((uint64_t)r.hot_begin + r.hot_count > n_hot) return fail(h, SG_E_INVAL, "hot item range out of bounds");
        if (!seen.emplace(r.flow_id, i).second) return fail(h, SG_E_INVAL, "duplicate flowId");
        int S = r.sample_count, interval = r.window_interval_ms;
        auto it = old_index.find(r.flow_id);
        if (it != old_index.end()) {  // the existing metric keeps its window shape
            S = h->cptab[it->second].S;
            interval = h->cptab[it->second].S * h->cptab[it->second].wl;
        }
        if (S > SG_MAX_SAMPLE_COUNT) return fail(h, SG_E_UNSUPPORTED, "sampleCount > 64");
        CPRule& R = tab[i];
        R.count = r.count;
        R.isec = interval / 1000.0;
        R.S = S;
        R.wl = interval / S;
        R.global = r.threshold_type == SG_THRESHOLD_GLOBAL;
        R.connected = h->ns[r.namespace_id].connected_count;
        R.hot_begin = r.hot_begin;
        R.hot_count = r.hot_count;
        R.table_base = base;
        R.table_mask = (1ull << lg) - 1;
        {
            auto wit = std::find(wls.begin(), wls.end(), R.wl);
            if (wit == wls.end()) {
                if ((int)wls.size() == kMaxWl) return fail(h, SG_E_UNSUPPORTED, "more than 8 distinct param window lengths");
                wls.push_back(R.wl);
                wit = wls.end() - 1;
            }
            R.wl_idx = (int32_t)(wit - wls.begin());
            R.pad = 0;
        }
        base += per;
        stride = std::max(stride, S);
        std::sort(hs.begin() + r.hot_begin, hs.begin() + r.hot_begin + r.hot_count,
                  [](const sg_param_hot_item& x, const sg_param_hot_item& y) { return x.value < y.value; });
    }
    if (base >= (1ull << 32)) return fail(h, SG_E_UNSUPPORTED, "param tables larger than 2^32 slots");
    DevBuf<CPRule> d_rules;
    DevBuf<sg_param_hot_item> d_hot;
    DevBuf<uint64_t> d_keys;
    DevBuf<CPBucket> d_ring;
    if (n) {
        if (!d_rules.alloc(n) || !d_keys.alloc(base) || !d_ring.alloc(base * stride) || (n_hot && !d_hot.alloc(n_hot)))
            return fail(h, SG_E_NOMEM, "param table allocation");
        HIP_TRY(h, hipMemcpy(d_rules, tab.data(), sizeof(CPRule) * n, hipMemcpyHostToDevice));
        if (n_hot) HIP_TRY(h, hipMemcpy(d_hot, hs.data(), sizeof(sg_param_hot_item) * n_hot, hipMemcpyHostToDevice));
        HIP_TRY(h, launch_cp_clear(d_keys, d_ring, base, stride, 0));
        for (uint32_t i = 0; i < n; ++i) {  // surviving flowIds: move their sub-tables
            auto it = old_index.find(rules[i].flow_id);
            if (it == old_index.end()) continue;
            const CPRule& O = h->cptab[it->second];
            const uint64_t slots = std::min(O.table_mask, tab[i].table_mask) + 2;
            if (O.table_mask != tab[i].table_mask) return fail(h, SG_E_UNSUPPORTED, "capacity change of a live param rule");
            HIP_TRY(h, launch_cp_copy(h->d_cpkeys, h->d_cpring, O.table_base, h->cpstride, d_keys, d_ring, tab[i].table_base,
                                      stride, slots, O.S, 0));
        }
        HIP_TRY(h, hipDeviceSynchronize());
    }
    h->d_cprules = std::move(d_rules);
    h->d_cphot = std::move(d_hot);
    h->d_cpkeys = std::move(d_keys);
    h->d_cpring = std::move(d_ring);
    h->cprules.assign(rules, rules + n);
    h->cptab = tab;
    h->l_groups_stale = true;  // cluster-mode param rules group by these rules' flowIds and namespaces
    h->ps_groups_stale = true;
    h->cp_wls = wls;
    h->cptotal = base;
    h->cpstride = stride;
    if (!h->d_cplast_ts) {
        if (!h->d_cplast_ts.alloc_bytes(sizeof(int64_t))) return fail(h, SG_E_NOMEM, "ts");
        const int64_t neg = -1;
        HIP_TRY(h, hipMemcpy(h->d_cplast_ts, &neg, sizeof(neg), hipMemcpyHostToDevice));
    }
    const int frc = upload_cp_fid_table(h, rules, n);  // sg_codec_decode_param's flowId lookup
    if (frc) return frc;
    return slog_sync_fids(h);
}

static CPArgs cp_args(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values, uint64_t n_values,
                      sg_result* out) {
    CPArgs c{};
    c.req = req;
    c.values = values;
    c.n_values = n_values;
    c.out = out;
    c.n = n;
    c.ibits = bits_for(h->cfg.max_batch > 1 ? h->cfg.max_batch - 1 : 1);
    c.imask = (1ull << c.ibits) - 1;
    c.rules = h->d_cprules;
    c.n_rules = (uint32_t)h->cptab.size();
    c.hot = h->d_cphot;
    c.keys = h->d_cpkeys;
    c.ring = h->d_cpring;
    c.stride = h->cpstride;
    c.total_slots = h->cptotal;
    c.per = h->cptab.empty() ? 1 : h->cptab[0].table_mask + 2;
    c.err = h->ws[0].err;
    c.last_ts = h->d_cplast_ts;
    return c;
}

namespace {

// allowProceed → GlobalRequestLimiter.tryPass for the namespaces with a limiter (state shared with flow tokens):
// the limiter slot of every cluster param rule's namespace on the device (h->cp_any_lim: some rule has one)
int cp_rule_limiters(sg_handle* h, hipStream_t stream) {
    const uint32_t R = (uint32_t)h->cprules.size();
    std::vector<uint8_t> rl(R ? R : 1, 0xFF);
    bool any_lim = false;
    for (uint32_t k = 0; k < R; ++k) {
        const int ns = h->cprules[k].namespace_id;
        if (ns >= 0 && (size_t)ns < h->ns_slot.size() && h->ns_slot[ns] >= 0) {
            rl[k] = (uint8_t)h->ns_slot[ns];
            any_lim = true;
        }
    }
    h->cp_any_lim = any_lim;
    if (any_lim && (rl != h->cp_rule_lim_host || !h->d_cp_rule_lim)) {
        h->d_cp_rule_lim.reset();
        if (!h->d_cp_rule_lim.alloc_bytes(rl.size())) return fail(h, SG_E_NOMEM, "cparam limiter table");
        HIP_TRY(h, hipMemcpyAsync(h->d_cp_rule_lim, rl.data(), rl.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        h->cp_rule_lim_host = rl;
    }
    return SG_OK;
}

int cparam_batch(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values, uint64_t n_values,
                 sg_result* out, hipStream_t stream);

}  // namespace

// With a sharded namespace limiter (sg_set_shard, world > 1) every batch consumes an armed sg_lim_exchange over the
// node's param requests (sg_lim_arrivals_param); a batch rejected on the device, an empty one or one refused
// before the device still walks the armed arrivals (the shard's replica of the namespace windows advances).
int sg_cparam_decide_batch(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                           uint64_t n_values, sg_result* out, void* stream_) {
    if (!h) return SG_E_INVAL;
    const bool xshard = h->shard_world > 1 && h->n_lim > 0;
    if (xshard && !h->lim_x_armed)
        return fail(h, SG_E_UNSUPPORTED, "sharded namespace limiter: sg_lim_exchange must precede every param batch");
    const bool armed = h->lim_x_armed;
    h->lim_x_armed = false;  // consumed by this call, whatever its outcome
    hipStream_t stream = (hipStream_t)stream_;
    const char* early = n == 0 ? "" : (!req || !out || (!values && n_values)) ? "null buffer"
                        : n > h->cfg.max_batch ? "batch larger than max_batch"
                        : !h->d_cplast_ts ? "sg_cparam_load_rules first" : nullptr;
    if (early) {
        if (armed) {
            int rc = lim_plan_only(h, stream);
            if (rc) return rc;
        }
        if (n == 0) return SG_OK;
        return fail(h, n > h->cfg.max_batch ? SG_E_CAPACITY : SG_E_INVAL, early);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    h->lim_x_armed = armed;  // read by cparam_batch's limiter step
    const int rc = cparam_batch(h, req, n, values, n_values, out, stream);
    const bool unused = h->lim_x_armed;  // still set: the batch stopped before its limiter step
    h->lim_x_armed = false;
    if (unused && armed) {
        const int rc2 = lim_plan_only(h, stream);
        if (rc2 && !rc) return rc2;
    }
    return rc;
}

namespace {

// A cparam batch's error flags → return code, one order for every exit: what is wrong with the batch itself (time
// order, value ranges, window periods) comes before what the tables could not take of it.
int cparam_status(sg_handle* h, int err) {
    if (err & kErrTime) return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    if (err & kErrBounds)
        return fail(h, SG_E_INVAL, "a request's values lie outside the value array, overlap another's or go backwards");
    if (err & kErrPeriods) return fail(h, SG_E_UNSUPPORTED, "batch spans more than 65536 window or limiter periods");
    if (err & kErrTableFull) return fail(h, SG_E_CAPACITY, "a param rule's value table is full");
    return SG_OK;
}

// A batch that ends without its walk changes no state, table capacity included: the value slots k_cp_prep2 claimed
// before the verdict go back (the sub-tables rebuilt from a copy that lives for this call). When there is no memory
// for the copy the claims stay — they cost free slots, never an answer — and the caller's code stands.
int cparam_release_claims(sg_handle* h, const CPArgs& c, hipStream_t stream) {
    if (!h->cptotal) return SG_OK;
    DevBuf<uint64_t> okeys;
    DevBuf<CPBucket> oring;
    const size_t cells = (size_t)h->cptotal * h->cpstride;
    if (!okeys.alloc(h->cptotal) || !oring.alloc(cells)) return SG_OK;
    HIP_TRY(h, hipMemcpyAsync(okeys, h->d_cpkeys, sizeof(uint64_t) * h->cptotal, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(h, hipMemcpyAsync(oring, h->d_cpring, sizeof(CPBucket) * cells, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(h, launch_cp_rebuild(c, okeys, oring, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return SG_OK;
}

int cparam_batch(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values, uint64_t n_values,
                 sg_result* out, hipStream_t stream) {
    CPArgs c = cp_args(h, req, n, values, n_values, out);
    const uint64_t nv = n_values ? n_values : 1;
    const int gbits = bits_for(h->cptotal + 1);
    // value records {slot : gbits | multi : 1 | acquire code : 7 | request index or value position : idbits}
    const int pbits = 64 - gbits;
    const int idbits = pbits - 8;
    if (gbits > 32 || idbits < std::max(bits_for(nv), bits_for(n)))
        return fail(h, SG_E_UNSUPPORTED, "param tables x values too large for 64-bit records");
    // scratch sized for the batch's value positions
    if (nv > h->cp_val_cap) {
        h->cp_val_cap = 0;  // the whole group is laid out for one size: none of it counts until all of it is there
        h->d_cp_long.reset();
        h->d_cp_short.reset();
        if (!h->d_cp_items.alloc(9 * nv) || !h->d_cp_owner.alloc(nv) || !h->d_cp_pslot.alloc(nv) || !h->d_cp_chk.alloc(nv) ||
            !h->d_cp_rec.alloc(nv) || !h->d_cp_rec2.alloc(nv) || !h->d_cp_hist.alloc(radix_hist_words(nv)))
            return fail(h, SG_E_NOMEM, "cparam batch scratch");
        uint64_t off = 0;  // k_seg's class slices for nv records (as sg_create sizes them for max_batch)
        for (int c = 0; c < kClasses; ++c) {
            h->cp_class_off[c] = off;
            off += (c == 0 ? nv : nv / (kClassMax[c - 1] + 1)) + 1;
        }
        if (!h->d_cp_long.alloc(nv + 1) || !h->d_cp_short.alloc(off))
            return fail(h, SG_E_NOMEM, "cparam segment lists");
        h->cp_val_cap = nv;
    }
    if (!h->d_cp_slot_item.reserve(h->cptotal)) return fail(h, SG_E_NOMEM, "cparam slot items");
    if (!h->d_cp_counts && (!h->d_cp_counts.alloc_bytes(8 * sizeof(uint32_t)) ||
                            !h->d_cp_mlist.alloc_bytes(sizeof(uint32_t) * h->cfg.max_batch)))
        return fail(h, SG_E_NOMEM, "cparam batch scratch");
    if (!h->d_cp_assume && (!h->d_cp_assume.alloc_bytes(h->cfg.max_batch) ||
                            !h->d_cp_changed.alloc_bytes(sizeof(int) * (2 + (size_t)h->cp_max_rounds))))
        return fail(h, SG_E_NOMEM, "cparam batch scratch");
    int rc = cp_rule_limiters(h, stream);
    if (rc) return rc;
    const bool any_lim = h->cp_any_lim;
    const uint32_t R = (uint32_t)h->cprules.size();
    HIP_TRY(h, hipMemsetAsync(h->ws[0].err, 0, sizeof(int), stream));
    CPBatch b{};
    b.owner = h->d_cp_owner;
    b.chk = h->d_cp_chk;
    b.assume = h->d_cp_assume;
    b.rec = h->d_cp_rec;
    b.pbits = pbits;
    b.pmask = (1ull << pbits) - 1;
    b.idbits = idbits;
    b.idmask = (1ull << idbits) - 1;
    b.n_wl = (int)h->cp_wls.size();
    for (int w = 0; w < b.n_wl; ++w) b.wl[w] = h->cp_wls[w];
    if (!h->d_cp_bnd && (!h->d_cp_bnd.alloc_bytes(sizeof(uint32_t) * kMaxWl * kMaxPeriods) ||
                         !h->d_cp_p0.alloc_bytes(sizeof(int64_t) * kMaxWl) ||
                         !h->d_cp_np.alloc_bytes(sizeof(uint32_t) * kMaxWl)))
        return fail(h, SG_E_NOMEM, "cparam period tables");
    b.bnd = h->d_cp_bnd;
    b.p0 = h->d_cp_p0;
    b.np = h->d_cp_np;
    b.changed = h->d_cp_changed;
    b.pslot = h->d_cp_pslot;
    b.dflag = h->d_cp_items;                      // [nv] (items <= value positions)
    b.item_start = h->d_cp_items + nv;           // [nv]
    b.slot_item = h->d_cp_slot_item;
    b.item_end = h->d_cp_items + 6 * nv;         // [nv]
    b.item_slot = h->d_cp_items + 7 * nv;        // [nv]
    b.dq = h->d_cp_items + 8 * nv;               // [nv]
    b.dcap = (uint32_t)nv;                       // re-walk lists: 2 buffers x {long, short} x nv
    b.mlist = h->d_cp_mlist;
    b.mcount = h->d_cp_counts + 4;
    b.lim = any_lim ? 1 : 0;
    if (h->d_slog) {  // the stat log: the group fallback's replay notes where it blocked a request
        if (!h->d_slog_blk && !h->d_slog_blk.alloc(h->cfg.max_batch)) return fail(h, SG_E_NOMEM, "server log positions");
        b.slog_blk = h->d_slog_blk;
        HIP_TRY(h, hipMemsetAsync(b.slog_blk, 0xFF, sizeof(uint32_t) * n, stream));
    }
    HIP_TRY(h, hipMemsetAsync(h->d_cp_changed, 0, sizeof(int), stream));
    HIP_TRY(h, hipMemsetAsync(b.mcount, 0, sizeof(uint32_t), stream));
    HIP_TRY(h, launch_cp_prep2(c, b, stream));  // sets *changed iff a request has several values, lists them
    if (n_values == 0) {  // every request is BAD_REQUEST, NO_RULE_EXISTS or out of bounds (none reaches the limiter)
        HIP_TRY(h, launch_cp_finish_batch(c, stream));
        int err = 0;
        HIP_TRY(h, hipMemcpyAsync(&err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        h->cp_rounds = 0;
        return cparam_status(h, err);  // no value: nothing was claimed
    }
    uint64_t* sorted = nullptr;
    HIP_TRY(h, radix_sort_records(h->d_cp_rec, h->d_cp_rec2, nv, pbits, h->d_cp_hist, &sorted, stream, 64));
    HIP_TRY(h, launch_cp_order(c, b, sorted, nv, stream));
    if (any_lim) {  // after validation: a rejected batch leaves the limiter untouched
        BatchArgs a{};
        int kb = bits_for((uint64_t)R);
        if (kb < 1) kb = 1;
        a.n = n;
        a.rec = h->ws[0].rec;
        a.kshift = 64 - kb;
        a.K = R;
        a.bnd = h->ws[0].bnd;
        a.np = h->ws[0].np;
        a.p0 = h->ws[0].p0;
        a.out = out;
        a.err = h->ws[0].err;
        HIP_TRY(h, launch_cp_limprep(c, a, stream));
        LimArgs L{};
        L.n_lim = h->n_lim;
        L.wl_idx = 0;  // the cparam batch's 100 ms periods are row 0
        std::memcpy(L.qps, h->lim_qps, sizeof(L.qps));
        L.rule_lim = h->d_cp_rule_lim;
        L.slot = h->d_lim_slot;
        const uint64_t tiles = n / 4096 + 1;
        L.tile_tot = h->d_lim_tile;
        L.tile_off = h->d_lim_tile + tiles * kMaxLim;
        L.arrivals = h->d_lim_period;
        L.prefix = h->d_lim_period + (size_t)kMaxLim * kMaxPeriods;
        L.quota = h->d_lim_period + (size_t)2 * kMaxLim * kMaxPeriods;
        L.ring = h->d_lim_ring;
        if (h->lim_x_armed) {  // sharded: the node's gathered param arrivals (sg_lim_exchange)
            L.xg = h->lim_xg;
            L.ts = &req[0].ts_ms;
            L.ts_stride = sizeof(sg_cparam_req) / sizeof(int64_t);
            L.t_base = h->lim_xt;
            L.n_ms = h->lim_xn;
            L.world = h->shard_world;
            L.rank = h->shard_rank;
            h->lim_x_armed = false;
        }
        HIP_TRY(h, launch_limiter(a, L, stream));
    }
    // one lane per (rule, value) slot: k_seg's lists over the sorted value records
    BatchArgs sgm{};
    sgm.n = nv;
    sgm.rec_sorted = sorted;
    sgm.kshift = pbits;
    sgm.K = (uint32_t)h->cptotal;
    sgm.err = h->ws[0].err;
    sgm.long_list = h->d_cp_long;
    sgm.long_count = h->ws[0].counts;
    sgm.short_list = h->d_cp_short;
    sgm.short_count = h->ws[0].counts + 1;
    for (int cl = 0; cl < kClasses; ++cl) sgm.class_off[cl] = h->cp_class_off[cl];
    sgm.short_max = (h->cfg.flags & SG_FLAG_WAVE_ONLY) ? 0u
                    : (h->cfg.flags & SG_FLAG_SERIAL_ONLY) ? 0xFFFFFFFFu : h->cparam_short_max;
    HIP_TRY(h, hipMemsetAsync(h->ws[0].counts, 0, (1 + kClasses) * sizeof(uint32_t), stream));
    HIP_TRY(h, launch_seg(sgm, stream));
    // are there multi-value requests? (then the first walk saves the touched rings for the re-walks)
    uint32_t counts[1 + kClasses], np[kMaxWl] = {};
    int err = 0, has_multi = 0;
    HIP_TRY(h, hipMemcpyAsync(counts, h->ws[0].counts, sizeof(counts), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipMemcpyAsync(np, b.np, sizeof(uint32_t) * b.n_wl, hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipMemcpyAsync(&err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipMemcpyAsync(&has_multi, h->d_cp_changed, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    uint64_t touched = 0;
    for (uint32_t x : counts) touched += x;
    // work items: segment bounds and each touched slot's item (the walkers need the bounds in every round)
    if (!err && touched > 0) HIP_TRY(h, launch_cp_items(b, sgm, touched, stream));
    if (!err && has_multi && touched > 0) {
        // re-walk flags clear, the multi-value requests' list
        HIP_TRY(h, hipMemsetAsync(b.dflag, 0, sizeof(uint32_t) * touched, stream));
        HIP_TRY(h, launch_cp_mlist(c, b, stream));
        if (!h->d_cp_save.reserve((size_t)touched * h->cpstride)) {
            (void)cparam_release_claims(h, c, stream);  // the batch ends here: its claims go back
            return fail(h, SG_E_NOMEM, "cparam ring save area");
        }
        b.save = h->d_cp_save;  // the first walk saves the touched rings, re-walks restore the dirty ones
        // hot slots' ring at the opening of every window period, so a re-walk resumes at the first period a changed
        // outcome touches (batches of <= kCkMaxPeriods periods, within a memory cap)
        constexpr uint32_t kCkMaxPeriods = 64;
        constexpr uint64_t kCkMaxBytes = 1ull << 30;
        uint32_t ck_np = 0;
        for (int w = 0; w < b.n_wl; ++w) ck_np = std::max(ck_np, np[w]);
        const uint64_t ck = (uint64_t)counts[0] * ck_np * h->cpstride;
        if (counts[0] > 0 && ck_np <= kCkMaxPeriods && ck * sizeof(CPBucket) <= kCkMaxBytes) {
            if (!h->d_cp_ckpt.reserve(ck)) {
                (void)cparam_release_claims(h, c, stream);  // the batch ends here: its claims go back
                return fail(h, SG_E_NOMEM, "cparam ring checkpoints");
            }
            b.ckpt = h->d_cp_ckpt;
            b.ck_np = ck_np;
            HIP_TRY(h, hipMemsetAsync(b.dq, 0xFF, sizeof(uint32_t) * touched, stream));
        }
    }
    // saturated ranges of hot slots (pieces of <= 4096 records, each >= 256: at most 2 nv / 256 + 1)
    {
        const uint64_t cap = 2 * nv / 256 + 1;
        if (!h->d_cp_skips.reserve(cap) || !h->d_cp_skip_count.reserve(1)) {
            (void)cparam_release_claims(h, c, stream);  // the batch ends here: its claims go back
            return fail(h, SG_E_NOMEM, "cparam skip list");
        }
        b.skips = h->d_cp_skips;
        b.skip_count = h->d_cp_skip_count;
        b.skip_cap = (uint32_t)cap;
    }
    // rounds: walk every slot under the assumed multi-value outcomes, then recompute the outcomes
    const uint32_t kMaxRounds = h->cp_max_rounds;
    uint32_t round = 0;
    bool converged = false;
    if (!err && !has_multi) {  // single-value requests only: the slots are independent, one walk is exact
        HIP_TRY(h, hipMemsetAsync(b.skip_count, 0, sizeof(uint32_t), stream));
        HIP_TRY(h, launch_cp_walk2(c, b, sgm, stream, h->aux, h->fork, h->join));
        converged = true;
    }
    // Rounds are enqueued kChain at a time and the host reads their flags once per chain (a host round trip costs
    // ~90 us between rounds): round r's combine sets flag r (d_cp_changed[1 + r]) iff an outcome changed, and a round
    // after one that changed nothing returns at once (its lists are empty, combine and relist check the flags).
    // Each round's counters are zeroed on the device: dout_count by combine, skip_count by relist.
    constexpr uint32_t kChain = 3;
    if (!err && !converged) {
        HIP_TRY(h, hipMemsetAsync(h->d_cp_changed + 1, 0, sizeof(int) * (1 + (size_t)kMaxRounds), stream));
        HIP_TRY(h, hipMemsetAsync(b.skip_count, 0, sizeof(uint32_t), stream));
    }
    while (!err && !converged && round < kMaxRounds) {
        const uint32_t r0 = round, r1 = std::min(round + kChain, kMaxRounds);
        for (uint32_t r = r0; r < r1; ++r) {
            b.round = (int)r;
            // this round walks the lists the previous combine filled (buffer r & 1), and combine fills the other
            b.din = h->d_cp_items + (size_t)(2 + 2 * (r & 1)) * nv;
            b.din_count = h->d_cp_counts + 2 * (r & 1);
            b.dout = h->d_cp_items + (size_t)(2 + 2 * ((r + 1) & 1)) * nv;
            b.dout_count = h->d_cp_counts + 2 * ((r + 1) & 1);
            b.changed = h->d_cp_changed + 1 + r;
            b.changed_prev = r > 0 ? h->d_cp_changed + r : nullptr;
            HIP_TRY(h, launch_cp_walk2(c, b, sgm, stream, h->aux, h->fork, h->join));
            HIP_TRY(h, launch_cp_combine(c, b, sgm, touched, stream));
        }
        int changed[kChain] = {0, 0, 0};
        HIP_TRY(h, hipMemcpyAsync(changed, h->d_cp_changed + 1 + r0, sizeof(int) * (r1 - r0), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipMemcpyAsync(&err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        round = r1;
        for (uint32_t r = r0; r < r1; ++r) {
            if (!changed[r - r0]) {
                converged = true;
                round = r + 1;
                break;
            }
        }
    }
    if (!err && !converged) {  // rare: replay the groups of linked slots, each in arrival order, from the saved rings
        CPGroups g{};
        g.items = (uint32_t)touched;
        g.label = h->d_cp_items + 2 * nv;  // the re-walk lists are done with (the flags [0, nv) mark moving groups)
        g.flag = h->d_cp_items + 3 * nv;
        g.heads = h->d_cp_items + 4 * nv;
        g.changed = h->d_cp_changed;
        g.ent = h->d_cp_rec;               // the sorted value records are done with too
        g.ent_count = h->d_cp_counts + 5;
        g.head_count = h->d_cp_counts + 6;
        g.ibits = bits_for(n);
        g.all = round == 0 ? 1 : 0;
        uint32_t mreq = 0;
        HIP_TRY(h, hipMemcpyAsync(&mreq, b.mcount, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, launch_cpfb(c, b, g, 0, 0, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        for (int moved = 1; moved;) {  // labels strictly decrease: terminates
            HIP_TRY(h, hipMemsetAsync(g.changed, 0, sizeof(int), stream));
            HIP_TRY(h, launch_cpfb(c, b, g, 1, mreq, stream));
            HIP_TRY(h, hipMemcpyAsync(&moved, g.changed, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIP_TRY(h, hipStreamSynchronize(stream));
        }
        HIP_TRY(h, hipMemsetAsync(g.ent_count, 0, 2 * sizeof(uint32_t), stream));
        HIP_TRY(h, launch_cpfb(c, b, g, 2, mreq, stream));
        uint32_t m = 0;
        HIP_TRY(h, hipMemcpyAsync(&m, g.ent_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        HIP_TRY(h, radix_sort_records(h->d_cp_rec, h->d_cp_rec2, m, 0, h->d_cp_hist, &g.ent_sorted, stream,
                                      g.ibits + bits_for(touched)));
        HIP_TRY(h, launch_cpfb(c, b, g, 3, m, stream));
    }
    h->cp_rounds = converged ? (round ? round : 1) : kMaxRounds + 1;
    if (h->d_slog) HIP_TRY(h, launch_slog_add_param(c, b, slog_args(h), stream));  // behind the last writer of out
    HIP_TRY(h, launch_cp_finish_batch(c, stream));
    HIP_TRY(h, hipMemcpyAsync(&err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (err) {  // refused: no walker ran, and what k_cp_prep2 claimed goes back
        const int rc2 = cparam_release_claims(h, c, stream);
        if (rc2) return rc2;
    }
    return cparam_status(h, err);
}

}  // namespace

int sg_cparam_last_rounds(const sg_handle* h, uint32_t* rounds) {
    if (!h || !rounds) return SG_E_INVAL;
    *rounds = h->cp_rounds;
    return SG_OK;
}

int sg_cparam_decide_batch_host(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                                uint64_t n_values, sg_result* out) {
    if (!h) return SG_E_INVAL;
    // empty or refused before the device: the device entry point answers (and walks an armed exchange)
    if (n == 0 || n > h->cfg.max_batch || !req || !out || (!values && n_values))
        return sg_cparam_decide_batch(h, n ? req : nullptr, n, values, n_values, out, nullptr);
    HIP_TRY(h, hipSetDevice(h->device));
    uint64_t* d_vals = nullptr;
    if (!h->stage.get(2, n_values, d_vals)) return fail(h, SG_E_NOMEM, "host-path values");
    if (n_values) HIP_TRY(h, hipMemcpy(d_vals, values, 8 * n_values, hipMemcpyHostToDevice));
    return host_batch(h, h->device, req, n, out, [&](sg_cparam_req* d_req, sg_result* d_out) {
        return sg_cparam_decide_batch(h, d_req, n, d_vals, n_values, d_out, nullptr);
    });
}

int sg_cparam_read_sum(sg_handle* h, uint32_t rule, uint64_t value, int64_t now_ms, int64_t* sum) {
    if (!h || !sum || rule >= h->cptab.size()) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf<int64_t> d;
    if (!d.alloc(1)) return fail(h, SG_E_DEVICE, "read buffer: out of memory");
    CPArgs c = cp_args(h, nullptr, 0, nullptr, 0, nullptr);
    hipError_t e = launch_cp_read(c, rule, value, now_ms, d, 0);
    if (e == hipSuccess) e = hipMemcpy(sum, d, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    return SG_OK;
}

int sg_cparam_top_values(sg_handle* h, int64_t now_ms, uint32_t number, uint64_t* values, double* qps, uint32_t* counts) {
    if (!h || number == 0 || (!h->cptab.empty() && (!values || !qps || !counts))) return SG_E_INVAL;
    const uint32_t R = (uint32_t)h->cptab.size();
    if (R == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    CPArgs c = cp_args(h, nullptr, 0, nullptr, 0, nullptr);
    const uint64_t per = h->cptotal / R;
    DevBuf<CPTop> d_top;
    DevBuf<unsigned long long> d_cnt;
    if (!d_top.alloc(h->cptotal) || !d_cnt.alloc(1)) return fail(h, SG_E_NOMEM, "top values buffer");
    unsigned long long cnt = 0;
    hipError_t e = hipMemset(d_cnt, 0, sizeof(cnt));
    if (e == hipSuccess) e = launch_cp_top(c, now_ms, per, d_top, d_cnt, 0);
    if (e == hipSuccess) e = hipMemcpy(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost);
    std::vector<CPTop> top(cnt);
    if (e == hipSuccess && cnt) e = hipMemcpy(top.data(), d_top, sizeof(CPTop) * cnt, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    // per rule: count descending (the reference compares (int) casts of the counts), ties by value
    std::sort(top.begin(), top.end(), [](const CPTop& a, const CPTop& b) {
        if (a.rule != b.rule) return a.rule < b.rule;
        const int32_t ca = (int32_t)a.sum, cb = (int32_t)b.sum;
        if (ca != cb) return ca > cb;
        return a.value < b.value;
    });
    std::fill(counts, counts + R, 0u);
    for (const CPTop& t : top) {
        uint32_t& k = counts[t.rule];
        if (k >= number) continue;
        values[(size_t)t.rule * number + k] = t.value;
        qps[(size_t)t.rule * number + k] = (double)t.sum / h->cptab[t.rule].isec;  // count / getIntervalInSecond
        ++k;
    }
    return SG_OK;
}

// ClusterParamMetric's value → count maps simply grow. The grown keys and rings are allocated and filled beside the
// ones in force (grow.hip: a claim pass, then a coalesced move of the buckets) and swapped in at the end; cp_args
// builds every batch's arguments — the embedded token server's too (pslot_embed) — from the members written here, and
// the scratch sized by cptotal follows at the next batch (d_cp_slot_item.reserve).
int sg_cparam_resize(sg_handle* h, int32_t capacity_log2) {
    if (!h) return SG_E_INVAL;
    const uint32_t R = (uint32_t)h->cptab.size();
    const GrowPlan plan = grow_plan_cparam(R, R ? h->cptab[0].table_mask : 0, capacity_log2, h->cfg.max_batch);
    if (plan.code) return fail(h, plan.code, plan.why);
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    std::vector<CPRule> tab = h->cptab;
    for (uint32_t i = 0; i < R; ++i) {
        tab[i].table_base = plan.base[i];
        tab[i].table_mask = plan.mask[i];
    }
    DevBuf<CPRule> d_rules;
    DevBuf<uint64_t> d_keys;
    DevBuf<CPBucket> d_ring;
    DevBuf<uint32_t> d_map;
    if (!d_rules.alloc(R) || !d_keys.alloc(plan.total) || !d_ring.alloc((size_t)plan.total * h->cpstride) ||
        !d_map.alloc(h->cptotal))
        return fail(h, SG_E_NOMEM, "grown cluster param tables");
    HIP_TRY(h, hipMemcpy(d_rules, tab.data(), sizeof(CPRule) * R, hipMemcpyHostToDevice));
    CPArgs nc = cp_args(h, nullptr, 0, nullptr, 0, nullptr);
    nc.rules = d_rules;
    nc.keys = d_keys;
    nc.ring = d_ring;
    nc.total_slots = plan.total;
    nc.per = plan.mask[0] + 2;
    HIP_TRY(h, launch_cp_grow(nc, h->d_cprules, h->cptab[0].table_mask + 2, h->d_cpkeys, h->d_cpring, h->cptotal, d_map, 0));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_cprules = std::move(d_rules);
    h->d_cpkeys = std::move(d_keys);
    h->d_cpring = std::move(d_ring);
    h->cptab = tab;
    h->cptotal = plan.total;
    return SG_OK;
}

int sg_cparam_table_used(sg_handle* h, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity) {
    if (!h || rule >= h->cptab.size()) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const CPRule& R = h->cptab[rule];
    DevBuf<unsigned long long> d;
    if (!d.alloc(2)) return fail(h, SG_E_NOMEM, "table count buffer");
    unsigned long long got[2] = {0, 0};
    HIP_TRY(h, launch_cp_used(h->d_cpkeys, h->d_cpring, h->cpstride, R.S, R.table_base, R.table_mask + 1, d, 0));
    HIP_TRY(h, hipMemcpy(got, d, sizeof(got), hipMemcpyDeviceToHost));
    if (used) *used = got[0];
    if (live) *live = got[1];
    if (capacity) *capacity = R.table_mask + 1;
    return SG_OK;
}

// sg_cparam_resize at the size in force, rings with no bucket live at now_ms left out (grow.hip k_cpsweep_claim, then
// the move pass of the growth). The rules on the device stay: bases and masks do not change.
int sg_cparam_sweep(sg_handle* h, int64_t now_ms, sg_sweep_stats* out) {
    if (!h) return SG_E_INVAL;
    if (h->cptab.empty()) return fail(h, SG_E_INVAL, "no cluster param rules loaded");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    // sg_cparam_* and the embedded token server of the slot chain stamp the same word (pslot_embed, LArgs::ps)
    int64_t* const ts[1] = {h->d_cplast_ts.get()};
    int rc = sweep_time_check(h, now_ms, ts, 1);
    if (rc) return rc;
    DevBuf<uint64_t> d_keys;
    DevBuf<CPBucket> d_ring;
    DevBuf<uint32_t> d_map;
    DevBuf<unsigned long long> d_cnt;
    if (!d_keys.alloc(h->cptotal) || !d_ring.alloc((size_t)h->cptotal * h->cpstride) || !d_map.alloc(h->cptotal) ||
        !d_cnt.alloc(4))
        return fail(h, SG_E_NOMEM, "swept cluster param tables");
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIP_TRY(h, hipMemset(d_cnt, 0, sizeof(cnt)));
    CPArgs nc = cp_args(h, nullptr, 0, nullptr, 0, nullptr);
    nc.keys = d_keys;
    nc.ring = d_ring;
    HIP_TRY(h, launch_cp_sweep(nc, h->d_cpkeys, h->d_cpring, now_ms, d_map, d_cnt, 0));
    HIP_TRY(h, hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipDeviceSynchronize());
    rc = sweep_time_raise(h, now_ms, ts, 1);
    if (rc) return rc;  // SG_E_DEVICE only; the tables in force are untouched, some timestamps may be raised
    h->d_cpkeys = std::move(d_keys);
    h->d_cpring = std::move(d_ring);
    sweep_stats_out(out, cnt);
    return SG_OK;
}

// ------------------------------------------------------------------------------ local slot chain

namespace {
// LArgs::res_app on the device from h->l_res_app (nothing while the block log is off). The caller has drained the
// pipeline: no batch in flight reads the old table.
int blog_sync_apps(sg_handle* h) {
    if (!h->d_blog) return SG_OK;
    const size_t K = h->l_res_app.size();
    DevBuf<int32_t> d;
    if (!d.alloc(K ? K : 1)) return fail(h, SG_E_NOMEM, "block log limitApp table");
    if (K) HIP_TRY(h, hipMemcpy(d, h->l_res_app.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_lres_app = std::move(d);
    return SG_OK;
}
}  // namespace

int sg_local_load_rules(sg_handle* h, const sg_local_config* cfg, const sg_local_rule* rules, uint32_t n) {
    if (!h || !cfg || (!rules && n)) return SG_E_INVAL;
    if (n >= SG_KEY_BAD) return fail(h, SG_E_INVAL, "too many resources");
    if (cfg->sample_count <= 0 || cfg->interval_ms <= 0 || cfg->interval_ms % cfg->sample_count != 0)
        return fail(h, SG_E_INVAL, "invalid statistic window (SAMPLE_COUNT / INTERVAL)");
    if (cfg->sample_count > kMinuteS) return fail(h, SG_E_UNSUPPORTED, "SAMPLE_COUNT > 60");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    std::vector<LRule> tab(n);
    for (uint32_t i = 0; i < n; ++i) {
        const sg_local_rule& r = rules[i];
        if (r.flow_grade < -1 || r.flow_grade > 1) return fail(h, SG_E_INVAL, "flow grade");
        if (r.flow_grade >= 0 && !(r.flow_count >= 0)) return fail(h, SG_E_INVAL, "flow count must be >= 0");
        if (r.n_breakers < 0 || r.n_breakers > 2) return fail(h, SG_E_INVAL, "at most two degrade rules");
        LRule& L = tab[i];
        L = LRule{};
        L.flow_count = r.flow_count;
        L.flow_grade = r.flow_grade;
        L.nb = r.n_breakers;
        for (int j = 0; j < 2; ++j) {
            LBreakerRule& b = L.b[j];
            b = LBreakerRule{};
            b.stat_ms = 1;
            if (j >= r.n_breakers) continue;
            const sg_degrade_rule& d = r.breakers[j];
            // DegradeRuleManager.isValidRule (:183-202): what it drops is refused here, the rules in force stay
            bool valid = d.grade >= SG_DEGRADE_RT && d.grade <= SG_DEGRADE_EXCEPTION_COUNT && d.count >= 0 &&
                         d.time_window_sec > 0 && d.min_request_amount > 0 && d.stat_interval_ms > 0;
            if (valid && d.grade == SG_DEGRADE_RT)
                valid = d.slow_ratio_threshold >= 0 && d.slow_ratio_threshold <= 1;  // NaN fails both
            if (valid && d.grade == SG_DEGRADE_EXCEPTION_RATIO) valid = d.count <= 1;
            if (!valid) return fail(h, SG_E_INVAL, "invalid degrade rule");
            b.grade = d.grade;
            b.count = d.count;
            b.slow_ratio = d.slow_ratio_threshold;
            b.max_rt = java_round(d.count);  // ResponseTimeCircuitBreaker.java:52
            b.min_request = d.min_request_amount;
            b.recovery_ms = (int32_t)((uint32_t)d.time_window_sec * 1000u);  // int arithmetic, wraps
            b.stat_ms = d.stat_interval_ms;
        }
    }
    // window lengths of the period tables: the second window's bucket and the minute window's 1000 ms
    h->l_n_wl = 0;
    const int32_t wl2 = cfg->interval_ms / cfg->sample_count;
    h->l_wl[h->l_n_wl++] = wl2;
    h->l_wsec = 0;
    h->l_wmin = (wl2 == kMinuteWl) ? 0 : h->l_n_wl;
    if (wl2 != kMinuteWl) h->l_wl[h->l_n_wl++] = kMinuteWl;

    h->d_lrules.reset();
    h->d_lfrules.reset();
    h->d_lctl.reset();
    h->d_lauth.reset();  // fresh resources: the authority rules go as the flow rules do
    h->d_lauth_ids.reset();
    h->d_lhead.reset();
    h->d_lsec.reset();
    h->d_lbor.reset();
    h->d_lmin.reset();
    h->l_nodes = n;
    h->l_n_origins = 0;
    h->l_n_contexts = 0;
    h->l_has_cx = false;
    h->l_cluster_rules = false;
    h->l_base_cx.clear();
    h->l_relate.clear();
    h->l_cluster_refs.clear();
    h->l_groups_stale = false;
    h->l_rule_slot.clear();
    h->d_lnkeys.reset();
    h->d_lnvals.reset();
    h->d_ldyn.reset();
    h->l_pool_cap = h->l_pool_used = 0;
    h->l_epoch = 0;
    h->l_batches = 0;
    h->d_lgkey.reset();
    h->d_linbound.reset();  // every resource's entries EntryType.OUT until sg_local_set_entry_types
    h->l_inbound.clear();
    local_sys_drop(h);      // the system rules, the ENTRY_NODE and its tracking go with the resources
    h->l_ps_applied = 0;
    if (!h->d_lentry_fetch && (!h->d_lentry_fetch.alloc_bytes(sizeof(int64_t)) ||
                               !h->d_lentry_acc.alloc_bytes(sizeof(LBucket) * kMinuteS)))
        return fail(h, SG_E_NOMEM, "ENTRY_NODE state");
    {
        const int64_t neg1 = -1;  // StatisticNode.lastFetchTime of Constants.ENTRY_NODE
        HIP_TRY(h, hipMemcpy(h->d_lentry_fetch, &neg1, sizeof(neg1), hipMemcpyHostToDevice));
    }
    if (!h->d_llast_ts && !h->d_llast_ts.alloc_bytes(sizeof(int64_t))) return fail(h, SG_E_NOMEM, "ts");
    const int64_t neg = -1;
    HIP_TRY(h, hipMemcpy(h->d_llast_ts, &neg, sizeof(neg), hipMemcpyHostToDevice));
    h->lcfg = *cfg;
    h->ltab = tab;
    h->l_res_app.assign(n, SG_LIMIT_APP_DEFAULT);  // no flow rule list yet: every FlowException is the one rule's
    {
        const int rc = blog_sync_apps(h);
        if (rc) return rc;
    }
    if (n) {
        if (!h->d_lrules.alloc_bytes(sizeof(LRule) * n) || !h->d_lhead.alloc_bytes(sizeof(LHead) * n) ||
            !h->d_lsec.alloc_bytes(sizeof(LBucket) * (size_t)n * cfg->sample_count) ||
            !h->d_lbor.alloc_bytes(sizeof(LFuture) * (size_t)n * cfg->sample_count) ||
            !h->d_lmin.alloc_bytes(sizeof(LBucket) * (size_t)n * kMinuteS))
            return fail(h, SG_E_NOMEM, "local state allocation");
        HIP_TRY(h, hipMemcpy(h->d_lrules, tab.data(), sizeof(LRule) * n, hipMemcpyHostToDevice));
        LArgs L{};
        L.K = n;
        L.N = n;
        L.S = cfg->sample_count;
        L.head = h->d_lhead;
        L.sec = h->d_lsec;
        L.bor = h->d_lbor;
        L.minute = h->d_lmin;
        HIP_TRY(h, launch_local_init(L, 0));
        h->d_llast_fetch.reset();
        if (!h->d_llast_fetch.alloc_bytes(sizeof(int64_t) * n)) return fail(h, SG_E_NOMEM, "lastFetchTime");
        std::vector<int64_t> neg1(n, -1);  // StatisticNode.lastFetchTime = -1
        HIP_TRY(h, hipMemcpy(h->d_llast_fetch, neg1.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipDeviceSynchronize());
    }
    return SG_OK;
}

int sg_local_set_entry_types(sg_handle* h, const uint8_t* inbound, uint32_t n) {
    if (!h || (!inbound && n)) return SG_E_INVAL;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    if (n != h->ltab.size()) return fail(h, SG_E_INVAL, "one entry type per resource");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    std::vector<uint8_t> v(n);
    for (uint32_t k = 0; k < n; ++k) v[k] = inbound[k] ? 1 : 0;
    h->d_linbound.reset();
    if (n && !h->d_linbound.alloc_bytes(n)) return fail(h, SG_E_NOMEM, "entry types");
    if (n) HIP_TRY(h, hipMemcpy(h->d_linbound, v.data(), n, hipMemcpyHostToDevice));
    h->l_inbound = v;
    return local_sys_image(h);
}

namespace {
int local_metrics(sg_handle* h, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows, int raw,
                  bool device_out = false);
void local_group_keys(sg_handle* h, std::vector<uint32_t>& gkey);
}

int sg_local_metrics(sg_handle* h, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows) {
    return local_metrics(h, now_ms, out, cap, n_rows, 0);
}

int sg_local_metrics_raw(sg_handle* h, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows) {
    return local_metrics(h, now_ms, out, cap, n_rows, 1);
}

int sg_local_metrics_raw_device(sg_handle* h, int64_t now_ms, sg_metric_node* d_out, uint64_t cap, uint64_t* n_rows) {
    return local_metrics(h, now_ms, d_out, cap, n_rows, 1, true);
}

int sg_local_metrics_raw_enqueue(sg_handle* h, int64_t now_ms, sg_metric_node* d_out, uint64_t cap, uint64_t* d_count,
                                 void* stream_) {
    if (!h || !d_count || (!d_out && cap)) return SG_E_INVAL;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)stream_;
    if (h->ltab.empty()) {
        HIP_TRY(h, hipMemsetAsync(d_count, 0, sizeof(uint64_t), stream));
        return SG_OK;
    }
    int rc = pipe_setup(h);
    if (rc) return rc;
    if (!h->lm_done) {
        HIP_TRY(h, hipEventCreateWithFlags(h->lm_in.put(), hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(h->lm_done.put(), hipEventDisableTiming));
    }
    if ((!h->d_lm_cnt && !h->d_lm_cnt.alloc_bytes(sizeof(unsigned long long))) ||
        (!h->d_lm_gate && !h->d_lm_gate.alloc_bytes(sizeof(int))))
        return fail(h, SG_E_NOMEM, "metric row counter");
    LArgs L{};
    L.K = (uint32_t)h->ltab.size();
    L.minute = h->d_lmin;
    L.last_fetch = h->d_llast_fetch;
    L.inbound = h->d_linbound;
    L.entry_acc = h->d_lentry_acc;
    L.entry_fetch = h->d_lentry_fetch;
    // after the batches already enqueued (their back halves on s_back) and the caller's earlier work on `stream`
    // (e.g. the rollup still reading a previous call's rows); before every batch enqueued later
    hipStream_t s = h->s_back;
    HIP_TRY(h, hipEventRecord(h->lm_in, stream));
    HIP_TRY(h, hipStreamWaitEvent(s, h->lm_in, 0));
    // a capacity that covers every possible row (59 per resource, 60 of the ENTRY_NODE) needs no count pass: the
    // emit pass alone, its counter copied out
    const bool worst = cap >= (uint64_t)L.K * (kMinuteS - 1) + kMinuteS;
    for (int emit = worst ? 1 : 0; emit < 2; ++emit) {
        HIP_TRY(h, launch_entry_acc_reset(h->d_lentry_acc, s));
        HIP_TRY(h, hipMemsetAsync(h->d_lm_cnt, 0, sizeof(unsigned long long), s));
        const int* gate = emit && !worst ? h->d_lm_gate : nullptr;
        HIP_TRY(h, launch_local_metrics(L, now_ms, emit ? d_out : nullptr, h->d_lm_cnt, emit, 1, s, gate));
        if (h->d_linbound)
            HIP_TRY(h, launch_local_entry_rows(L, now_ms, emit ? d_out : nullptr, h->d_lm_cnt, emit, 1, s, gate));
        if (!emit) HIP_TRY(h, launch_metrics_gate(h->d_lm_cnt, cap, (unsigned long long*)d_count, h->d_lm_gate, s));
    }
    if (worst) HIP_TRY(h, hipMemcpyAsync(d_count, h->d_lm_cnt, sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipEventRecord(h->lm_done, s));
    HIP_TRY(h, hipStreamWaitEvent(stream, h->lm_done, 0));
    return SG_OK;
}

int sg_local_owners(sg_handle* h, uint32_t world, uint32_t* owner, uint32_t n) {
    if (!h || world == 0 || (!owner && n)) return SG_E_INVAL;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    const uint32_t K = (uint32_t)h->ltab.size();
    if (n != K) return fail(h, SG_E_INVAL, "owner buffer must hold one entry per resource");
    if (world > 1 && h->l_cluster_state == SG_CLUSTER_SERVER && h->n_lim > 0 && (h->l_cluster_rules || h->ps_cluster))
        return fail(h, SG_E_UNSUPPORTED, "an embedded token server with namespace limiters serves the node from one GPU");
    std::vector<uint32_t> gkey;
    local_group_keys(h, gkey);
    for (uint32_t k = 0; k < K; ++k) {  // splitmix64(group key) mod world (sentinel_amd/cluster.py local_owners)
        owner[k] = (uint32_t)(mix64((uint64_t)gkey[k]) % world);
    }
    return SG_OK;
}

namespace {
int local_metrics(sg_handle* h, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows, int raw,
                  bool device_out) {
    if (!h || !n_rows || (!out && cap)) return SG_E_INVAL;
    *n_rows = 0;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    if (h->ltab.empty()) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    LArgs L{};
    L.K = (uint32_t)h->ltab.size();
    L.minute = h->d_lmin;
    L.last_fetch = h->d_llast_fetch;
    L.inbound = h->d_linbound;
    L.entry_acc = h->d_lentry_acc;
    L.entry_fetch = h->d_lentry_fetch;
    // MetricTimerListener.run: the resources' rows, then the ENTRY_NODE's (counted first, then emitted: the emit
    // pass has the side effects)
    auto pass = [&](sg_metric_node* dst, unsigned long long* d_cnt, int emit) -> hipError_t {
        hipError_t e = launch_entry_acc_reset(h->d_lentry_acc, 0);
        if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), 0);
        if (e == hipSuccess) e = launch_local_metrics(L, now_ms, dst, d_cnt, emit, raw, 0);
        if (e == hipSuccess && h->d_linbound) e = launch_local_entry_rows(L, now_ms, dst, d_cnt, emit, raw, 0);
        return e;
    };
    if (!h->d_lm_cnt && !h->d_lm_cnt.alloc_bytes(sizeof(unsigned long long)))
        return fail(h, SG_E_NOMEM, "metric row counter");
    unsigned long long* d_cnt = h->d_lm_cnt;
    unsigned long long cnt = 0;
    hipError_t e = pass(nullptr, d_cnt, 0);
    if (e == hipSuccess) e = hipMemcpy(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    *n_rows = cnt;
    if (cnt > cap) return fail(h, SG_E_CAPACITY, "metric row buffer too small (*n_rows rows)");
    if (device_out) {  // the rows straight into the caller's device buffer, unsorted (the node rollup sorts)
        e = pass(out, d_cnt, 1);
        if (e == hipSuccess) e = hipStreamSynchronize(0);
        if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
        return SG_OK;
    }
    DevBuf<sg_metric_node> d_out;
    if (cnt && !d_out.alloc(cnt)) return fail(h, SG_E_NOMEM, "metric rows");
    e = pass(d_out, d_cnt, 1);
    if (e == hipSuccess && cnt) e = hipMemcpy(out, d_out, sizeof(sg_metric_node) * cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    std::sort(out, out + cnt, [](const sg_metric_node& a, const sg_metric_node& b) {  // the listener's TreeMap by time
        return a.timestamp != b.timestamp ? a.timestamp < b.timestamp : a.resource < b.resource;
    });
    return SG_OK;
}
}  // namespace

namespace {

// The ParamFlowSlot flags of the resources (LRule.ps: rules loaded by sg_pslot_load_rules for the resource) on the
// device rule image: a resource with param rules is walked by the full-chain walker.
int local_apply_params(sg_handle* h) {
    const uint64_t want = h->ps_loaded ? h->ps_gen : 0;
    if (h->l_ps_applied == want) return SG_OK;
    const uint32_t K = (uint32_t)h->ltab.size();
    std::vector<LRule> tab = h->ltab;
    bool any = false;
    for (uint32_t k = 0; k < K && h->ps_loaded && k < h->ps_res_rules.size(); ++k) {
        if (!h->ps_res_rules[k]) continue;
        tab[k].ps = 1;
        tab[k].cx = 1;
        any = true;
    }
    if (K) HIP_TRY(h, hipMemcpy(h->d_lrules, tab.data(), sizeof(LRule) * K, hipMemcpyHostToDevice));
    h->l_has_cx_ps = any;
    h->l_ps_applied = want;
    return local_sys_image(h);
}

// Node pool: a map with room for every key a batch of n events may add at load <= 1/2 (host rehash when it
// grows), the per-event slot buffer and the per-resource epochs.
int lnode_prepare(sg_handle* h, uint64_t n) {
    const uint32_t K = (uint32_t)h->ltab.size();
    if (!h->d_lev_node) {
        if (!h->d_lev_node.alloc_bytes(sizeof(uint2) * h->cfg.max_batch) ||
            !h->d_lnode_new.alloc_bytes(sizeof(uint32_t)) ||
            !h->h_lnode_new.alloc_bytes(sizeof(uint32_t)))
            return fail(h, SG_E_NOMEM, "node pool workspace");
    }
    if (!h->d_ldyn) {
        if (!h->d_ldyn.alloc_bytes(sizeof(uint32_t) * (K ? K : 1))) return fail(h, SG_E_NOMEM, "node pool");
        HIP_TRY(h, hipMemset(h->d_ldyn, 0, sizeof(uint32_t) * (K ? K : 1)));
        h->l_epoch = 0;
    }
    const uint64_t keys_per_event = (h->l_n_origins > 0 ? 1 : 0) + (h->l_n_contexts > 0 ? 1 : 0);
    const uint64_t need = 2 * ((uint64_t)h->l_pool_used + n * keys_per_event);
    if (h->d_lnkeys && need <= h->d_lnkeys.size()) return SG_OK;
    uint64_t cap = h->d_lnkeys ? h->d_lnkeys.size() : (1ull << 12);
    while (cap < need) cap <<= 1;
    std::vector<uint64_t> ok, nk(cap, 0);
    std::vector<uint32_t> ov, nv(cap, kNoNode);
    if (h->d_lnkeys) {  // rehash the existing keys
        ok.resize(h->d_lnkeys.size());
        ov.resize(h->d_lnkeys.size());
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(ok.data(), h->d_lnkeys, sizeof(uint64_t) * ok.size(), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(ov.data(), h->d_lnvals, sizeof(uint32_t) * ov.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ok.size(); ++i) {
            if (!ok[i]) continue;
            uint64_t j = lnode_hash(ok[i]) & (cap - 1);
            while (nk[j]) j = (j + 1) & (cap - 1);
            nk[j] = ok[i];
            nv[j] = ov[i];
        }
    }
    DevBuf<uint64_t> dk;
    DevBuf<uint32_t> dv;
    if (!dk.alloc(cap) || !dv.alloc(cap)) return fail(h, SG_E_NOMEM, "node pool map");
    hipError_t e = hipMemcpy(dk, nk.data(), sizeof(uint64_t) * cap, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dv, nv.data(), sizeof(uint32_t) * cap, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    h->d_lnkeys = std::move(dk);
    h->d_lnvals = std::move(dv);
    return SG_OK;
}

// Pool capacity >= used nodes: new node arrays (the resources, the old pool, empty nodes), geometric growth. Every
// growth copies the resources' nodes too (~4.2 KB each: 4 GB at 1M resources), so the pool starts at K / 16 nodes
// (~260 MB at 1M resources) and grows fourfold with room for twice the nodes in use.
int lnode_grow(sg_handle* h, uint64_t used) {
    if (used <= h->l_pool_cap) return SG_OK;
    // test aid: a failed growth. Read here, not in sg_create: tests/test_local_rules_gpu.py sets it on a live handle.
    if (const char* f = std::getenv("SG_TEST_POOL_FAIL"))
        if (std::atoi(f)) return fail(h, SG_E_NOMEM, "node pool (SG_TEST_POOL_FAIL)");
    const uint64_t K = h->ltab.size();
    uint64_t cap = std::max<uint64_t>({2ull * used, 4ull * h->l_pool_cap, 1024ull, K / 16});
    if (K + cap >= SG_KEY_BAD) cap = SG_KEY_BAD - 1 - K;
    if (K + used >= SG_KEY_BAD || cap < used) return fail(h, SG_E_CAPACITY, "too many origin / context nodes");
    const uint64_t N = K + cap, old = h->l_nodes;
    const int S = h->lcfg.sample_count;
    DevBuf<LHead> hd;
    DevBuf<LBucket> sec, mnt;
    DevBuf<LFuture> bor;
    if (!hd.alloc(N) || !sec.alloc(N * S) || !bor.alloc(N * S) || !mnt.alloc(N * kMinuteS))
        return fail(h, SG_E_NOMEM, "node pool");
    hipError_t e = hipMemcpy(hd, h->d_lhead, sizeof(LHead) * old, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(sec, h->d_lsec, sizeof(LBucket) * old * S, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(bor, h->d_lbor, sizeof(LFuture) * old * S, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(mnt, h->d_lmin, sizeof(LBucket) * old * kMinuteS, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) {
        LArgs L{};
        L.S = S;
        L.head = hd;
        L.sec = sec;
        L.bor = bor;
        L.minute = mnt;
        e = launch_local_init_range(L, old, N, 0);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, std::string("node pool growth: ") + hipGetErrorString(e));
    h->d_lhead = std::move(hd);
    h->d_lsec = std::move(sec);
    h->d_lbor = std::move(bor);
    h->d_lmin = std::move(mnt);
    h->l_nodes = (uint32_t)N;
    h->l_pool_cap = (uint32_t)cap;
    return SG_OK;
}

// The local path's batch buffers of one pipeline workspace: 0 the handle's own (every synchronous batch), 1 the
// flow pipeline's second workspace plus lws[1] (every other sg_local_enqueue batch).
struct LocalBufs {
    uint64_t* rec;
    uint64_t* rec_sorted;
    uint32_t* hist;
    uint32_t* bnd;
    int64_t* p0;
    uint32_t* np;
    int* err;
    uint32_t* long_list;
    uint32_t* counts;  // [1 + kClasses]: long count, short counts per class
    uint32_t* short_list;
    sg_handle::LocalWs* lw;
};

int local_bufs(sg_handle* h, int x, LocalBufs& b) {
    if (x == 0) {
        b = LocalBufs{h->ws[0].rec, h->ws[0].rec_sorted, h->ws[0].hist, h->ws[0].bnd, h->ws[0].p0, h->ws[0].np, h->ws[0].err, h->ws[0].long_list,
                      h->ws[0].counts, h->ws[0].short_list, &h->lws[0]};
    } else {
        const auto& w = h->ws[1];
        b = LocalBufs{w.rec, w.rec_sorted, w.hist, w.bnd, w.p0, w.np, w.err, w.long_list, w.counts, w.short_list, &h->lws[1]};
    }
    sg_handle::LocalWs& lw = h->lws[x];
    if (!lw.flags) {  // the local path's own buffers of the workspace (sized for max_batch)
        const uint64_t mb = h->cfg.max_batch;
        if (!lw.flags.alloc_bytes(sizeof(int)) ||
            !lw.exit_pos.alloc_bytes(sizeof(uint32_t) * (mb + 1)) ||
            !lw.exit_cnt.alloc_bytes(sizeof(uint32_t) * (mb / kLTile + 2)) ||
            !lw.skips.alloc(2 * mb / kSkipMin + 1) ||
            !lw.skip_count.alloc_bytes(sizeof(uint32_t)) ||
            !lw.cxw_next.alloc_bytes(sizeof(uint32_t)))
            return fail(h, SG_E_NOMEM, "local batch workspace");
    }
    return SG_OK;
}

BlogArgs blog_args(sg_handle* h) {
    BlogArgs b{};
    b.tab = h->d_blog;
    b.mask = h->d_blog.size() - 1;
    b.lost = h->d_blog_ctr;
    return b;
}

// The kernels' arguments of a local batch on workspace buffers b (node tracking set up by the caller).
int local_args(sg_handle* h, const LocalBufs& b, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
               const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values, sg_local_result* out,
               bool emb, LArgs& L, BatchArgs& sgm) {
    const uint32_t K = (uint32_t)h->ltab.size();
    int kbits = bits_for((uint64_t)K);
    if (kbits < 1) kbits = 1;
    const int ibits = bits_for(h->cfg.max_batch > 1 ? h->cfg.max_batch - 1 : 1);
    const int abits = 64 - kbits - ibits;
    if (abits < 4) return fail(h, SG_E_UNSUPPORTED, "resources x max_batch too large for 64-bit records");

    L = LArgs{};
    L.ev = ev;
    L.out = out;
    L.cxw = h->l_cxw;
    // the short classes whose segments all have >= l_cxw_min records: one lane walking a few hundred records event by
    // event outlasts a wave that decides their dead periods 64 at a time
    L.cxw_cls = kClasses;
    for (int c = kClasses - 1; c >= 0 && (c == 0 ? 1u : kClassMax[c - 1] + 1u) >= h->l_cxw_min; --c) L.cxw_cls = c;
    L.n = n;
    L.rec = b.rec;
    L.rec_sorted = b.rec_sorted;
    L.kshift = 64 - kbits;
    L.abits = abits;
    L.imask = (ibits >= 64) ? ~0ull : ((1ull << ibits) - 1);
    L.amask = (1ull << abits) - 1;
    L.aesc = (1ull << (abits - 3)) - 1;
    L.K = K;
    L.N = h->l_nodes;
    L.rules = h->d_lrules;
    L.frules = h->d_lfrules;
    L.ctl = h->d_lctl;
    L.n_origins = h->l_n_origins;
    L.head = h->d_lhead;
    L.sec = h->d_lsec;
    L.bor = h->d_lbor;
    L.minute = h->d_lmin;
    L.S = h->lcfg.sample_count;
    L.wl2 = h->lcfg.interval_ms / h->lcfg.sample_count;
    L.interval = h->lcfg.interval_ms;
    L.isec = h->lcfg.interval_ms / 1000.0;
    L.occupy_timeout = h->lcfg.occupy_timeout_ms;
    L.wsec = h->l_wsec;
    L.wmin = h->l_wmin;
    L.n_wl = h->l_n_wl;
    std::memcpy(L.wl, h->l_wl, sizeof(L.wl));
    L.bnd = b.bnd;
    L.p0 = b.p0;
    L.np = b.np;
    L.err = b.err;
    L.last_ts = h->d_llast_ts;
    L.ext = ext;
    L.n_contexts = h->l_n_contexts;
    L.gkey = h->d_lgkey;
    L.has_ps = h->ps_loaded ? 1 : 0;
    if (h->ps_loaded) {
        L.ps = pslot_args(h);
        L.ps.args = args;
        L.ps.n_args = args ? n_args : 0;
        L.ps.values = values;
        L.ps.n_values = values ? n_values : 0;
        const int prc = pslot_embed(h, L.ps, 0);  // cluster-mode param rules on the embedded token server
        if (prc) return prc;
        if (h->l_cxw) {
            if (!b.lw->pslot && !b.lw->pslot.alloc_bytes(sizeof(uint64_t) * h->cfg.max_batch))
                return fail(h, SG_E_NOMEM, "param lookups of the local batch");
            L.pslot = b.lw->pslot;
        }
    }
    if (emb) {  // the embedded token server: this handle's cluster flow state
        L.emb = 1;
        L.c3_rules = h->d_rules;
        L.c3_ring = h->d_ring;
        L.c3_hot = h->d_hot;
        L.c3_occ = h->d_occ;
        L.c3_stride = h->stride;
        L.c3_K = h->K;
        L.max_occ_ratio = h->cfg.max_occupy_ratio;
        L.c3_rule_lim = h->d_rule_lim;
        L.lim_ring = h->d_lim_ring;
        for (int j = 0; j < kMaxLim; ++j) L.lim_qps[j] = h->lim_qps[j];
        L.c3_last_ts = h->d_last_ts;
    }
    // AuthoritySlot: only an event with an origin id can be rejected, and a handle with no origin id declared
    // refuses such events (so the pipelined path, which needs l_n_origins == 0, never carries the table)
    if (h->d_lauth && h->l_n_origins > 0) {
        if (!b.lw->auth_rej && !b.lw->auth_rej.alloc_bytes(h->cfg.max_batch))
            return fail(h, SG_E_NOMEM, "authority verdicts of the local batch");
        L.auth = h->d_lauth;
        L.auth_ids = h->d_lauth_ids;
        L.auth_rej = b.lw->auth_rej;
    }
    if (h->d_blog) {  // the block log: cx_entry's side word and the per-resource limitApps
        L.blog_app = h->d_blog_app;
        L.res_app = h->d_lres_app;
    }
    L.flags = b.lw->flags;
    L.cxw_next = b.lw->cxw_next;
    if (h->l_cxw && (h->l_has_cx || h->l_has_cx_ps)) {  // the cx wave walker's sorted-order side words
        if (!b.lw->cxside && !b.lw->cxside.alloc_bytes(sizeof(CxSide) * h->cfg.max_batch))
            return fail(h, SG_E_NOMEM, "side words of the local batch");
        L.cxside = b.lw->cxside;
    }
    if (h->l_has_cx || h->l_has_cx_ps || h->l_n_contexts > 0) {
        if (!b.lw->cx_list && !b.lw->cx_list.alloc_bytes(sizeof(uint32_t) * (h->cfg.max_batch + 1)))
            return fail(h, SG_E_NOMEM, "cx segment list of the local batch");
        L.cx_list = b.lw->cx_list;
        L.cx_count = b.lw->cx_list + h->cfg.max_batch;
    }
    L.exit_pos = b.lw->exit_pos;
    L.exit_cnt = b.lw->exit_cnt;
    L.skips = b.lw->skips;
    L.skip_count = b.lw->skip_count;
    L.skip_cap = (uint32_t)b.lw->skips.size();
    L.hist0 = b.hist;
    L.hist0_bits = radix_digit_bits(64 - L.kshift);

    sgm = BatchArgs{};  // segment lists (k_seg)
    sgm.dbg = h->dbg;
    sgm.dbg_ctr = h->d_dbg;
    sgm.n = n;
    sgm.rec_sorted = b.rec_sorted;
    sgm.kshift = L.kshift;
    sgm.K = K;
    sgm.err = b.err;
    sgm.long_list = b.long_list;
    sgm.long_count = b.counts;
    sgm.short_list = b.short_list;
    sgm.short_count = b.counts + 1;
    for (int c = 0; c < kClasses; ++c) sgm.class_off[c] = h->class_off[c];
    // Lane / wave walker split: with many events per resource (n >= 256 K) the lanes' longest class (65..256 events)
    // sets the lane walker's end and the wave walker takes those segments sooner (C2, 10k resources: 0.88 → 0.82
    // ms/step); with few (C5, 1M resources) 256 stays best (1.97 against 2.28 ms at 64). SG_SHORT_MAX overrides.
    const uint32_t lsplit = (!h->short_max_env && (uint64_t)n >= 256ull * K) ? 64u : h->short_max;
    sgm.short_max = (h->cfg.flags & SG_FLAG_WAVE_ONLY) ? 0u : (h->cfg.flags & SG_FLAG_SERIAL_ONLY) ? 0xFFFFFFFFu : lsplit;

    return SG_OK;
}

// Front half of a local batch on `stream`: validation, default results and packed records (k_local_prep, with the
// first sort digit's histogram), the stable sort by resource, the segment lists and the exit positions. Reads no
// state a walker writes (with L.defer_last the first timestamp's check waits for the back half).
int local_front(sg_handle* h, LArgs& L, BatchArgs& sgm, hipStream_t stream) {
    HIP_TRY(h, hipMemsetAsync(L.err, 0, sizeof(int), stream));
    HIP_TRY(h, hipMemsetAsync(sgm.long_count, 0, (1 + kClasses) * sizeof(uint32_t), stream));
    HIP_TRY(h, hipMemsetAsync(L.flags, 0, sizeof(int), stream));
    HIP_TRY(h, hipMemsetAsync(L.skip_count, 0, sizeof(uint32_t), stream));
    L.csum0 = nullptr;
    if (radix_csum_atomic()) {
        L.csum0 = radix_csum(L.hist0, L.n, L.hist0_bits);
        HIP_TRY(h, hipMemsetAsync(L.csum0, 0, radix_csum_bytes(L.n, L.hist0_bits), stream));
    }
    HIP_TRY(h, launch_local_prep(L, stream));
    return SG_OK;
}

// count_exits: k_seg also counts the exit records per exit tile (k_lexit_count's pass, pipelined path)
int local_sort(sg_handle* h, LArgs& L, BatchArgs& sgm, uint64_t* spare, hipStream_t stream, bool count_exits = false) {
    uint64_t* sorted = nullptr;
    HIP_TRY(h, radix_sort_records(L.rec, spare, L.n, L.kshift, L.hist0, &sorted, stream, 64, true,
                                  L.csum0 != nullptr));
    L.rec_sorted = sorted;
    sgm.rec_sorted = sorted;
    if (count_exits) {
        HIP_TRY(h, hipMemsetAsync(L.exit_cnt, 0, sizeof(uint32_t) * (L.n / kLTile + 2), stream));
        sgm.exit_cnt = L.exit_cnt;
        sgm.exit_amask = L.amask;
    }
    HIP_TRY(h, launch_seg(sgm, stream));
    return SG_OK;
}

// StatisticSlot around ParamFlowSlot → FlowSlot → DegradeSlot for a time-ordered batch (ext nullable).
int local_decide(sg_handle* h, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n, const sg_pslot_arg* args,
                 uint64_t n_args, const uint64_t* values, uint64_t n_values, sg_local_result* out, void* stream_) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!ev || !out) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    if (h->l_groups_stale && (h->l_cluster_rules || h->ps_cluster)) {
        const int grc = local_apply_groups(h);
        if (grc) return grc;
    }
    int prc = local_apply_params(h);
    if (prc) return prc;
    const bool emb = h->l_cluster_state == SG_CLUSTER_SERVER && h->l_cluster_rules;
    if (emb && h->shard_world > 1 && h->n_lim > 0)
        return fail(h, SG_E_UNSUPPORTED, "an embedded token server on a sharded handle with namespace limiters: the "
                                         "limiter exchange covers flow and param batches only");
    LocalBufs b;
    int rc = local_bufs(h, 0, b);
    if (rc) return rc;
    LArgs L;
    BatchArgs sgm;
    rc = local_args(h, b, ev, ext, n, args, n_args, values, n_values, out, emb, L, sgm);
    if (rc) return rc;
    const uint32_t K = L.K;
    // SystemSlot: with ENTRY_NODE tracked and some resource inbound, the batch is either proven clear of system
    // blocks (k_sys_scan; the normal image and walkers, ENTRY_NODE folded in afterwards by k_sys_apply_*) or walks the
    // system image, whose one key group decides every inbound event in order against ENTRY_NODE in memory. The
    // verdict is read here, before the records are built: they carry the chosen image's keys.
    if (h->l_sys_track && h->shard_world > 1)
        return fail(h, SG_E_UNSUPPORTED, "system rules on a sharded handle: ENTRY_NODE spans the shards");
    h->l_sys_path = 0;
    bool sys_serial = false, sys_apply = false;
    SysArgs SA{};
    if (h->l_sys_track) {
        h->l_sys_path = 1;
        h->l_sys_first = 0xFFFFFFFFu;
    }
    if (h->l_sys_track && h->l_sys_image) {
        SA.ev = ev;
        SA.out = out;
        SA.n = n;
        SA.K = K;
        SA.inbound = h->d_linbound;
        SA.sys = h->d_lsys;
        SA.S = L.S;
        SA.wl = L.wl2;
        SA.isec = L.isec;
        SA.pb = h->d_lsys_pb;
        SA.err = L.err;
        const LSysConf& c = h->l_sys_conf;
        const bool armed = c.check && ((c.load_set && h->l_sys_load > c.highest_load) ||
                                       (c.cpu_set && h->l_sys_cpu > c.highest_cpu));
        if (h->l_sys_force || armed) {
            sys_serial = true;
        } else if (c.check) {
            HIP_TRY(h, launch_sys_scan(SA, stream));
            HIP_TRY(h, hipMemcpyAsync(h->h_lsys_verdict, &((LSys*)h->d_lsys)->unproven, 2 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, stream));
            HIP_TRY(h, hipStreamSynchronize(stream));
            sys_serial = h->h_lsys_verdict[0] != 0;
            h->l_sys_first = h->h_lsys_verdict[1];
        }
        if (sys_serial) {
            L.rules = h->d_lrules_sys;
            L.gkey = h->d_lgkey_sys;
            L.sys = h->d_lsys;
            L.inbound = h->d_linbound;
            h->l_sys_path = 2;
        }
        sys_apply = !sys_serial;
    }
    const bool track = h->l_n_origins > 0 || h->l_n_contexts > 0;
    if (track) {
        const int rc = lnode_prepare(h, n);
        if (rc) return rc;
        L.nkeys = h->d_lnkeys;
        L.nvals = h->d_lnvals;
        L.nmask = h->d_lnkeys.size() - 1;
        L.node_base = K + h->l_pool_used;
        L.node_new = h->d_lnode_new;
        L.ev_node = h->d_lev_node;
        L.dyn = h->d_ldyn;
        if (++h->l_epoch == 0) {  // the epochs wrapped: no resource may match a stale one
            HIP_TRY(h, hipMemset(h->d_ldyn, 0, sizeof(uint32_t) * (K ? K : 1)));
            h->l_epoch = 1;
        }
        L.epoch = h->l_epoch;
        L.track_ctx = h->l_n_contexts > 0 ? 1 : 0;
    }

    if (h->stats_on) HIP_TRY(h, hipEventRecord(h->ev[0], stream));
    rc = local_front(h, L, sgm, stream);
    if (rc) return rc;
    if (track) {  // the batch's new pool nodes (only for a batch that passed validation), then room for them
        HIP_TRY(h, hipMemsetAsync(h->d_lnode_new, 0, sizeof(uint32_t), stream));
        HIP_TRY(h, launch_lnode_assign(L, stream));
        HIP_TRY(h, hipMemcpyAsync(h->h_lnode_new, h->d_lnode_new, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        const uint64_t used = (uint64_t)h->l_pool_used + *h->h_lnode_new;
        // The map now holds the batch's new nodes (indices below K + used), so the allocator moves past them even
        // when the pool cannot grow now: this batch is then refused, and the next one grows the pool before any
        // walker reads a node. Nodes a refused batch created stay, with zero counts (NodeSelectorSlot and
        // ClusterBuilderSlot create them at entry, before any rule is checked).
        const int rc = lnode_grow(h, used);
        h->l_pool_used = (uint32_t)used;
        if (rc) {
            if (L.pslot) (void)param_release_claims(h, stream);  // refused before any walker: the claims go back
            return rc;
        }
        L.N = h->l_nodes;
        L.head = h->d_lhead;
        L.sec = h->d_lsec;
        L.bor = h->d_lbor;
        L.minute = h->d_lmin;
    }
    if (h->stats_on) HIP_TRY(h, hipEventRecord(h->ev[1], stream));
    rc = local_sort(h, L, sgm, b.rec_sorted, stream);
    if (rc) return rc;
    h->last_sorted = L.rec_sorted;
    h->last_rec4_n = 0;
    if (h->stats_on) HIP_TRY(h, hipEventRecord(h->ev[2], stream));
    HIP_TRY(h, launch_local_walk(L, sgm, h->l_has_cx || h->l_has_cx_ps || track || sys_serial, h->aux, stream, h->fork,
                                 h->join));
    if (sys_apply) {
        SA.auth_rej = L.auth_rej;
        HIP_TRY(h, launch_sys_apply(SA, stream));
    }
    if (h->stats_on) HIP_TRY(h, hipEventRecord(h->ev[3], stream));
    if (h->d_blog) HIP_TRY(h, launch_blog_add(L, blog_args(h), stream));  // LogSlot, behind the decisions
    HIP_TRY(h, hipMemcpyAsync(h->h_err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (h->stats_on) {
        HIP_TRY(h, hipMemcpyAsync(h->h_long, h->ws[0].counts, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipMemcpyAsync(h->h_long + 1, L.skip_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipEventRecord(h->ev[4], stream));
    }
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (h->stats_on) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[4]);
        h->stats.total_ms = ms;
        (void)hipEventElapsedTime(&ms, h->ev[1], h->ev[2]);
        h->stats.sort_ms = ms;
        (void)hipEventElapsedTime(&ms, h->ev[2], h->ev[3]);
        h->stats.walk_ms = ms;
        h->stats.long_segments = h->h_long[0];
        h->stats.skipped_ranges = h->h_long[1];
    }
    rc = local_status(h, *h->h_err);
    if (rc) {  // the value slots k_local_prep claimed for the refused batch's entries go back
        if (L.pslot) (void)param_release_claims(h, stream);  // (the refusal's code and message stand)
        return rc;
    }
    ++h->l_batches;
    return SG_OK;
}

// Whether a local batch may go on the pipeline: no node tracking (the pool grows with a host round trip inside the
// batch), no embedded token server (it shares the cluster flow state and its last timestamp), no rule tables
// waiting to be uploaded, no per-batch phase timing. Other batches drain the pipeline and run synchronously.
bool local_pipelinable(sg_handle* h) {
    const uint64_t want = h->ps_loaded ? h->ps_gen : 0;
    return h->l_n_origins == 0 && h->l_n_contexts == 0 && h->l_cluster_state != SG_CLUSTER_SERVER && !h->l_sys_track &&
           !(h->l_groups_stale && (h->l_cluster_rules || h->ps_cluster)) && h->l_ps_applied == want && !h->stats_on;
}

// One local batch on the pipeline, as enqueue_flow_pipelined: its front half (validation, sort, segments, exit
// positions) on s_front waits for the back half of the batch two back (same workspace) and runs beside the previous
// batch's walkers; its back half on s_back follows its front half and the previous batch's back half (the batches
// share the window state), and checks the first timestamp against last_ts once that batch has advanced it.
int enqueue_local_pipelined(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out, int* err_dst,
                            hipEvent_t done) {
    int rc = pipe_setup(h);
    if (rc) return rc;
    const int x = (int)(h->pipe_seq & 1);
    LocalBufs b;
    rc = local_bufs(h, x, b);
    if (rc) return rc;
    LArgs L;
    BatchArgs sgm;
    rc = local_args(h, b, ev, nullptr, n, nullptr, 0, nullptr, 0, out, false, L, sgm);
    if (rc) return rc;
    L.defer_last = 1;
    if (h->pipe_seq >= 2) HIP_TRY(h, hipStreamWaitEvent(h->s_front, h->back_done[x], 0));
    rc = local_front(h, L, sgm, h->s_front);
    if (rc) return rc;
    rc = local_sort(h, L, sgm, b.rec_sorted, h->s_front, true);
    if (rc) return rc;
    HIP_TRY(h, launch_local_exits(L, h->s_front, true));
    HIP_TRY(h, hipEventRecord(h->front_done[x], h->s_front));
    HIP_TRY(h, hipStreamWaitEvent(h->s_back, h->front_done[x], 0));
    HIP_TRY(h, launch_local_back(L, sgm, h->l_has_cx || h->l_has_cx_ps, h->s_aux2, h->s_back, h->pfork, h->pjoin));
    // LogSlot on s_back, behind this batch's walkers and before back_done: the next batch's walkers (s_back) and the
    // batch after that (this workspace's records) both wait for it
    if (h->d_blog) HIP_TRY(h, launch_blog_add(L, blog_args(h), h->s_back));
    HIP_TRY(h, hipMemcpyAsync(err_dst, L.err, sizeof(int), hipMemcpyDeviceToHost, h->s_back));
    HIP_TRY(h, hipEventRecord(h->back_done[x], h->s_back));
    if (done) HIP_TRY(h, hipEventRecord(done, h->s_back));
    h->pipe_seq++;
    ++h->l_batches;
    return SG_OK;
}

}  // namespace

int sg_local_decide_batch(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out, void* stream) {
    return local_decide(h, ev, nullptr, n, nullptr, 0, nullptr, 0, out, stream);
}

int sg_slot_decide_batch(sg_handle* h, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                         const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                         sg_local_result* out, void* stream) {
    return local_decide(h, ev, ext, n, args, n_args, values, n_values, out, stream);
}

int sg_local_enqueue(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out, uint64_t* ticket) {
    if (!h || !ticket) return SG_E_INVAL;
    *ticket = 0;
    if (n == 0) return SG_OK;
    if (!ev || !out) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!local_pipelinable(h)) {  // the synchronous path (after the pipeline drained); its status waits for the ticket
        const int rc = local_decide(h, ev, nullptr, n, nullptr, 0, nullptr, 0, out, nullptr);
        if (rc == SG_E_DEVICE) return rc;
        *ticket = h->next_ticket++;
        h->finished[*ticket] = rc;
        return SG_OK;
    }
    sg_handle::DevTicket& d = h->dev[h->next_ticket % kDevSlots];
    if (!d.done) {
        if (!d.h_err.alloc_bytes(sizeof(int))) return fail(h, SG_E_NOMEM, "pinned error word");
        HIP_TRY(h, hipEventCreateWithFlags(d.done.put(), hipEventDisableTiming));
    }
    if (d.ticket) {  // every slot in flight: complete the oldest (its status waits in `finished`)
        hipError_t e = hipEventSynchronize(d.done);
        h->finished[d.ticket] = e != hipSuccess ? fail(h, SG_E_DEVICE, hipGetErrorString(e)) : ticket_status(h, d);
        d.ticket = 0;
    }
    const int rc = enqueue_local_pipelined(h, ev, n, out, d.h_err, d.done);
    if (rc) return rc;
    d.local = true;
    d.ticket = h->next_ticket++;
    *ticket = d.ticket;
    return SG_OK;
}

int sg_local_block_log_enable(sg_handle* h, int32_t capacity_log2) {
    if (!h) return SG_E_INVAL;
    if (capacity_log2 < 4 || capacity_log2 > 24) return fail(h, SG_E_INVAL, "capacity_log2 outside 4..24");
    if (h->d_blog)
        return capacity_log2 == h->blog_log2 ? SG_OK : fail(h, SG_E_INVAL, "the block log has another capacity");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);  // batches already enqueued stay unlogged: rows record what is decided from here on
    const size_t slots = (size_t)1 << capacity_log2;
    DevBuf<BlogSlot> tab;
    DevBuf<unsigned long long> ctr;
    DevBuf<sg_block_row> rows, keep;
    DevBuf<int32_t> app;
    if (!tab.alloc(slots) || !ctr.alloc(4) || !rows.alloc(slots) || !keep.alloc(slots) || !app.alloc(h->cfg.max_batch))
        return fail(h, SG_E_NOMEM, "block log table");
    HIP_TRY(h, hipMemset(tab, 0, sizeof(BlogSlot) * slots));
    HIP_TRY(h, hipMemset(ctr, 0, sizeof(unsigned long long) * 4));
    HIP_TRY(h, hipMemset(app, 0, sizeof(int32_t) * h->cfg.max_batch));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_blog = std::move(tab);
    h->d_blog_ctr = std::move(ctr);
    h->d_blog_rows = std::move(rows);
    h->d_blog_keep = std::move(keep);
    h->d_blog_app = std::move(app);
    h->blog_log2 = capacity_log2;
    const int rc = blog_sync_apps(h);
    if (rc) {  // off again: a handle is never left with half of the log's state
        h->d_blog.reset();
        h->blog_log2 = 0;
    }
    return rc;
}

int sg_local_block_log(sg_handle* h, int64_t now_ms, sg_block_row* rows, uint64_t cap, uint64_t* n_rows,
                       uint64_t* lost_events, uint64_t* lost_count) {
    if (!h || !n_rows || !lost_events || !lost_count || (!rows && cap)) return SG_E_INVAL;
    *n_rows = *lost_events = *lost_count = 0;
    if (!h->d_blog) return fail(h, SG_E_INVAL, "sg_local_block_log_enable first");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const BlogArgs b = blog_args(h);
    unsigned long long* ctr = h->d_blog_ctr;
    const int64_t limit = now_ms - now_ms % 1000;
    unsigned long long c[4] = {0, 0, 0, 0};
    // the count pass changes nothing: a capacity that is too small leaves the table and the lost totals as they were
    HIP_TRY(h, hipMemsetAsync(ctr + 2, 0, 2 * sizeof(unsigned long long), 0));
    HIP_TRY(h, launch_blog_take(b, limit, 0, nullptr, nullptr, ctr + 2, ctr + 3, 0));
    HIP_TRY(h, hipMemcpy(c, ctr, sizeof(c), hipMemcpyDeviceToHost));
    *n_rows = c[2];
    if (c[2] > cap) return fail(h, SG_E_CAPACITY, "block log rows exceed cap");
    if (c[2]) {  // move the complete rows out, clear the table, put the open seconds' rows back
        HIP_TRY(h, hipMemsetAsync(ctr + 2, 0, 2 * sizeof(unsigned long long), 0));
        HIP_TRY(h, launch_blog_take(b, limit, 1, h->d_blog_rows, h->d_blog_keep, ctr + 2, ctr + 3, 0));
        HIP_TRY(h, hipMemsetAsync(h->d_blog, 0, sizeof(BlogSlot) * h->d_blog.size(), 0));
        HIP_TRY(h, launch_blog_put(b, h->d_blog_keep, ctr + 3, 0));
        HIP_TRY(h, hipMemcpy(rows, h->d_blog_rows, sizeof(sg_block_row) * c[2], hipMemcpyDeviceToHost));
        std::sort(rows, rows + c[2], [](const sg_block_row& x, const sg_block_row& y) {
            return std::tie(x.timestamp, x.resource, x.status, x.app_kind, x.app, x.origin) <
                   std::tie(y.timestamp, y.resource, y.status, y.app_kind, y.app, y.origin);
        });
    }
    HIP_TRY(h, hipMemset(ctr, 0, 2 * sizeof(unsigned long long)));
    HIP_TRY(h, hipDeviceSynchronize());
    *lost_events = c[0];
    *lost_count = c[1];
    return SG_OK;
}

int sg_server_log_enable(sg_handle* h, int32_t capacity_log2) {
    if (!h) return SG_E_INVAL;
    if (!slog_capacity_ok(capacity_log2)) return fail(h, SG_E_INVAL, "capacity_log2 outside 4..24");
    if (h->d_slog)
        return capacity_log2 == h->slog_log2 ? SG_OK : fail(h, SG_E_INVAL, "the server log has another capacity");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);  // batches already enqueued stay unlogged: rows record what is decided from here on
    const size_t slots = (size_t)slog_slots(capacity_log2);
    DevBuf<SlogSlot> tab, rows, keep;
    DevBuf<unsigned long long> ctr;
    if (!tab.alloc(slots) || !ctr.alloc(4) || !rows.alloc(slots) || !keep.alloc(slots))
        return fail(h, SG_E_NOMEM, "server log table");
    HIP_TRY(h, hipMemset(tab, 0, sizeof(SlogSlot) * slots));
    HIP_TRY(h, hipMemset(ctr, 0, sizeof(unsigned long long) * 4));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_slog = std::move(tab);
    h->d_slog_ctr = std::move(ctr);
    h->d_slog_rows = std::move(rows);
    h->d_slog_keep = std::move(keep);
    h->slog_log2 = capacity_log2;
    const int rc = slog_sync_fids(h);
    if (rc) {  // off again, and everything the call allocated freed: a handle is never left with half of the log's state
        h->d_slog.reset();
        h->d_slog_ctr.reset();
        h->d_slog_rows.reset();
        h->d_slog_keep.reset();
        h->d_slog_fid.reset();
        h->d_slog_cpfid.reset();
        h->slog_log2 = 0;
    }
    return rc;
}

int sg_server_log(sg_handle* h, int64_t now_ms, sg_server_row* rows, uint64_t cap, uint64_t* n_rows,
                  uint64_t* lost_events, uint64_t* lost_count) {
    if (!h || !n_rows || !lost_events || !lost_count || (!rows && cap)) return SG_E_INVAL;
    *n_rows = *lost_events = *lost_count = 0;
    if (!h->d_slog) return fail(h, SG_E_INVAL, "sg_server_log_enable first");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    HIP_TRY(h, hipDeviceSynchronize());  // the device-resident entry points' batches too
    const SlogArgs b = slog_args(h);
    unsigned long long* ctr = h->d_slog_ctr;
    const int64_t limit = now_ms - now_ms % 1000;
    unsigned long long c[4] = {0, 0, 0, 0};
    // the count pass changes nothing: a capacity that is too small leaves the table and the lost totals as they were
    HIP_TRY(h, hipMemsetAsync(ctr + 2, 0, 2 * sizeof(unsigned long long), 0));
    HIP_TRY(h, launch_slog_take(b, limit, 0, nullptr, nullptr, ctr + 2, ctr + 3, 0));
    HIP_TRY(h, hipMemcpy(c, ctr, sizeof(c), hipMemcpyDeviceToHost));
    if (slog_cap_answer(c[2], cap, n_rows) != SG_OK) return fail(h, SG_E_CAPACITY, "server log rows exceed cap");
    if (c[2]) {
        // copy the complete slots out and list the others (the table itself is only read), expand on the host, and only
        // when the rows are what the count pass promised clear the table and put the open seconds' slots back
        HIP_TRY(h, hipMemsetAsync(ctr + 2, 0, 2 * sizeof(unsigned long long), 0));
        HIP_TRY(h, launch_slog_take(b, limit, 1, h->d_slog_rows, h->d_slog_keep, ctr + 2, ctr + 3, 0));
        unsigned long long taken = 0;
        HIP_TRY(h, hipMemcpy(&taken, ctr + 2, sizeof(taken), hipMemcpyDeviceToHost));
        std::vector<SlogSlot> slots((size_t)taken);
        if (taken)
            HIP_TRY(h, hipMemcpy(slots.data(), h->d_slog_rows, sizeof(SlogSlot) * taken, hipMemcpyDeviceToHost));
        std::vector<sg_server_row> out;
        out.reserve((size_t)c[2]);
        for (const SlogSlot& s : slots) {
            SlogCounters k{s.ts, s.flow_id, s.value, s.family, {}};
            for (int x = 0; x < kSlogCtrs; ++x) k.c[x] = s.c[x];
            slog_expand(k, out);
        }
        slog_sort_merge(out);  // a handle's keys are distinct: the sort alone
        if (out.size() != c[2])  // nothing was removed yet: the table still holds every row
            return fail(h, SG_E_DEVICE, "server log rows changed between the count and the fetch");
        HIP_TRY(h, hipMemsetAsync(h->d_slog, 0, sizeof(SlogSlot) * h->d_slog.size(), 0));
        HIP_TRY(h, launch_slog_put(b, h->d_slog_keep, ctr + 3, 0));
        std::copy(out.begin(), out.end(), rows);
    }
    HIP_TRY(h, hipMemset(ctr, 0, 2 * sizeof(unsigned long long)));
    HIP_TRY(h, hipDeviceSynchronize());
    *lost_events = c[0];
    *lost_count = c[1];
    return SG_OK;
}

int sg_local_poll(sg_handle* h, uint64_t ticket) { return sg_flow_poll(h, ticket); }

int sg_local_wait(sg_handle* h, uint64_t ticket) { return sg_flow_wait(h, ticket); }

int sg_slot_decide_batch_host(sg_handle* h, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                              const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                              sg_local_result* out) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!ev || !out) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    // the events and the results through host_batch (slots 0, 1); ext and the arguments in slots 2, 3; the values,
    // of any length, in a buffer of this call
    sg_slot_ext* d_ext = nullptr;
    sg_pslot_arg* d_args = nullptr;
    DevBuf<uint64_t> d_vals;
    if (!args) n_args = 0;
    if (!values) n_values = 0;
    if ((ext && !h->stage.get(2, h->cfg.max_batch, d_ext)) || (n_args && !h->stage.get(3, n_args, d_args)) ||
        (n_values && !d_vals.alloc(n_values)))
        return fail(h, SG_E_NOMEM, "host-path buffers");
    if (ext) HIP_TRY(h, hipMemcpy(d_ext, ext, sizeof(sg_slot_ext) * n, hipMemcpyHostToDevice));
    if (n_args) HIP_TRY(h, hipMemcpy(d_args, args, sizeof(sg_pslot_arg) * n_args, hipMemcpyHostToDevice));
    if (n_values) HIP_TRY(h, hipMemcpy(d_vals, values, sizeof(uint64_t) * n_values, hipMemcpyHostToDevice));
    return host_batch(h, h->device, ev, n, out, [&](sg_local_event* d_ev, sg_local_result* d_out) {
        return local_decide(h, d_ev, d_ext, n, d_args, n_args, d_vals, n_values, d_out, nullptr);
    });
}

int sg_local_decide_batch_host(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    return host_batch(h, h->device, ev, n, out, [&](sg_local_event* d_ev, sg_local_result* d_out) {
        return sg_local_decide_batch(h, d_ev, n, d_out, nullptr);
    });
}

namespace {

// One node's windows (resource or origin node) in the sg_local_read_state layout.
int local_read_node(sg_handle* h, uint32_t node, int64_t* second, int64_t* borrow, int64_t* minute, int64_t* head) {
    if ((uint64_t)node >= h->l_nodes) return fail(h, SG_E_INVAL, "node index past the node arrays");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const int S = h->lcfg.sample_count;
    std::vector<LBucket> sb(S), mb(kMinuteS);
    std::vector<LFuture> fb(S);
    LHead hd;
    HIP_TRY(h, hipMemcpy(sb.data(), h->d_lsec + (size_t)node * S, sizeof(LBucket) * S, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(fb.data(), h->d_lbor + (size_t)node * S, sizeof(LFuture) * S, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(mb.data(), h->d_lmin + (size_t)node * kMinuteS, sizeof(LBucket) * kMinuteS, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(&hd, h->d_lhead + node, sizeof(LHead), hipMemcpyDeviceToHost));
    auto dump = [](const LBucket& b, int64_t* o) {
        const bool p = b.start != INT64_MIN;
        o[0] = b.start;
        for (int e = 0; e < kLEv; ++e) o[1 + e] = p ? b.c[e] : 0;
        o[7] = p ? b.min_rt : 0;
    };
    for (int j = 0; j < S; ++j) {
        dump(sb[j], second + 8 * j);
        borrow[2 * j] = fb[j].start;
        borrow[2 * j + 1] = fb[j].start != INT64_MIN ? fb[j].pass : 0;
    }
    for (int j = 0; j < kMinuteS; ++j) dump(mb[j], minute + 8 * j);
    head[0] = hd.threads;
    for (int j = 0; j < 2; ++j) {
        int64_t* o = head + 1 + 6 * j;
        o[0] = hd.cb[j].state;
        o[1] = hd.cb[j].next_retry;
        o[2] = hd.cb[j].stat_start;
        o[3] = hd.cb[j].stat_start != INT64_MIN ? hd.cb[j].bad : 0;
        o[4] = hd.cb[j].stat_start != INT64_MIN ? hd.cb[j].total : 0;
        o[5] = 0;
    }
    head[13] = 0;
    return SG_OK;
}

// A pool node's windows (sg_local_read_state layout): 1 when the node exists, 0 when no event created it yet (the
// dumps of an empty node: null slots, zero counters and threads).
int local_read_pool_node(sg_handle* h, uint64_t key, int64_t* second, int64_t* borrow, int64_t* minute, int64_t* head) {
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    uint32_t node = kNoNode;
    if (h->d_lnkeys) {
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, launch_lnode_find(h->d_lnkeys, h->d_lnvals, h->d_lnkeys.size() - 1, key, h->d_lnode_new, 0));
        HIP_TRY(h, hipMemcpy(&node, h->d_lnode_new, sizeof(node), hipMemcpyDeviceToHost));
    }
    // A node a refused batch created past the pool's capacity (lnode_grow failed, l_pool_used moved past it) has
    // no storage yet: it exists with zero counts, which is what the empty dumps below say.
    const bool stored = node != kNoNode && (uint64_t)node < h->l_nodes;
    if (stored) {
        const int rc = local_read_node(h, node, second, borrow, minute, head);
        return rc ? rc : 1;
    }
    const int S = h->lcfg.sample_count;
    for (int j = 0; j < S; ++j) {
        for (int e = 0; e < 8; ++e) second[8 * j + e] = e == 0 ? INT64_MIN : 0;
        borrow[2 * j] = INT64_MIN;
        borrow[2 * j + 1] = 0;
    }
    for (int j = 0; j < kMinuteS; ++j)
        for (int e = 0; e < 8; ++e) minute[8 * j + e] = e == 0 ? INT64_MIN : 0;
    std::fill(head, head + 14, 0);
    head[3] = head[9] = INT64_MIN;  // the breakers' stat buckets of a fresh node: never created
    return node != kNoNode ? 1 : 0;
}

// FlowRuleUtil.isValidRule (:167-251) for local rules: count >= 0, grade / strategy / behaviour >= 0; QPS rules:
// checkClusterField (an invalid ClusterFlowConfig), checkStrategyField (RELATE / CHAIN need a refResource) and
// checkControlBehaviorField (warm-up period > 0, queueing time > 0); THREAD rules: checkClusterConcurrentField
bool local_flow_rule_valid(const sg_local_flow_rule& r) {
    if (!(r.count >= 0) || r.grade < 0 || r.strategy < 0 || r.control_behavior < 0) return false;
    if (r.cluster_mode == SG_CLUSTER_MODE_INVALID) return false;
    if (r.grade == 0) return true;
    if (r.grade != 1) return false;
    if ((r.strategy == SG_STRATEGY_RELATE || r.strategy == SG_STRATEGY_CHAIN) && r.ref_resource < 0) return false;
    switch (r.control_behavior) {
    case SG_CONTROL_WARM_UP: return r.warm_up_period_sec > 0;
    case SG_CONTROL_RATE_LIMITER: return r.max_queueing_ms > 0;
    case SG_CONTROL_WARM_UP_RATE_LIMITER: return r.warm_up_period_sec > 0 && r.max_queueing_ms > 0;
    default: return true;
    }
}

// FlowRule.equals (FlowRule.java, AbstractRule.equals): Double.compare on count, refResource, clusterMode and the
// ClusterFlowConfig (its caller-given id)
bool local_flow_rule_same(const sg_local_flow_rule& a, const sg_local_flow_rule& b) {
    return a.resource == b.resource && a.grade == b.grade && std::memcmp(&a.count, &b.count, sizeof(double)) == 0 &&
           a.control_behavior == b.control_behavior && a.limit_app == b.limit_app && a.strategy == b.strategy &&
           a.warm_up_period_sec == b.warm_up_period_sec && a.max_queueing_ms == b.max_queueing_ms &&
           (a.ref_resource < 0 ? b.ref_resource < 0 : a.ref_resource == b.ref_resource) &&
           (a.cluster_mode != 0) == (b.cluster_mode != 0) &&
           (a.cluster_mode == 0 || (a.cluster_mode == b.cluster_mode && a.cluster_config == b.cluster_config));
}

// The controller constants of one flow rule (FlowRuleUtil.generateRater; WarmUpController.construct :83-106 in
// Java int arithmetic).
LFlowRule make_flow_rule(const sg_local_flow_rule& r, int cold) {
    LFlowRule f{};
    f.count = r.count;
    f.grade = r.grade;
    f.behavior = (r.grade == 1 && r.control_behavior >= SG_CONTROL_WARM_UP &&
                  r.control_behavior <= SG_CONTROL_WARM_UP_RATE_LIMITER) ? r.control_behavior : SG_CONTROL_DEFAULT;
    f.limit_app = r.limit_app;
    f.max_queue_ms = r.max_queueing_ms;
    f.cold = cold;
    f.strategy = r.strategy;
    f.ref = r.ref_resource < 0 ? -1 : r.ref_resource;
    f.cluster_mode = r.cluster_mode;
    f.cluster_key = r.cluster_key;
    if (f.behavior == SG_CONTROL_WARM_UP || f.behavior == SG_CONTROL_WARM_UP_RATE_LIMITER) {
        f.warning_token = java_d2i(r.warm_up_period_sec * r.count) / (cold - 1);
        const int32_t two_w = (int32_t)(2u * (uint32_t)r.warm_up_period_sec);  // 2 * warmUpPeriodInSec: int
        f.max_token = (int32_t)((uint32_t)f.warning_token + (uint32_t)java_d2i(two_w * r.count / (1.0 + cold)));
        f.slope = (cold - 1.0) / r.count / (double)(int32_t)((uint32_t)f.max_token - (uint32_t)f.warning_token);
    }
    return f;
}

}  // namespace

int sg_local_read_state(sg_handle* h, uint32_t res, int64_t* second, int64_t* borrow, int64_t* minute, int64_t* head) {
    if (!h || res >= h->ltab.size() || !second || !borrow || !minute || !head) return SG_E_INVAL;
    return local_read_node(h, res, second, borrow, minute, head);
}

int sg_local_read_origin_state(sg_handle* h, uint32_t res, int32_t origin, int64_t* second, int64_t* borrow,
                               int64_t* minute, int64_t* head) {
    if (!h || res >= h->ltab.size() || !second || !borrow || !minute || !head) return SG_E_INVAL;
    if (origin <= 0 || origin > h->l_n_origins) return fail(h, SG_E_INVAL, "origin id outside 1..n_origins");
    return local_read_pool_node(h, lnode_key(res, 0, (uint32_t)origin), second, borrow, minute, head);
}

int sg_local_read_context_state(sg_handle* h, uint32_t res, int32_t context, int64_t* second, int64_t* borrow,
                                int64_t* minute, int64_t* head) {
    if (!h || res >= h->ltab.size() || !second || !borrow || !minute || !head) return SG_E_INVAL;
    if (context < 0 || context >= h->l_n_contexts) return fail(h, SG_E_INVAL, "context id outside 0..n_contexts-1");
    return local_read_pool_node(h, lnode_key(res, kLNodeCtx, (uint32_t)context), second, borrow, minute, head);
}

int sg_local_read_controller(sg_handle* h, uint32_t rule, int64_t* state3) {
    if (!h || !state3 || rule >= h->l_rule_slot.size() || h->l_rule_slot[rule] == -1) return SG_E_INVAL;
    const int64_t slot = h->l_rule_slot[rule];
    if (slot == -2) {  // a DefaultController keeps no state
        state3[0] = 0;
        state3[1] = 0;
        state3[2] = -1;
        return SG_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    LCtl c;
    HIP_TRY(h, hipMemcpy(&c, h->d_lctl + slot, sizeof(LCtl), hipMemcpyDeviceToHost));
    state3[0] = c.stored;
    state3[1] = c.last_filled;
    state3[2] = c.latest;
    return SG_OK;
}

int sg_local_set_cluster_state(sg_handle* h, int32_t state) {
    if (!h) return SG_E_INVAL;
    if (state != SG_CLUSTER_CLIENT && state != SG_CLUSTER_SERVER && state != SG_CLUSTER_NOT_STARTED)
        return fail(h, SG_E_INVAL, "cluster state: CLIENT 0, SERVER 1 or NOT_STARTED -1");
    if (state == SG_CLUSTER_CLIENT && (h->l_cluster_rules || h->ps_cluster))
        return fail(h, SG_E_UNSUPPORTED, "cluster-mode flow / param rules on a token client: the tokens come over the "
                                         "network, not in event order (INTEGRATION.md §8)");
    if (state != h->l_cluster_state) h->l_groups_stale = h->ps_groups_stale = true;  // key groups follow the state
    h->l_cluster_state = state;
    return SG_OK;
}

namespace {

// The embedded token server's sharing among the cluster-mode param rules (ParamFlowChecker.passClusterCheck →
// requestParamToken): rules naming one cluster param rule share its ClusterParamMetric, rules whose cluster param rule
// lies in a limiter-enabled namespace share its GlobalRequestLimiter (by_slot: a resource per limiter slot, shared with
// the flow rules' groups). unite(a, b) joins two resources.
void ps_cluster_unions(sg_handle* h, const std::function<void(uint32_t, uint32_t)>& unite, int* by_slot) {
    std::unordered_map<uint32_t, uint32_t> by_key;
    for (const auto& cr : h->ps_cluster_refs) {
        const uint32_t key = cr.second & SG_KEY_INDEX;
        if (key >= h->cprules.size()) continue;  // NO_RULE_EXISTS / BAD_REQUEST: no shared state
        auto it = by_key.emplace(key, cr.first).first;
        unite(cr.first, it->second);
        const int ns = h->cprules[key].namespace_id;
        const int sl = (ns >= 0 && (size_t)ns < h->ns_slot.size()) ? h->ns_slot[ns] : -1;
        if (sl >= 0) {
            if (by_slot[sl] < 0) by_slot[sl] = (int)cr.first;
            unite(cr.first, (uint32_t)by_slot[sl]);
        }
    }
}

// Key groups of the local chain (union-find, smallest resource first): a RELATE rule reads another resource's
// ClusterNode (FlowRuleChecker.selectReferenceNode :96-112); on an embedded token server the resources whose
// cluster-mode rules share a flowId share its ClusterMetric, and those naming flowIds of one limiter-enabled
// namespace share its GlobalRequestLimiter — each group walks in event order on one lane. Sets LRule.grp / cx and
// uploads the rule image and the record keys.
// The key groups of the local chain (resources whose decisions read each other's state): RELATE references and, on
// an embedded token server, resources sharing a flowId's ClusterMetric or a limited namespace. gkey[k] = the smallest
// resource of k's group.
void local_group_keys(sg_handle* h, std::vector<uint32_t>& gkey) {
    const uint32_t K = (uint32_t)h->ltab.size();
    std::vector<uint32_t> parent(K);
    for (uint32_t k = 0; k < K; ++k) parent[k] = k;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    auto unite = [&](uint32_t a, uint32_t b) {
        if (a >= K || b >= K) return;  // param rules of resources the chain does not have
        const uint32_t x = find(a), y = find(b);
        if (x != y) parent[std::max(x, y)] = std::min(x, y);
    };
    for (const auto& pr : h->l_relate) unite(pr.first, pr.second);
    if (h->l_cluster_state == SG_CLUSTER_SERVER) {
        std::unordered_map<uint32_t, uint32_t> by_key;
        int by_slot[kMaxLim];
        for (int j = 0; j < kMaxLim; ++j) by_slot[j] = -1;
        if (h->ps_loaded && h->ps_cluster) ps_cluster_unions(h, unite, by_slot);
        for (const auto& cr : h->l_cluster_refs) {
            const uint32_t key = cr.second & SG_KEY_INDEX;
            if (key >= h->K) continue;  // NO_RULE_EXISTS / BAD_REQUEST: no shared state
            auto it = by_key.emplace(key, cr.first).first;
            unite(cr.first, it->second);
            const int ns = h->rules[key].namespace_id;
            const int sl = (ns >= 0 && (size_t)ns < h->ns_slot.size()) ? h->ns_slot[ns] : -1;
            if (sl >= 0) {
                if (by_slot[sl] < 0) by_slot[sl] = (int)cr.first;
                unite(cr.first, (uint32_t)by_slot[sl]);
            }
        }
    }
    gkey.resize(K);
    for (uint32_t k = 0; k < K; ++k) gkey[k] = find(k);
}

int local_apply_groups(sg_handle* h) {
    const uint32_t K = (uint32_t)h->ltab.size();
    std::vector<uint32_t> gkey, gsize(K, 0);
    local_group_keys(h, gkey);
    for (uint32_t k = 0; k < K; ++k) ++gsize[gkey[k]];
    bool groups = false, has_cx = false;
    for (uint32_t k = 0; k < K; ++k) {
        LRule& L = h->ltab[k];
        L.grp = gsize[gkey[k]] > 1 ? 1 : 0;
        L.cx = (h->l_base_cx.size() == K && h->l_base_cx[k]) || L.grp ? 1 : 0;
        groups = groups || L.grp;
        has_cx = has_cx || L.cx;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_lgkey.reset();
    if (groups) {
        if (!h->d_lgkey.alloc_bytes(sizeof(uint32_t) * K)) return fail(h, SG_E_NOMEM, "key groups");
        HIP_TRY(h, hipMemcpy(h->d_lgkey, gkey.data(), sizeof(uint32_t) * K, hipMemcpyHostToDevice));
    }
    if (K) HIP_TRY(h, hipMemcpy(h->d_lrules, h->ltab.data(), sizeof(LRule) * K, hipMemcpyHostToDevice));
    h->l_has_cx = has_cx;
    h->l_ps_applied = 0;  // param flags are re-applied to the new rule image by the next batch
    h->l_groups_stale = false;
    return local_sys_image(h);
}

// SystemSlot's rule image (serial path): the normal image (key groups and param flags as the device holds them) with
// every inbound resource, and every key group holding one, in a single key group walked by the lane cx walker in
// event order (system_rules.h). Rebuilt after every change of the normal image, of the entry types and of the
// tracking; nothing without tracking or without an inbound resource.
int local_sys_image(sg_handle* h) {
    h->l_sys_image = false;
    const uint32_t K = (uint32_t)h->ltab.size();
    if (!h->l_sys_track || h->l_inbound.size() != K) return SG_OK;
    bool any = false;
    for (uint32_t k = 0; k < K; ++k) any = any || h->l_inbound[k];
    if (!any) return SG_OK;
    std::vector<uint32_t> gkey, skey;
    std::vector<uint8_t> in_group;
    local_group_keys(h, gkey);
    system_group_keys(gkey, h->l_inbound, skey, in_group);
    std::vector<LRule> tab = h->ltab;
    for (uint32_t k = 0; k < K; ++k) {
        if (h->ps_loaded && k < h->ps_res_rules.size() && h->ps_res_rules[k]) tab[k].ps = tab[k].cx = 1;
        if (in_group[k]) tab[k].grp = tab[k].cx = 1;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    if (!h->d_lrules_sys.alloc(K) || !h->d_lgkey_sys.alloc(K)) return fail(h, SG_E_NOMEM, "system image");
    HIP_TRY(h, hipMemcpy(h->d_lrules_sys, tab.data(), sizeof(LRule) * K, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_lgkey_sys, skey.data(), sizeof(uint32_t) * K, hipMemcpyHostToDevice));
    h->l_sys_image = true;
    return SG_OK;
}

void local_sys_drop(sg_handle* h) {
    h->l_sys_track = false;
    h->l_sys_conf = system_defaults();
    h->l_sys_image = false;
    h->l_sys_path = 0;
    h->l_sys_first = 0xFFFFFFFFu;
    h->d_lsys.reset();
    h->d_lsys_sec.reset();
    h->d_lsys_lastp.reset();
    h->d_lsys_acc.reset();
    h->d_lsys_pb.reset();
    h->d_lrules_sys.reset();
    h->d_lgkey_sys.reset();
}

}  // namespace

int sg_local_load_flow_rules(sg_handle* h, const sg_local_flow_rule* rules, uint32_t n, int32_t n_origins,
                             int32_t n_contexts) {
    if (!h || (!rules && n)) return SG_E_INVAL;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    if (n_origins < 0 || n_contexts < 0) return fail(h, SG_E_INVAL, "n_origins / n_contexts < 0");
    if (n_origins < h->l_n_origins || n_contexts < h->l_n_contexts)
        return fail(h, SG_E_INVAL, "origin / context ids keep their meaning across loads: the counts cannot shrink");
    drain_async(h);  // batches on the pipeline decide under the rules they were enqueued with (and settle l_batches)
    if (n_contexts > 0 && h->l_n_contexts == 0 && h->l_batches > 0)
        return fail(h, SG_E_UNSUPPORTED, "context tracking (n_contexts >= 1) starts before the first batch: a DefaultNode "
                                         "holds every entry of its context since the resource's first one");
    const bool track_ctx = n_contexts > 0;
    const uint32_t K = (uint32_t)h->ltab.size();
    const int cold = h->lcfg.cold_factor > 1 ? h->lcfg.cold_factor : 3;
    // FlowRuleUtil.buildFlowRuleMap (:83-130): drop invalid rules and duplicates (its HashSet), group by resource
    std::vector<int64_t> slot(n, -1);
    std::vector<std::vector<uint32_t>> by_res(K);
    bool cluster_rules = false;
    for (uint32_t i = 0; i < n; ++i) {
        const sg_local_flow_rule& r = rules[i];
        if (r.resource >= K || !local_flow_rule_valid(r)) continue;
        if (r.limit_app > n_origins || r.limit_app < SG_LIMIT_APP_OTHER)
            return fail(h, SG_E_INVAL, "limit_app names an origin id outside 1..n_origins");
        if (r.strategy == SG_STRATEGY_CHAIN && r.ref_resource >= n_contexts)
            return fail(h, SG_E_INVAL, "a CHAIN rule names a context id outside 0..n_contexts-1");
        if (r.cluster_mode != SG_CLUSTER_MODE_OFF && r.cluster_mode != SG_CLUSTER_MODE_FALLBACK &&
            r.cluster_mode != SG_CLUSTER_MODE_NO_FALLBACK)
            return fail(h, SG_E_INVAL, "cluster_mode");
        if (r.cluster_mode != SG_CLUSTER_MODE_OFF && h->l_cluster_state == SG_CLUSTER_CLIENT)
            return fail(h, SG_E_UNSUPPORTED, "cluster-mode flow rules on a token client (INTEGRATION.md §8)");
        bool dup = false;
        for (uint32_t j : by_res[r.resource]) dup = dup || local_flow_rule_same(rules[j], r);
        if (!dup) by_res[r.resource].push_back(i);
        cluster_rules = cluster_rules || r.cluster_mode != SG_CLUSTER_MODE_OFF;
    }
    std::vector<std::pair<uint32_t, uint32_t>> relate, cluster_refs;
    std::vector<uint8_t> base_cx(K, 0);
    std::vector<LRule> tab = h->ltab;
    std::vector<LFlowRule> fr;
    for (uint32_t k = 0; k < K; ++k) {
        std::vector<uint32_t>& v = by_res[k];
        // Collections.sort(FlowRuleComparator) (:30-55): stable; cluster-mode rules last, then limitApp "default" last
        auto key = [&](uint32_t x) {
            return (rules[x].cluster_mode != SG_CLUSTER_MODE_OFF ? 2 : 0) + (rules[x].limit_app == SG_LIMIT_APP_DEFAULT ? 1 : 0);
        };
        std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
        for (uint32_t i : v) {
            const sg_local_flow_rule& r = rules[i];
            if (r.strategy == SG_STRATEGY_RELATE && r.ref_resource >= 0 && (uint32_t)r.ref_resource < K &&
                (uint32_t)r.ref_resource != k)
                relate.emplace_back(k, (uint32_t)r.ref_resource);
            if (r.cluster_mode != SG_CLUSTER_MODE_OFF) cluster_refs.emplace_back(k, r.cluster_key);
        }
        LRule& L = tab[k];
        L.fr_begin = L.fr_n = 0;
        L.cx = 0;
        L.ps = 0;
        L.grp = 0;
        L.flow_grade = -1;
        L.flow_count = 0;
        // (with context tracking every event also updates its context's DefaultNode: the cx walker; a fast resource
        // that lands in a key group is walked there too, its one rule read from flow_grade / flow_count)
        const bool fast = v.size() == 1 && !track_ctx && rules[v[0]].limit_app == SG_LIMIT_APP_DEFAULT &&
                          rules[v[0]].strategy == SG_STRATEGY_DIRECT && rules[v[0]].cluster_mode == SG_CLUSTER_MODE_OFF &&
                          make_flow_rule(rules[v[0]], cold).behavior == SG_CONTROL_DEFAULT;
        if (fast) {  // the fast walkers' one DefaultController rule on the ClusterNode
            L.flow_grade = rules[v[0]].grade;
            L.flow_count = rules[v[0]].count;
            slot[v[0]] = -2;
            continue;
        }
        if (v.empty() && !track_ctx) continue;
        base_cx[k] = 1;
        L.fr_begin = (uint32_t)fr.size();
        L.fr_n = (uint32_t)v.size();
        for (uint32_t i : v) {
            slot[i] = (int64_t)fr.size();
            fr.push_back(make_flow_rule(rules[i], cold));
        }
    }
    // the nodes (ClusterNodes and the pool) are untouched: statistics outlive the reload
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    DevBuf<LFlowRule> d_fr;
    DevBuf<LCtl> d_ctl;
    if (!fr.empty() && (!d_fr.alloc(fr.size()) || !d_ctl.alloc(fr.size())))
        return fail(h, SG_E_NOMEM, "local flow rule allocation");
    hipError_t e = hipSuccess;
    if (!fr.empty()) {
        e = hipMemcpy(d_fr, fr.data(), sizeof(LFlowRule) * fr.size(), hipMemcpyHostToDevice);
        std::vector<LCtl> c(fr.size(), LCtl{0, 0, -1, 0});  // storedTokens 0, lastFilledTime 0, latestPassedTime -1
        if (e == hipSuccess) e = hipMemcpy(d_ctl, c.data(), sizeof(LCtl) * c.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, std::string("local flow rule upload: ") + hipGetErrorString(e));
    h->d_lfrules = std::move(d_fr);
    h->d_lctl = std::move(d_ctl);
    h->ltab = tab;
    h->l_base_cx = base_cx;
    h->l_relate = relate;
    h->l_cluster_refs = cluster_refs;
    h->l_n_origins = n_origins;
    h->l_n_contexts = n_contexts;
    h->l_cluster_rules = cluster_rules;
    h->l_rule_slot = slot;
    blocklog_limit_apps(rules, by_res, h->l_res_app);  // LogSlot: which resources need the failing rule reported
    {
        const int rc = blog_sync_apps(h);
        if (rc) return rc;
    }
    const int rc = local_apply_groups(h);
    if (rc) return rc;
    int kept = 0;
    for (int64_t x : slot) kept += x != -1;
    return kept;
}

// AuthorityRuleManager.loadRules: the rule compiler is authority_rules.h (host only); the device table is swapped in
// only after a successful upload, and nothing else of the handle is touched (statistics, nodes, controllers and param
// tables stay).
int sg_local_load_authority_rules(sg_handle* h, const sg_authority_rule* rules, uint32_t n, const int32_t* origins,
                                  uint32_t n_origin_ids, int32_t n_origins) {
    if (!h || (!rules && n) || (!origins && n_origin_ids)) return SG_E_INVAL;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    if (n_origins < 0) return fail(h, SG_E_INVAL, "n_origins < 0");
    drain_async(h);  // batches on the pipeline decide under the rules they were enqueued with
    const uint32_t K = (uint32_t)h->ltab.size();
    std::vector<LAuth> tab;
    std::vector<int32_t> ids;
    const int kept = authority_compile(rules, n, origins, n_origin_ids, K, tab, ids);
    if (kept < 0)
        return fail(h, kept, "an authority rule's resource index, an origin id <= 0 or an origin range outside origins[]");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    DevBuf<LAuth> d_tab;
    DevBuf<int32_t> d_ids;
    if (kept > 0) {
        if (!d_tab.alloc(K) || (!ids.empty() && !d_ids.alloc(ids.size())))
            return fail(h, SG_E_NOMEM, "authority rule allocation");
        hipError_t e = hipMemcpy(d_tab, tab.data(), sizeof(LAuth) * K, hipMemcpyHostToDevice);
        if (e == hipSuccess && !ids.empty())
            e = hipMemcpy(d_ids, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(h, SG_E_DEVICE, std::string("authority rule upload: ") + hipGetErrorString(e));
    }
    h->d_lauth = std::move(d_tab);
    h->d_lauth_ids = std::move(d_ids);
    if (n_origins > h->l_n_origins) h->l_n_origins = n_origins;  // never shrinks (the ids keep their meaning)
    return kept;
}

// ---- SystemSlot ----

namespace {
// The thresholds and status values on the device (LSys up to `threads`; the ENTRY_NODE behind them stays).
int local_sys_upload(sg_handle* h) {
    LSys head{};
    head.conf = h->l_sys_conf;
    head.load = h->l_sys_load;
    head.cpu = h->l_sys_cpu;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->d_lsys, &head, offsetof(LSys, threads), hipMemcpyHostToDevice));
    return SG_OK;
}
}  // namespace

int sg_local_load_system_rules(sg_handle* h, const sg_system_rule* rules, uint32_t n) {
    if (!h || (!rules && n)) return SG_E_INVAL;
    if (!h->d_llast_ts) return fail(h, SG_E_INVAL, "sg_local_load_rules first");
    drain_async(h);  // (and settles l_batches)
    if (!h->l_sys_track) {
        if (h->l_batches > 0)
            return fail(h, SG_E_UNSUPPORTED, "ENTRY_NODE tracking (the first sg_local_load_system_rules) starts before "
                                             "the first batch: the node holds every inbound entry since then");
        const int S = h->lcfg.sample_count;
        HIP_TRY(h, hipSetDevice(h->device));
        if (!h->d_lsys.alloc(1) || !h->d_lsys_sec.alloc(S) || !h->d_lsys_lastp.alloc(S) ||
            !h->d_lsys_acc.alloc((size_t)S * 8) || !h->d_lsys_pb.alloc(3 * (size_t)kMaxPeriods) ||
            (!h->h_lsys_verdict && !h->h_lsys_verdict.alloc(2))) {
            local_sys_drop(h);
            return fail(h, SG_E_NOMEM, "ENTRY_NODE");
        }
        std::vector<LBucket> sec(S);
        for (LBucket& b : sec) {
            b.start = INT64_MIN;
            for (int e = 0; e < kLEv; ++e) b.c[e] = 0;
            b.min_rt = kStatMaxRt;
        }
        std::vector<int64_t> acc((size_t)S * 8, 0);
        for (int j = 0; j < S; ++j) acc[(size_t)8 * j + 7] = INT64_MAX;
        LSys sys{};
        sys.sec = h->d_lsys_sec;
        sys.lastp = h->d_lsys_lastp;
        sys.acc = h->d_lsys_acc;
        sys.first_unproven = 0xFFFFFFFFu;
        HIP_TRY(h, hipMemcpy(h->d_lsys_sec, sec.data(), sizeof(LBucket) * S, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_lsys_acc, acc.data(), sizeof(int64_t) * acc.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemset(h->d_lsys_lastp, 0, sizeof(unsigned long long) * S));
        HIP_TRY(h, hipMemcpy(h->d_lsys, &sys, sizeof(LSys), hipMemcpyHostToDevice));
        h->l_sys_track = true;
    }
    h->l_sys_conf = system_merge(rules, n);
    int rc = local_sys_upload(h);
    if (rc) return rc;
    rc = local_sys_image(h);
    if (rc) return rc;
    return h->l_sys_conf.check;
}

int sg_local_set_system_status(sg_handle* h, double load, double cpu_usage) {
    if (!h) return SG_E_INVAL;
    drain_async(h);
    h->l_sys_load = load;
    h->l_sys_cpu = cpu_usage;
    return h->l_sys_track ? local_sys_upload(h) : SG_OK;
}

int sg_local_read_entry_node(sg_handle* h, int64_t* second, int64_t* cur_thread_num) {
    if (!h || !second || !cur_thread_num) return SG_E_INVAL;
    if (!h->l_sys_track) return fail(h, SG_E_INVAL, "ENTRY_NODE is not tracked: sg_local_load_system_rules first");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    const int S = h->lcfg.sample_count;
    std::vector<LBucket> sb(S);
    LSys sys;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(sb.data(), h->d_lsys_sec, sizeof(LBucket) * S, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(&sys, h->d_lsys, sizeof(LSys), hipMemcpyDeviceToHost));
    for (int j = 0; j < S; ++j) {
        const bool p = sb[j].start != INT64_MIN;
        int64_t* o = second + 8 * j;
        o[0] = sb[j].start;
        for (int e = 0; e < kLEv; ++e) o[1 + e] = p ? sb[j].c[e] : 0;
        o[7] = p ? sb[j].min_rt : 0;
    }
    *cur_thread_num = sys.threads;
    return SG_OK;
}

int sg_local_system_last_path(const sg_handle* h, uint32_t* path) {
    if (!h || !path) return SG_E_INVAL;
    *path = h->l_sys_path;
    return SG_OK;
}

int sg_local_system_first_unproven(const sg_handle* h, uint32_t* index) {
    if (!h || !index) return SG_E_INVAL;
    *index = h->l_sys_first;
    return SG_OK;
}

// ------------------------------------------------------------------------ concurrent cluster tokens

namespace {

// Upload what the concurrency kernels read (thresholds, timeouts, flowIds, counters) after rules / namespaces /
// timeouts changed; first use allocates the token table and the per-batch buffers.
int conc_prepare(sg_handle* h) {
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->d_ctok) {
        h->ctok_slots = 1ull << 20;
        if (!h->d_ctok.alloc_bytes(sizeof(CTok) * h->ctok_slots) ||
            !h->d_calive.alloc_bytes(h->cfg.max_batch) || !h->d_clast_ts.alloc_bytes(sizeof(int64_t)))
            return fail(h, SG_E_NOMEM, "concurrent token table");
        HIP_TRY(h, hipMemset(h->d_ctok, 0, sizeof(CTok) * h->ctok_slots));
        const int64_t neg = -1;
        HIP_TRY(h, hipMemcpy(h->d_clast_ts, &neg, sizeof(neg), hipMemcpyHostToDevice));
        h->ctok_used = 0;
    }
    if (!h->conc_dirty) return SG_OK;
    const uint32_t K = h->K;
    if (h->c_off.size() != K) {
        h->c_off.assign(K, 2000);
        h->c_res.assign(K, 2000);
    }
    std::vector<double> thr(K);
    std::vector<int64_t> fid(K);
    for (uint32_t k = 0; k < K; ++k) {  // ConcurrentClusterFlowChecker.calcGlobalThreshold (:36-46)
        const sg_flow_rule& r = h->rules[k];
        const int connected = (r.namespace_id >= 0 && (size_t)r.namespace_id < h->ns.size())
                                  ? h->ns[r.namespace_id].connected_count : 0;
        thr[k] = r.threshold_type == SG_THRESHOLD_GLOBAL ? r.count : r.count * connected;
        fid[k] = r.flow_id;
    }
    std::vector<int32_t> now = h->cnow_pending ? h->cnow_host : std::vector<int32_t>(K, 0);
    if (!h->cnow_pending && h->d_cnow && now.size() == K) {  // unchanged rules: keep the device counters
        HIP_TRY(h, hipMemcpy(now.data(), h->d_cnow, sizeof(int32_t) * K, hipMemcpyDeviceToHost));
    }
    h->d_cnow.reset();
    h->d_cthr.reset();
    h->d_coff.reset();
    h->d_cres.reset();
    h->d_cfid.reset();
    const size_t k1 = K ? K : 1;
    if (!h->d_cnow.alloc_bytes(sizeof(int32_t) * k1) || !h->d_cthr.alloc_bytes(sizeof(double) * k1) ||
        !h->d_coff.alloc_bytes(sizeof(int64_t) * k1) || !h->d_cres.alloc_bytes(sizeof(int64_t) * k1) ||
        !h->d_cfid.alloc_bytes(sizeof(int64_t) * k1))
        return fail(h, SG_E_NOMEM, "concurrency rule state");
    if (K) {
        HIP_TRY(h, hipMemcpy(h->d_cnow, now.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_cthr, thr.data(), sizeof(double) * K, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_coff, h->c_off.data(), sizeof(int64_t) * K, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_cres, h->c_res.data(), sizeof(int64_t) * K, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_cfid, fid.data(), sizeof(int64_t) * K, hipMemcpyHostToDevice));
    }
    if (!h->d_fid) {
        int rc = upload_fid_table(h);
        if (rc) return rc;
    }
    h->cnow_pending = false;
    h->conc_dirty = false;
    return SG_OK;
}

ConcArgs conc_args(sg_handle* h) {
    ConcArgs c{};
    c.base = h->conc_seq;
    c.K = h->K;
    c.thr = h->d_cthr;
    c.now = h->d_cnow;
    c.client_off = h->d_coff;
    c.res_to = h->d_cres;
    c.flow_id = h->d_cfid;
    c.tab = h->d_ctok;
    c.tmask = h->ctok_slots - 1;
    c.fid = h->d_fid;
    c.fid_mask = h->fid_mask;
    c.alive = h->d_calive;
    c.err = h->ws[0].err;
    c.last_ts = h->d_clast_ts;
    return c;
}

// Keeps the token table at most half full: a rehash into a larger table when the batch could overflow it.
int conc_reserve(sg_handle* h, uint64_t n) {
    if (h->ctok_used + n <= h->ctok_slots / 2) return SG_OK;
    ConcArgs c = conc_args(h);
    DevBuf<unsigned long long> d_live;
    if (!d_live.alloc(1)) return fail(h, SG_E_DEVICE, "live counter: out of memory");
    HIP_TRY(h, hipMemset(d_live, 0, sizeof(unsigned long long)));
    HIP_TRY(h, launch_conc_count(c, d_live, 0));
    unsigned long long live = 0;
    HIP_TRY(h, hipMemcpy(&live, d_live, sizeof(live), hipMemcpyDeviceToHost));
    uint64_t slots = 1ull << 20;
    while (slots < 4 * (live + n)) slots <<= 1;
    DevBuf<CTok> t;
    if (!t.alloc(slots)) return fail(h, SG_E_NOMEM, "concurrent token table");
    HIP_TRY(h, hipMemset(t, 0, sizeof(CTok) * slots));
    HIP_TRY(h, hipMemset(h->ws[0].err, 0, sizeof(int)));
    HIP_TRY(h, launch_conc_rehash(h->d_ctok, h->ctok_slots, t, slots - 1, h->ws[0].err, 0));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_ctok = std::move(t);
    h->ctok_slots = slots;
    h->ctok_used = live;
    return SG_OK;
}

}  // namespace

int sg_conc_set_rule_timeouts(sg_handle* h, const int64_t* client_offline_ms, const int64_t* resource_timeout_ms,
                              uint32_t n) {
    if (!h || (n && (!client_offline_ms || !resource_timeout_ms))) return SG_E_INVAL;
    if (n != h->K) return fail(h, SG_E_INVAL, "one timeout pair per loaded rule");
    drain_async(h);
    h->c_off.assign(client_offline_ms, client_offline_ms + n);
    h->c_res.assign(resource_timeout_ms, resource_timeout_ms + n);
    h->conc_dirty = true;
    return SG_OK;
}

int sg_conc_decide_batch(sg_handle* h, const sg_conc_req* req, uint64_t n, sg_conc_result* out, void* stream_) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out) return fail(h, SG_E_INVAL, "null buffer");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    int rc = conc_prepare(h);
    if (rc) return rc;
    rc = conc_reserve(h, n);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    int kbits = bits_for((uint64_t)h->K);
    if (kbits < 1) kbits = 1;
    if (kbits + bits_for(h->cfg.max_batch) > 64) return fail(h, SG_E_UNSUPPORTED, "rules x max_batch too large");
    ConcArgs c = conc_args(h);
    c.req = req;
    c.out = out;
    c.n = n;
    c.rec = h->ws[0].rec;
    c.kshift = 64 - kbits;
    c.imask = (1ull << c.kshift) - 1;
    if (h->d_slog) {  // the stat log: the walker stores each released token's count beside its result
        if (!h->d_slog_rel && !h->d_slog_rel.alloc(h->cfg.max_batch)) return fail(h, SG_E_NOMEM, "server log release counts");
        c.slog_rel = h->d_slog_rel;
    }
    HIP_TRY(h, hipMemsetAsync(h->ws[0].err, 0, sizeof(int), stream));
    HIP_TRY(h, launch_conc_batch(c, h->ws[0].rec_sorted, h->ws[0].hist, stream));
    if (h->d_slog) HIP_TRY(h, launch_slog_add_conc(c, slog_args(h), stream));  // behind the batch's last writer of out
    HIP_TRY(h, hipMemcpyAsync(h->h_err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (*h->h_err & kErrTime)
        return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    if (*h->h_err & kErrTableFull) return fail(h, SG_E_CAPACITY, "concurrent token table full");
    h->conc_seq += n;
    h->ctok_used += n;
    return SG_OK;
}

int sg_conc_decide_batch_host(sg_handle* h, const sg_conc_req* req, uint64_t n, sg_conc_result* out) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    return host_batch(h, h->device, req, n, out, [&](sg_conc_req* d_req, sg_conc_result* d_out) {
        return sg_conc_decide_batch(h, d_req, n, d_out, nullptr);
    });
}

int sg_conc_expire(sg_handle* h, int64_t now_ms, const uint8_t* client_online, uint32_t n_clients, uint64_t* removed) {
    if (!h || (n_clients && !client_online)) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    int rc = conc_prepare(h);
    if (rc) return rc;
    DevBuf<uint8_t> d_on;
    DevBuf<unsigned long long> d_rm;
    if (!d_on.alloc(n_clients ? n_clients : 1) || !d_rm.alloc(1)) return fail(h, SG_E_DEVICE, "expire buffers: out of memory");
    hipError_t e = n_clients ? hipMemcpy(d_on, client_online, n_clients, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipMemset(d_rm, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = launch_conc_expire(conc_args(h), now_ms, d_on, n_clients, d_rm, 0);
    unsigned long long rm = 0;
    if (e == hipSuccess) e = hipMemcpy(&rm, d_rm, sizeof(rm), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    if (removed) *removed = rm;
    return SG_OK;
}

int sg_conc_read_state(sg_handle* h, uint32_t key, int32_t* now_calls, uint64_t* live_tokens) {
    if (!h || key >= h->K) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    int rc = conc_prepare(h);
    if (rc) return rc;
    if (now_calls) HIP_TRY(h, hipMemcpy(now_calls, h->d_cnow + key, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (live_tokens) {
        DevBuf<unsigned long long> d;
        if (!d.alloc(1)) return fail(h, SG_E_DEVICE, "live counter: out of memory");
        hipError_t e = hipMemset(d, 0, sizeof(unsigned long long));
        if (e == hipSuccess) e = launch_conc_count(conc_args(h), d, 0);
        unsigned long long v = 0;
        if (e == hipSuccess) e = hipMemcpy(&v, d, sizeof(v), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
        *live_tokens = v;
    }
    return SG_OK;
}

// ------------------------------------------------------------------------------ ParamFlowSlot chain

namespace {

PSArgs pslot_args(sg_handle* h) {
    PSArgs s{};
    s.cmode = h->d_ps_cmode;
    s.ckey = h->d_ps_ckey;
    s.p.rules = h->d_prules;
    s.p.n_rules = (uint32_t)h->ptab.size();
    s.p.hot = h->d_phot;
    s.p.table = h->d_ptable;
    s.p.total_slots = h->ptotal;
    s.p.err = h->ws[0].err;
    s.n_res = h->ps_nres;
    s.res_begin = h->d_ps_begin;
    s.res_rules = h->d_ps_rules;
    s.grade = h->d_ps_grade;
    s.cur_idx = h->d_ps_idx;
    s.inited = h->d_ps_init;
    s.tc = h->d_ps_tc;
    s.tc_mask = h->ps_tc_slots - 1;
    s.err = h->ws[0].err;
    s.last_ts = h->d_ps_last_ts;
    return s;
}

// The embedded token server of the cluster-mode param rules (ClusterStateManager SERVER with cluster rules loaded):
// this handle's cluster param state (sg_cparam_load_rules), its namespace limiters and the param batches' last
// timestamp. Without cluster param rules every token would be NO_RULE_EXISTS, which falls back as NOT_STARTED does.
int pslot_embed(sg_handle* h, PSArgs& s, hipStream_t stream) {
    s.emb = 0;
    if (!(h->l_cluster_state == SG_CLUSTER_SERVER && h->ps_cluster && h->d_cplast_ts)) return SG_OK;
    if (h->shard_world > 1 && h->n_lim > 0)
        return fail(h, SG_E_UNSUPPORTED, "an embedded token server on a sharded handle with namespace limiters: the "
                                         "limiter exchange covers flow and param batches only");
    const int rc = cp_rule_limiters(h, stream);
    if (rc) return rc;
    s.emb = 1;
    s.cp = cp_args(h, nullptr, 0, nullptr, 0, nullptr);
    s.cp_rule_lim = h->cp_any_lim ? h->d_cp_rule_lim : nullptr;
    s.lim_ring = h->d_lim_ring;
    for (int j = 0; j < kMaxLim; ++j) s.lim_qps[j] = h->lim_qps[j];
    s.cp_last_ts = h->d_cplast_ts;
    return SG_OK;
}

// Key groups of sg_pslot_decide_batch on an embedded token server (ps_cluster_unions): the record key of each resource.
int pslot_apply_groups(sg_handle* h) {
    if (!h->ps_groups_stale) return SG_OK;
    const uint32_t R = h->ps_nres;
    std::vector<uint32_t> parent(R);
    for (uint32_t k = 0; k < R; ++k) parent[k] = k;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    auto unite = [&](uint32_t a, uint32_t b) {
        const uint32_t x = find(a), y = find(b);
        if (x != y) parent[std::max(x, y)] = std::min(x, y);
    };
    int by_slot[kMaxLim];
    for (int j = 0; j < kMaxLim; ++j) by_slot[j] = -1;
    if (h->l_cluster_state == SG_CLUSTER_SERVER && h->ps_cluster) ps_cluster_unions(h, unite, by_slot);
    std::vector<uint32_t> gkey(R);
    bool groups = false;
    for (uint32_t k = 0; k < R; ++k) groups = (gkey[k] = find(k)) != k || groups;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    h->d_ps_gkey.reset();
    if (groups) {
        if (!h->d_ps_gkey.alloc_bytes(sizeof(uint32_t) * R)) return fail(h, SG_E_NOMEM, "key groups");
        HIP_TRY(h, hipMemcpy(h->d_ps_gkey, gkey.data(), sizeof(uint32_t) * R, hipMemcpyHostToDevice));
    }
    h->ps_groups_stale = false;
    return SG_OK;
}

}  // namespace

int sg_pslot_load_rules(sg_handle* h, const sg_pslot_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                        uint32_t n_hot, uint32_t n_resources) {
    if (!h || (!rules && n)) return SG_E_INVAL;
    drain_async(h);
    std::vector<sg_param_rule> pr(n);
    std::vector<std::vector<uint32_t>> per(n_resources);
    std::vector<int32_t> grade(n), idx(n), zero(n, 0), cmode(n);
    std::vector<uint32_t> ckey(n);
    std::vector<std::pair<uint32_t, uint32_t>> cluster_refs;
    for (uint32_t i = 0; i < n; ++i) {
        if (rules[i].resource >= n_resources) return fail(h, SG_E_INVAL, "rule resource >= n_resources");
        if (rules[i].grade != 0 && rules[i].grade != 1) return fail(h, SG_E_INVAL, "grade must be THREAD or QPS");
        const int32_t cm = rules[i].cluster_mode;
        if (cm != SG_CLUSTER_MODE_OFF && cm != SG_CLUSTER_MODE_FALLBACK && cm != SG_CLUSTER_MODE_NO_FALLBACK &&
            cm != SG_CLUSTER_MODE_INVALID)
            return fail(h, SG_E_INVAL, "cluster_mode must be SG_CLUSTER_MODE_*");
        pr[i] = rules[i].rule;
        // ParamFlowRuleManager keeps the valid rules only (ParamFlowRuleUtil.isValidRule → checkCluster :54-66), per
        // resource in load order (getRulesOfResource)
        if (cm != SG_CLUSTER_MODE_INVALID) per[rules[i].resource].push_back(i);
        grade[i] = rules[i].grade;
        idx[i] = rules[i].param_idx;
        cmode[i] = cm;
        ckey[i] = rules[i].cluster_key;
        if ((cm == SG_CLUSTER_MODE_FALLBACK || cm == SG_CLUSTER_MODE_NO_FALLBACK) && rules[i].grade == 1)
            cluster_refs.emplace_back(rules[i].resource, rules[i].cluster_key);  // passCheck → passClusterCheck
    }
    if (!cluster_refs.empty() && h->l_cluster_state == SG_CLUSTER_CLIENT)
        return fail(h, SG_E_UNSUPPORTED, "cluster-mode param rules on a token client: the tokens come over the network, "
                                         "not in event order (INTEGRATION.md §8)");
    int rc = sg_param_load_rules(h, pr.data(), n, hot, n_hot);
    if (rc) return rc;
    std::vector<uint32_t> begin(n_resources + 1, 0), list;
    for (uint32_t r = 0; r < n_resources; ++r) {
        begin[r] = (uint32_t)list.size();
        list.insert(list.end(), per[r].begin(), per[r].end());
    }
    begin[n_resources] = (uint32_t)list.size();
    HIP_TRY(h, hipSetDevice(h->device));
    h->d_ps_begin.reset();
    h->d_ps_rules.reset();
    h->d_ps_grade.reset();
    h->d_ps_idx.reset();
    h->d_ps_init.reset();
    h->d_ps_cmode.reset();
    h->d_ps_ckey.reset();
    const size_t n1 = n ? n : 1;
    if (!h->d_ps_begin.alloc_bytes(sizeof(uint32_t) * (n_resources + 1)) ||
        !h->d_ps_rules.alloc_bytes(sizeof(uint32_t) * n1) ||
        !h->d_ps_grade.alloc_bytes(sizeof(int32_t) * n1) ||
        !h->d_ps_idx.alloc_bytes(sizeof(int32_t) * n1) || !h->d_ps_init.alloc_bytes(sizeof(int32_t) * n1) ||
        !h->d_ps_cmode.alloc_bytes(sizeof(int32_t) * n1) || !h->d_ps_ckey.alloc_bytes(sizeof(uint32_t) * n1))
        return fail(h, SG_E_NOMEM, "param slot rules");
    HIP_TRY(h, hipMemcpy(h->d_ps_begin, begin.data(), sizeof(uint32_t) * (n_resources + 1), hipMemcpyHostToDevice));
    if (!list.empty()) HIP_TRY(h, hipMemcpy(h->d_ps_rules, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice));
    if (n) {
        HIP_TRY(h, hipMemcpy(h->d_ps_cmode, cmode.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_ps_ckey, ckey.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_ps_grade, grade.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_ps_idx, idx.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_ps_init, zero.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    }
    if (!h->d_ps_tc) {
        h->ps_tc_slots = 1ull << 20;
        if (!h->d_ps_tc.alloc_bytes(sizeof(PSThread) * h->ps_tc_slots) ||
            !h->d_ps_last_ts.alloc_bytes(sizeof(int64_t)))
            return fail(h, SG_E_NOMEM, "thread count table");
    }
    HIP_TRY(h, launch_pslot_clear(h->d_ps_tc, h->ps_tc_slots, 0));
    const int64_t neg = -1;
    HIP_TRY(h, hipMemcpy(h->d_ps_last_ts, &neg, sizeof(neg), hipMemcpyHostToDevice));
    HIP_TRY(h, hipDeviceSynchronize());
    h->ps_nres = n_resources;
    h->ps_loaded = true;
    h->ps_cluster = !cluster_refs.empty();
    h->ps_cluster_refs = cluster_refs;
    h->ps_groups_stale = true;
    h->l_groups_stale = true;  // the slot chain's key groups include the cluster-mode param rules
    h->ps_res_rules.assign(n_resources, 0);
    for (uint32_t r = 0; r < n_resources; ++r) h->ps_res_rules[r] = (uint32_t)per[r].size();
    ++h->ps_gen;
    return SG_OK;
}

int sg_pslot_decide_batch(sg_handle* h, const sg_pslot_event* ev, uint64_t n, const sg_pslot_arg* args, uint64_t n_args,
                          const uint64_t* values, uint64_t n_values, sg_pslot_result* out, void* stream_) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!ev || !out) return fail(h, SG_E_INVAL, "null buffer");
    if (!h->ps_loaded) return fail(h, SG_E_INVAL, "sg_pslot_load_rules first");
    if (n > h->cfg.max_batch) return fail(h, SG_E_CAPACITY, "batch larger than max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    int kbits = bits_for((uint64_t)h->ps_nres);
    if (kbits < 1) kbits = 1;
    if (kbits + bits_for(h->cfg.max_batch) > 64) return fail(h, SG_E_UNSUPPORTED, "resources x max_batch too large");
    hipStream_t stream = (hipStream_t)stream_;
    int rc = pslot_apply_groups(h);
    if (rc) return rc;
    PSArgs s = pslot_args(h);
    rc = pslot_embed(h, s, stream);
    if (rc) return rc;
    s.gkey = s.emb ? h->d_ps_gkey : nullptr;
    s.ev = ev;
    s.args = args;
    s.n_args = n_args;
    s.values = values;
    s.n_values = n_values;
    s.out = out;
    s.n = n;
    s.rec = h->ws[0].rec;
    s.kshift = 64 - kbits;
    s.imask = (1ull << s.kshift) - 1;
    HIP_TRY(h, hipMemsetAsync(h->ws[0].err, 0, sizeof(int), stream));
    HIP_TRY(h, launch_pslot_batch(s, h->ws[0].rec_sorted, h->ws[0].hist, stream));
    HIP_TRY(h, hipMemcpyAsync(h->h_err, h->ws[0].err, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    if (*h->h_err & kErrTime)
        return fail(h, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than earlier batches");
    if (*h->h_err & kErrBounds) return fail(h, SG_E_INVAL, "an event's arguments lie outside the arg / value arrays");
    if (*h->h_err & kErrTableFull) return fail(h, SG_E_CAPACITY, "a param or thread-count table is full");
    return SG_OK;
}

int sg_pslot_decide_batch_host(sg_handle* h, const sg_pslot_event* ev, uint64_t n, const sg_pslot_arg* args,
                               uint64_t n_args, const uint64_t* values, uint64_t n_values, sg_pslot_result* out) {
    if (!h) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    // this entry point has no max_batch bound of its own: its buffers are this call's
    DevBuf<sg_pslot_event> d_ev;
    DevBuf<sg_pslot_arg> d_args;
    DevBuf<uint64_t> d_vals;
    DevBuf<sg_pslot_result> d_out;
    hipError_t e = d_ev.alloc(n) && d_args.alloc(n_args ? n_args : 1) && d_vals.alloc(n_values ? n_values : 1) && d_out.alloc(n)
                       ? hipSuccess
                       : hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpy(d_ev, ev, sizeof(sg_pslot_event) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_args) e = hipMemcpy(d_args, args, sizeof(sg_pslot_arg) * n_args, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_values) e = hipMemcpy(d_vals, values, sizeof(uint64_t) * n_values, hipMemcpyHostToDevice);
    int rc = SG_E_DEVICE;
    if (e == hipSuccess) {
        rc = sg_pslot_decide_batch(h, d_ev, n, d_args, n_args, d_vals, n_values, d_out, nullptr);
        if (rc == SG_OK) e = hipMemcpy(out, d_out, sizeof(sg_pslot_result) * n, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    return rc;
}

int sg_pslot_thread_count(sg_handle* h, uint32_t resource, int32_t param_idx, uint64_t value, int64_t* count) {
    if (!h || !count || !h->ps_loaded || resource >= h->ps_nres || param_idx < 0) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    DevBuf<int64_t> d;
    if (!d.alloc(1)) return fail(h, SG_E_DEVICE, "read buffer: out of memory");
    hipError_t e = launch_pslot_thread_read(pslot_args(h), resource, param_idx, value, d, 0);
    if (e == hipSuccess) e = hipMemcpy(count, d, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(e));
    return SG_OK;
}

int sg_pslot_param_idx(sg_handle* h, uint32_t rule, int32_t* param_idx) {
    if (!h || !param_idx || !h->ps_loaded || rule >= h->ptab.size()) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    drain_async(h);
    HIP_TRY(h, hipMemcpy(param_idx, h->d_ps_idx + rule, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SG_OK;
}

int sg_debug_copy(sg_handle* h, int what, void* dst, uint64_t bytes) {
    if (!h || !dst) return SG_E_INVAL;
    const void* src = nullptr;
    uint64_t cap = 0;
    switch (what) {
    case 0: src = (h->last_sorted == h->ws[0].rec) ? h->ws[0].rec_sorted : h->ws[0].rec; cap = h->cfg.max_batch * 8; break;
    case 1: src = h->last_sorted ? h->last_sorted : h->ws[0].rec_sorted; cap = h->cfg.max_batch * 8; break;
    case 2: src = h->ws[0].bnd; cap = sizeof(uint32_t) * kMaxWl * kMaxPeriods; break;
    case 3: src = h->ws[0].p0; cap = sizeof(int64_t) * kMaxWl; break;
    case 4: src = h->ws[0].np; cap = sizeof(uint32_t) * kMaxWl; break;
    case 5: src = h->d_dbg; cap = 128 * 8; break;
    case 6: src = h->d_cp_skip_count; cap = h->d_cp_skip_count ? sizeof(uint32_t) : 0; break;
    default: return SG_E_INVAL;
    }
    if (bytes > cap || !src) return SG_E_INVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    if (what == 1 && h->last_rec4_n > 0 && src == h->ws[0].rec_sorted && h->ws[0].bin_buf) {
        // the compact layout keeps 4-byte sorted records: the 8-byte view is rebuilt from them and the batch's segment
        // lists into the regular bins' buffer (free once the batch is done)
        drain_async(h);
        HIP_TRY(h, hipDeviceSynchronize());
        BatchArgs a = flow_args(h, h->ws[0], nullptr, h->last_rec4_n, nullptr);
        a.rec4 = 1;
        HIP_TRY(h, launch_rec4_expand(a, h->ws[0].bin_buf, nullptr));
        HIP_TRY(h, hipDeviceSynchronize());
        src = h->ws[0].bin_buf;
        if (bytes > h->last_rec4_n * 8) return SG_E_INVAL;
    }
    HIP_TRY(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return SG_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ node handle
//
// One token server over G shard handles (include/sentinel_gpu.h, sg_node_*): the reference's single TokenService
// (DefaultTokenService.java:39-50) serving every flowId, with the flowIds hashed over the shards (SURVEY §8(b)
// "multi-GPU fan-out is internal to the handle", §8(e)). A batch in caller order goes to the front handle (on the
// first shard's device: validation and the namespace limiter over the whole batch in caller order — the node's
// exact arrival order), then is split by owner (node.hip), decided by every shard concurrently on its own stream
// (peer copies for shards on other devices), and gathered back into caller order.

struct sg_node {
    ~sg_node();  // drains the node, destroys the shards and the front; then devices[0]'s members free under devices[0]
    std::string err;
    sg_config cfg{};
    std::vector<int32_t> devices;       // device of each shard
    sg_handle* front = nullptr;         // devices[0]: validation + namespace limiter over the node batch
    std::vector<sg_handle*> shards;
    // What the node keeps for one shard on that shard's device; its destructor makes the device current, so the members
    // are freed there.
    struct Shard {
        explicit Shard(int32_t dev) : device(dev) {}
        Shard(Shard&&) = default;
        ~Shard() { (void)hipSetDevice(device); }
        int32_t device;
        Stream stream;
        Event done;                     // its slice decided (and copied back)
        PinnedBuf<int> h_err;
        DevBuf<sg_req> r_req;           // a shard on another device than devices[0]: its slice there
        DevBuf<sg_result> r_out;
        DevBuf<uint8_t> r_nreq, r_nout; // the same for the param / concurrent slices (see d_sub_nreq)
        DevBuf<uint64_t> r_vals;
        DevBuf<sg_slot_ext> r_ext;      // the slot chain's slice: ext records and compacted args (values in r_vals)
        DevBuf<sg_pslot_arg> r_args;
        DevBuf<double> r_snap;         // its part of the node snapshot
        DevBuf<sg_metric_node> r_mrows; // its metric rows
        DevBuf<uint64_t> r_mcnt;        // its row count (on its device wherever that is)
    };
    std::vector<Shard> sh;              // one per shard
    Stream s0;           // devices[0]
    Event routed;
    std::vector<sg_flow_rule> rules;
    std::vector<uint8_t> shard_of;
    std::vector<uint32_t> local_of;
    DevBuf<uint8_t> d_shard_of;
    DevBuf<uint32_t> d_local_of;
    DevBuf<uint32_t> d_tile_cnt;
    DevBuf<uint32_t> d_base;            // [kMaxShards + 1] bases, then [kMaxShards] totals
    PinnedBuf<uint32_t> h_base;         // pinned copy
    PinnedBuf<int> h_front_err;         // pinned
    DevBuf<sg_req> d_sub_req;
    DevBuf<uint32_t> d_sub_pos;
    DevBuf<sg_result> d_sub_out;
    // every shard on the front's device with the front's request-index / acquire layout: the records path (the
    // shards start at the sort, on the front's period tables, and write the caller's results in place)
    bool rec_path = false;
    DevBuf<uint64_t> d_sub_rec;         // [max_batch] the shards' record slices
    std::vector<sg_namespace> ns;       // the node's namespaces (rollback of a failed sg_node_set_namespaces)
    // pipelined node batches (sg_node_flow_enqueue, records path): two workspaces alternating, as the single
    // handle's pipeline — the front's k_prep / limiter / routing of batch i+1 and the shards' sorts beside the
    // shards' walkers of batch i
    struct PipeSlot {
        uint64_t ticket = 0;
        Event done;   // every shard's back half of the slot's batch (recorded on s0)
        PinnedBuf<int> h_err;        // pinned [kMaxShards]: each shard's error word
        PinnedBuf<uint32_t> h_base;  // pinned [2 * kMaxShards + 1]: slice bases and counts
        uint32_t G_used = 0;         // shards the batch went to
    };
    PipeSlot pipe[2];
    Event fdone[2];  // the front's part of the slot's batch
    DevBuf<uint64_t> d_sub_rec2;               // workspace 1's record slices
    uint64_t pseq = 0, next_ticket = 1;
    std::unordered_map<uint64_t, int> finished;  // tickets completed while making room, not yet collected
    // cluster param and concurrent tokens over the node (sg_node_cparam_*, sg_node_conc_*): a param rule lives on the
    // shard owning its flowId; a concurrent token on the shard owning its flow rule's flowId
    std::vector<sg_cparam_rule> cp_rules;
    std::vector<uint8_t> cp_shard_of;
    std::vector<uint32_t> cp_local_of;
    DevBuf<uint8_t> d_cp_shard_of;
    DevBuf<uint32_t> d_cp_local_of;
    DevBuf<uint64_t> d_nrec;           // [max_batch] owner records, then the sort's other buffer
    DevBuf<uint64_t> d_nrec2;
    DevBuf<uint32_t> d_nhist;
    DevBuf<uint32_t> d_nvals;          // [max_batch]
    DevBuf<uint32_t> d_ncnt;           // [3 * kMaxShards]: requests, values, value bases per shard
    DevBuf<uint32_t> d_ntsum;          // [tiles]
    DevBuf<int> d_nerr;
    DevBuf<uint8_t> d_sub_nreq;        // [max_batch] slices (sg_cparam_req / sg_conc_req: 24 B / 32 B each)
    DevBuf<uint8_t> d_sub_nout;        // [max_batch] slice results (sg_result / sg_conc_result)
    DevBuf<uint64_t> d_sub_vals;       // the param slices' values
    int64_t cp_last_ts = -1, cc_last_ts = -1;  // the node's previous param / concurrent batch (time order)
    Staging stage;                     // the _host entry points' device copies (host_batch), on devices[0]
    // node snapshot on the device: each shard's part gathered into the front's buffer in node rule order
    std::vector<DevBuf<uint32_t>> d_node_key;  // per shard (on the front's device): node rule of each local rule
    DevBuf<double> d_snap;
    bool node_key_stale = true;         // the flow rules changed since d_node_key was built
    // the local slot chain over the node (sg_node_local_*): every shard holds the node's rules under the node's
    // resource indices and decides the events of the resources it owns; the front is the staging copy of the rules
    // (it carries no local traffic) and names the owners
    bool l_loaded = false;
    sg_local_config l_cfg{};
    std::vector<sg_local_rule> l_rules;
    std::vector<sg_local_flow_rule> l_frules;   // the flow rules in force (the front's rollback)
    bool l_has_frules = false;
    std::vector<sg_authority_rule> l_arules;    // the authority rules in force and their origin ids (the same)
    std::vector<int32_t> l_aorigins;
    int32_t l_n_origins = 0, l_n_contexts = 0;
    std::vector<uint32_t> l_owner;      // [K] owner shard of each resource
    DevBuf<uint8_t> d_l_owner;          // the same on devices[0]
    int64_t l_last_ts = -1;             // the node's previous local batch (time order)
    uint64_t l_batches = 0;             // local batches decided since sg_node_local_load_rules
    DevBuf<sg_local_event> d_lsub_ev;      // [max_batch] the shards' slices
    DevBuf<sg_local_result> d_lsub_out;    // [max_batch] their results
    DevBuf<int> d_lerr;
    // the whole slot chain over the node (sg_node_slot_decide_batch, sg_node_pslot_load_rules): the param rules in
    // force (every shard holds all of them under the node's indices; the front's rollback), the slices' ext records,
    // and the compacted argument arrays of the shards that cannot read the caller's (node.hip k_lcmp_*)
    bool l_ps_loaded = false;
    std::vector<sg_pslot_rule> l_prules;
    std::vector<sg_param_hot_item> l_phot;
    bool compact_args = false;             // test aid (env SG_NODE_COMPACT_ARGS=1, read at sg_node_create): every shard
                                           // gets compacted arrays, so one GPU exercises that path
    DevBuf<sg_slot_ext> d_lsub_ext;        // [max_batch]
    std::vector<DevBuf<sg_pslot_arg>> d_cargs;  // per shard, on devices[0] (grown on demand)
    std::vector<DevBuf<uint64_t>> d_cvals;
    DevBuf<unsigned long long> d_ctsum;    // the shards' tile sums, one region per shard
    DevBuf<unsigned long long> d_ctot;     // [kMaxShards][2] arg and value totals
    // the node's metric rows: every shard's raw rows one after the other, merged by k_merge_*
    DevBuf<unsigned long long> d_mbits;     // [60][W]
    DevBuf<uint32_t> d_mpre;                // [60][W]
    uint32_t m_words = 0;                   // W of the allocation
    DevBuf<MergeSlots> d_mslots;
    DevBuf<sg_metric_node> d_mrows;         // the shards' raw rows (grown on demand)
    DevBuf<sg_metric_node> d_mout;          // the host form's merged table
    // the node's logs (sg_node_server_log_enable / sg_node_local_block_log_enable; 0: off). Rows a fetch took from
    // some handles before another failed, and lost totals already consumed from a handle, wait here for the next
    // successful fetch: nothing a handle handed out is dropped.
    int32_t slog_log2 = 0, blog_log2 = 0;
    std::vector<sg_server_row> slog_held;
    std::vector<sg_block_row> blog_held;
    uint64_t slog_lost[2] = {0, 0}, blog_lost[2] = {0, 0};
};

namespace {

int nfail(sg_node* nd, int code, const std::string& msg) {
    if (nd) nd->err = msg;
    return code;
}

#define NHIP(nd, expr)                                                                          \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return nfail((nd), SG_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(_e));   \
    } while (0)

// splitmix64(flowId) mod G: the owner shard (sentinel_amd/cluster.py shard_of)
uint32_t node_owner(int64_t flow_id, uint32_t G) {
    return (uint32_t)(mix64((uint64_t)flow_id) % G);
}

// A shard's error, in the node's words.
int node_child(sg_node* nd, sg_handle* h, int rc) {
    if (rc < 0) nd->err = h->err;
    return rc;
}

// The shards' rules indexed into the front's window-length table (a superset: the front holds every node rule, and the
// limiter's 100 ms), so that a shard walks the node batch's period tables as the front's k_prep built them; and
// whether the records path applies (every shard on the front's device, the same record layout below the key).
int node_sync_layout(sg_node* nd) {
    sg_handle* f = nd->front;
    int rc = ensure_layout(f);
    if (rc) return node_child(nd, f, rc);
    bool same = true;
    for (size_t g = 0; g < nd->shards.size(); ++g) {
        sg_handle* h = nd->shards[g];
        rc = ensure_layout(h);
        if (rc) return node_child(nd, h, rc);
        same = same && nd->devices[g] == nd->devices[0] && h->ibits == f->ibits && h->abits == f->abits;
        if (!h->K) continue;
        for (uint32_t k = 0; k < h->K; ++k) {
            Rule& R = h->rule_tab[k];
            int w = 0;
            while (w < f->n_wl && f->wl[w] != R.wl) ++w;
            if (w == f->n_wl) return nfail(nd, SG_E_DEVICE, "a shard window length missing at the front");
            R.wl_idx = w;
        }
        h->n_wl = f->n_wl;
        std::memcpy(h->wl, f->wl, sizeof(h->wl));
        NHIP(nd, hipSetDevice(h->device));
        NHIP(nd, hipMemcpy(h->d_rules, h->rule_tab.data(), sizeof(Rule) * h->K, hipMemcpyHostToDevice));
    }
    nd->rec_path = same && std::getenv("SG_NODE_LEGACY") == nullptr;
    if (nd->rec_path && !nd->d_sub_rec) {
        NHIP(nd, hipSetDevice(nd->devices[0]));
        if (!nd->d_sub_rec.alloc_bytes(sizeof(uint64_t) * (nd->cfg.max_batch + kRecW)))
            return nfail(nd, SG_E_NOMEM, "shard record slices");
    }
    return SG_OK;
}

// The walker CUs of shard g: its device's share when several shards of the node live on one device (each shard's
// persistent walker grids were sized for the whole CU set, and G of them contended for it: round 5's G = 4 step took
// 5x one handle's). `cus` is the CU set the walkers' streams may use (0: the whole device).
int node_walk_cus(const sg_node* nd, uint32_t g, int cus) {
    int same = 0;
    for (int32_t d : nd->devices) same += d == nd->devices[g] ? 1 : 0;
    if (same <= 1) return cus;
    if (cus <= 0) {
        int all = 0;
        (void)hipDeviceGetAttribute(&all, hipDeviceAttributeMultiprocessorCount, nd->devices[g]);
        cus = all > 0 ? all : 256;
    }
    return std::max(1, cus / same);
}

// Waits for the shard streams [0, g) (an early return must not leave slices in flight).
void node_sync_shards(sg_node* nd, uint32_t g) {
    for (uint32_t x = 0; x < g && x < nd->sh.size(); ++x) {
        (void)hipSetDevice(nd->devices[x]);
        (void)hipStreamSynchronize(nd->sh[x].stream);
    }
    (void)hipSetDevice(nd->devices[0]);
}

// One shard's slice of a node batch on the records path: the sort of its records (node request indices), its
// segments, both walkers and the skipped BLOCK counts, its error word into err_dst. `front` carries the sort and
// segments, `back` the walkers (the same stream for a synchronous node batch); front_done (may be null) joins them.
int node_shard_rec(sg_handle* h, BatchArgs b, uint64_t cnt, uint64_t n_node, uint32_t* hist, hipStream_t front,
                   hipStream_t back, hipStream_t aux, hipEvent_t fork, hipEvent_t join, hipEvent_t front_done,
                   int* err_dst) {
    HIP_TRY(h, hipMemsetAsync(b.err, 0, sizeof(int), front));
    HIP_TRY(h, hipMemsetAsync(b.long_count, 0, (1 + kClasses) * sizeof(uint32_t), front));
    HIP_TRY(h, hipMemsetAsync(b.skip_count, 0, sizeof(uint32_t), front));
    uint64_t* sorted = nullptr;
    HIP_TRY(h, radix_sort_records(b.rec, b.rec_sorted, cnt, b.kshift, hist, &sorted, front, 64, b.hist0 != nullptr,
                                  b.csum0 != nullptr));
    b.rec_sorted = sorted;
    HIP_TRY(h, launch_seg_flow(b, front));
    if (front_done) {
        HIP_TRY(h, hipEventRecord(front_done, front));
        HIP_TRY(h, hipStreamWaitEvent(back, front_done, 0));
    }
    HIP_TRY(h, hipEventRecord(fork, back));
    HIP_TRY(h, hipStreamWaitEvent(aux, fork, 0));
    HIP_TRY(h, launch_walk_long(b, aux));
    HIP_TRY(h, launch_walk_short(b, back));
    HIP_TRY(h, hipEventRecord(join, aux));
    HIP_TRY(h, hipStreamWaitEvent(back, join, 0));
    HIP_TRY(h, launch_skip_apply(b, back));
    if (h->d_slog) {  // the token server's stat log (sg_node_server_log_enable), behind the slice's decisions
        const int src = slog_add_flow(h, b, back, n_node);
        if (src) return src;
    }
    HIP_TRY(h, hipMemcpyAsync(err_dst, b.err, sizeof(int), hipMemcpyDeviceToHost, back));
    return SG_OK;
}

// A completed pipelined node batch's status: the first shard error (the front's was answered at enqueue).
int node_slot_status(sg_node* nd, const sg_node::PipeSlot& sl) {
    for (uint32_t g = 0; g < sl.G_used; ++g)
        if (sl.h_err[g]) return node_child(nd, nd->shards[g], flow_status(nd->shards[g], sl.h_err[g]));
    return SG_OK;
}

// Completes the node's pipelined batches (their statuses wait for sg_node_flow_poll / _wait): every other node call
// starts from a drained node, and the synchronous path uses workspace 0.
int node_drain(sg_node* nd) {
    for (auto& sl : nd->pipe) {
        if (!sl.ticket) continue;
        (void)hipSetDevice(nd->devices[0]);
        const hipError_t e = hipEventSynchronize(sl.done);
        nd->finished[sl.ticket] = e != hipSuccess ? nfail(nd, SG_E_DEVICE, hipGetErrorString(e)) : node_slot_status(nd, sl);
        sl.ticket = 0;
    }
    for (sg_handle* h : nd->shards) drain_async(h);
    if (nd->front) drain_async(nd->front);
    if (!nd->devices.empty()) (void)hipSetDevice(nd->devices[0]);
    return SG_OK;
}

}  // namespace

sg_node::~sg_node() {
    node_drain(this);
    for (size_t g = 0; g < shards.size(); ++g) sg_destroy(shards[g]);
    sh.clear();  // each under its own device
    sg_destroy(front);
    (void)hipSetDevice(devices.empty() ? 0 : devices[0]);
}

extern "C" {

void sg_node_destroy(sg_node* nd) { delete nd; }

const char* sg_node_last_error(const sg_node* nd) { return nd ? nd->err.c_str() : "null node"; }

int sg_node_create(const sg_config* cfg, const int32_t* devices, uint32_t n_shards, sg_node** out) {
    if (!cfg || !devices || !out || n_shards == 0 || n_shards > (uint32_t)kMaxShards) return SG_E_INVAL;
    *out = nullptr;
    sg_node* nd = new sg_node();
    nd->cfg = *cfg;
    nd->devices.assign(devices, devices + n_shards);
    nd->sh.reserve(n_shards);
    if (const char* p = std::getenv("SG_NODE_COMPACT_ARGS")) nd->compact_args = std::atoi(p) != 0;
    nd->d_cargs.resize(n_shards);
    nd->d_cvals.resize(n_shards);
    auto bail = [&](int rc) {
        delete nd;
        return rc;
    };
    sg_config c = *cfg;
    c.device = devices[0];
    int rc = sg_create(&c, &nd->front);
    if (rc) return bail(rc);
    nd->front->front_only = true;
    for (uint32_t g = 0; g < n_shards; ++g) {
        c.device = devices[g];
        sg_handle* h = nullptr;
        rc = sg_create(&c, &h);
        if (rc) return bail(rc);
        nd->shards.push_back(h);
        if (hipSetDevice(devices[g]) != hipSuccess) return bail(SG_E_DEVICE);
        nd->sh.emplace_back(devices[g]);
        sg_node::Shard& s = nd->sh.back();
        if (hipStreamCreateWithFlags(s.stream.put(), hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(s.done.put(), hipEventDisableTiming) != hipSuccess || !s.h_err.alloc(1))
            return bail(SG_E_DEVICE);
        if (devices[g] != devices[0] && (!s.r_req.alloc(cfg->max_batch) || !s.r_out.alloc(cfg->max_batch)))
            return bail(SG_E_NOMEM);
    }
    // shards on other devices: peer access both ways (their slices and results cross xGMI as peer copies)
    for (uint32_t g = 1; g < n_shards; ++g) {
        const int d0 = devices[0], dg = devices[g];
        if (dg == d0) continue;
        int can0 = 0, can1 = 0;
        (void)hipDeviceCanAccessPeer(&can0, d0, dg);
        (void)hipDeviceCanAccessPeer(&can1, dg, d0);
        if (can0) {
            (void)hipSetDevice(d0);
            const hipError_t e = hipDeviceEnablePeerAccess(dg, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return bail(SG_E_DEVICE);
        }
        if (can1) {
            (void)hipSetDevice(dg);
            const hipError_t e = hipDeviceEnablePeerAccess(d0, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return bail(SG_E_DEVICE);
        }
        (void)hipGetLastError();  // an already-enabled peer leaves its error behind
    }
    if (hipSetDevice(devices[0]) != hipSuccess) return bail(SG_E_DEVICE);
    const uint64_t n = cfg->max_batch;
    if (hipStreamCreateWithFlags(nd->s0.put(), hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(nd->routed.put(), hipEventDisableTiming) != hipSuccess ||
        !nd->d_tile_cnt.alloc_bytes(sizeof(uint32_t) * kMaxShards * (route_tiles(n) + 1)) ||
        !nd->d_base.alloc_bytes(sizeof(uint32_t) * (2 * kMaxShards + 1)) ||
        !nd->d_sub_req.alloc_bytes(sizeof(sg_req) * n) ||
        !nd->d_sub_pos.alloc_bytes(sizeof(uint32_t) * n) ||
        !nd->d_sub_out.alloc_bytes(sizeof(sg_result) * n) ||
        !nd->h_base.alloc_bytes(sizeof(uint32_t) * (2 * kMaxShards + 1)) ||
        !nd->h_front_err.alloc_bytes(sizeof(int)))
        return bail(SG_E_NOMEM);
    *out = nd;
    return SG_OK;
}

int sg_node_set_namespaces(sg_node* nd, const sg_namespace* ns, uint32_t n) {
    if (!nd || (!ns && n)) return SG_E_INVAL;
    node_drain(nd);
    // the front runs every namespace limiter over the node batch (and validates the set); the shards see only admitted
    // requests. A shard that fails (allocation, device) puts the front and the shards before it back on the node's
    // previous namespaces.
    const std::vector<sg_namespace> old = nd->ns;
    auto limiters_off = [](std::vector<sg_namespace> v) {
        for (auto& x : v) x.limiter_enabled = 0;
        return v;
    };
    int rc = sg_set_namespaces(nd->front, ns, n);
    if (rc) return node_child(nd, nd->front, rc);
    const std::vector<sg_namespace> off = limiters_off(std::vector<sg_namespace>(ns, ns + n));
    for (size_t g = 0; g < nd->shards.size(); ++g) {
        rc = sg_set_namespaces(nd->shards[g], off.data(), n);
        if (rc) {
            rc = node_child(nd, nd->shards[g], rc);
            const std::vector<sg_namespace> old_off = limiters_off(old);
            (void)sg_set_namespaces(nd->front, old.data(), (uint32_t)old.size());
            for (size_t x = 0; x < g; ++x) (void)sg_set_namespaces(nd->shards[x], old_off.data(), (uint32_t)old_off.size());
            (void)node_sync_layout(nd);
            return rc;
        }
    }
    nd->ns.assign(ns, ns + n);
    return node_sync_layout(nd);
}

int sg_node_load_flow_rules(sg_node* nd, const sg_flow_rule* rules, uint32_t n) {
    if (!nd || (!rules && n)) return SG_E_INVAL;
    node_drain(nd);
    // All or nothing: the node's rule set is validated on the front, every shard's part and the front's whole set are
    // prepared beside the live state (surviving flowIds' metrics copied: a surviving flowId keeps its owner, hence its
    // ClusterMetric) together with the routing tables, and only when all of that succeeded is anything committed. A
    // failure (validation, allocation, device) leaves the node deciding with its previous rules.
    sg_handle* f = nd->front;
    NHIP(nd, hipSetDevice(nd->devices[0]));
    drain_async(f);
    int rc = flow_rules_validate(f, rules, n);
    if (rc) return node_child(nd, f, rc);
    const uint32_t G = (uint32_t)nd->shards.size();
    std::vector<std::vector<sg_flow_rule>> part(G);
    std::vector<uint8_t> so(n);
    std::vector<uint32_t> lo(n);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t g = node_owner(rules[k].flow_id, G);
        so[k] = (uint8_t)g;
        lo[k] = (uint32_t)part[g].size();
        part[g].push_back(rules[k]);
    }
    std::vector<FlowLoad> prep(G + 1);
    DevBuf<uint8_t> d_so;
    DevBuf<uint32_t> d_lo;
    auto abort_all = [&](uint32_t upto) {  // the prepared shards [0, upto), the front's (index G) and the tables
        for (uint32_t x = 0; x < upto; ++x) {
            (void)hipSetDevice(nd->devices[x]);
            flow_rules_abort(prep[x]);
        }
        (void)hipSetDevice(nd->devices[0]);
        flow_rules_abort(prep[G]);
        d_so.reset();
        d_lo.reset();
    };
    // env SG_TEST_NODE_FAIL_SHARD = g (tests): preparing shard g fails as an allocation would
    const char* inj = std::getenv("SG_TEST_NODE_FAIL_SHARD");
    const int fail_g = inj ? std::atoi(inj) : -1;
    for (uint32_t g = 0; g < G; ++g) {
        sg_handle* h = nd->shards[g];
        NHIP(nd, hipSetDevice(h->device));
        drain_async(h);
        rc = (int)g == fail_g ? fail(h, SG_E_NOMEM, "injected shard load failure (SG_TEST_NODE_FAIL_SHARD)")
                              : flow_rules_validate(h, part[g].data(), (uint32_t)part[g].size());
        if (!rc) rc = flow_rules_prepare(h, part[g].data(), (uint32_t)part[g].size(), prep[g]);
        if (rc) {
            rc = node_child(nd, h, rc);
            abort_all(g);
            return rc;
        }
    }
    NHIP(nd, hipSetDevice(nd->devices[0]));
    rc = flow_rules_prepare(f, rules, n, prep[G]);
    if (!rc && n && (!d_so.alloc_bytes(n) || !d_lo.alloc_bytes(sizeof(uint32_t) * n) ||
                     hipMemcpy(d_so, so.data(), n, hipMemcpyHostToDevice) != hipSuccess ||
                     hipMemcpy(d_lo, lo.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice) != hipSuccess))
        rc = fail(f, SG_E_NOMEM, "routing tables");
    if (rc) {
        rc = node_child(nd, f, rc);
        abort_all(G);
        return rc;
    }
    // commit (host tables and pointer swaps; only the small per-rule uploads can still fail)
    for (uint32_t g = 0; g < G; ++g) {
        NHIP(nd, hipSetDevice(nd->devices[g]));
        rc = flow_rules_commit(nd->shards[g], part[g].data(), (uint32_t)part[g].size(), prep[g]);
        if (rc) return node_child(nd, nd->shards[g], rc);
    }
    NHIP(nd, hipSetDevice(nd->devices[0]));
    rc = flow_rules_commit(f, rules, n, prep[G]);
    if (rc) return node_child(nd, f, rc);
    nd->d_shard_of = std::move(d_so);
    nd->d_local_of = std::move(d_lo);
    nd->rules.assign(rules, rules + n);
    nd->shard_of = so;
    nd->local_of = lo;
    nd->node_key_stale = true;
    return node_sync_layout(nd);
}

sg_handle* sg_node_front(sg_node* nd) { return nd ? nd->front : nullptr; }

int sg_node_shard_of(const sg_node* nd, uint32_t key, uint32_t* shard, uint32_t* local_key) {
    if (!nd || !shard || !local_key || key >= nd->shard_of.size()) return SG_E_INVAL;
    *shard = nd->shard_of[key];
    *local_key = nd->local_of[key];
    return SG_OK;
}

int sg_node_flow_decide_batch(sg_node* nd, const sg_req* req, uint64_t n, sg_result* out, void* stream_) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    sg_handle* f = nd->front;
    const uint32_t G = (uint32_t)nd->shards.size();
    hipStream_t user = (hipStream_t)stream_;
    NHIP(nd, hipSetDevice(nd->devices[0]));
    node_drain(nd);
    int rc = ensure_layout(f);
    if (rc) return node_child(nd, f, rc);
    // 1. the front: validation + namespace limiter in caller order, the batch's time check, its last timestamp, the
    // default results in the caller's buffer, the batch's period tables
    NHIP(nd, hipStreamSynchronize(user));  // the caller's batch is in place
    sg_handle::FlowWs& w = f->ws[0];
    BatchArgs a = flow_args(f, w, req, n, out);
    // one shard holding every rule in the front's order (G = 1): the front's records are its records as they are
    const bool direct = nd->rec_path && G == 1 && nd->shards[0]->K == f->K && nd->shards[0]->kbits == f->kbits;
    if (!direct) a.hist0 = nullptr;
    a.csum0 = nullptr;
    NHIP(nd, hipMemsetAsync(a.err, 0, sizeof(int), nd->s0));
    if (a.hist0 && radix_csum_atomic()) {
        a.csum0 = radix_csum(a.hist0, a.n, a.hist0_bits);
        NHIP(nd, hipMemsetAsync(a.csum0, 0, radix_csum_bytes(a.n, a.hist0_bits), nd->s0));
    }
    NHIP(nd, launch_prep(a, nd->s0));
    rc = flow_limiter(f, a, nd->s0);
    if (rc) return node_child(nd, f, rc);
    NHIP(nd, launch_finish(a, nd->s0));
    // 2. routing by owner (not for one shard on the records path)
    RouteArgs r{};
    r.req = req;
    r.rec = a.rec;
    r.n = n;
    r.kshift = a.kshift;
    r.abits = a.abits;
    r.imask = a.imask;
    r.K = f->K;
    r.shard_of = nd->d_shard_of;
    r.local_of = nd->d_local_of;
    r.G = (int)G;
    r.tile_cnt = nd->d_tile_cnt;
    r.shard_base = nd->d_base;
    r.shard_tot = nd->d_base + kMaxShards + 1;
    r.sub_req = nd->d_sub_req;
    r.sub_pos = nd->d_sub_pos;
    if (nd->rec_path) {
        r.sub_rec = nd->d_sub_rec;
        r.low_mask = (1ull << a.kshift) - 1;
        for (uint32_t g = 0; g < G; ++g) r.skshift[g] = 64 - nd->shards[g]->kbits;
    }
    if (!direct) {
        NHIP(nd, launch_route(r, nd->s0));
        NHIP(nd, hipMemcpyAsync(nd->h_base, nd->d_base, sizeof(uint32_t) * (2 * kMaxShards + 1), hipMemcpyDeviceToHost,
                                nd->s0));
    }
    NHIP(nd, hipMemcpyAsync(nd->h_front_err, a.err, sizeof(int), hipMemcpyDeviceToHost, nd->s0));
    NHIP(nd, hipEventRecord(nd->routed, nd->s0));
    NHIP(nd, hipStreamSynchronize(nd->s0));
    if (*nd->h_front_err) return node_child(nd, f, flow_status(f, *nd->h_front_err));
    if (direct) {
        nd->h_base[0] = 0;
        nd->h_base[kMaxShards + 1] = (uint32_t)n;  // the sentinel records of rejected requests sort to the end
    }
    // 3. every shard decides its slice on its own stream
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t base = nd->h_base[g], cnt = nd->h_base[kMaxShards + 1 + g];
        *nd->sh[g].h_err = 0;
        if (cnt == 0) continue;
        sg_handle* h = nd->shards[g];
        const int dev = nd->devices[g];
        NHIP(nd, hipSetDevice(dev));
        NHIP(nd, hipStreamWaitEvent(nd->sh[g].stream, nd->routed, 0));
        if (nd->rec_path) {
            // the slice's records (node request indices) through the shard's sort and walkers; the period tables,
            // window lengths, requests and results are the node batch's
            sg_handle::FlowWs& sw = h->ws[0];
            BatchArgs b = flow_args(h, sw, req, cnt, out);
            b.rec = direct ? a.rec : nd->d_sub_rec + base;
            b.rec_sorted = direct ? h->ws[0].rec_sorted : sw.rec;  // the sort's other buffer
            b.hist0 = direct ? a.hist0 : nullptr;
            b.hist0_bits = a.hist0_bits;
            b.csum0 = direct ? a.csum0 : nullptr;
            b.n_wl = a.n_wl;
            std::memcpy(b.wl, a.wl, sizeof(b.wl));
            b.bnd = a.bnd;
            b.p0 = a.p0;
            b.np = a.np;
            b.walk_cus = node_walk_cus(nd, g, 0);
            hipStream_t st = nd->sh[g].stream;
            rc = node_shard_rec(h, b, cnt, n, direct ? w.hist : sw.hist, st, st, h->aux, h->fork, h->join, nullptr,
                                nd->sh[g].h_err);
            if (rc) {
                node_sync_shards(nd, g + 1);
                return node_child(nd, h, rc);
            }
        } else {
            const sg_req* sreq = nd->d_sub_req + base;
            sg_result* sout = nd->d_sub_out + base;
            if (dev != nd->devices[0]) {
                NHIP(nd, hipMemcpyPeerAsync(nd->sh[g].r_req, dev, sreq, nd->devices[0], sizeof(sg_req) * cnt, nd->sh[g].stream));
                sreq = nd->sh[g].r_req;
                sout = nd->sh[g].r_out;
            }
            rc = enqueue_flow(h, sreq, cnt, sout, nd->sh[g].stream, nd->sh[g].h_err, false);
            if (rc) {
                node_sync_shards(nd, g + 1);
                return node_child(nd, h, rc);
            }
            if (dev != nd->devices[0])
                NHIP(nd, hipMemcpyPeerAsync(nd->d_sub_out + base, nd->devices[0], sout, dev, sizeof(sg_result) * cnt,
                                            nd->sh[g].stream));
        }
        NHIP(nd, hipEventRecord(nd->sh[g].done, nd->sh[g].stream));
    }
    // 4. back into caller order (the sub_req path; the records path wrote the results in place)
    NHIP(nd, hipSetDevice(nd->devices[0]));
    for (uint32_t g = 0; g < G; ++g)
        if (nd->h_base[kMaxShards + 1 + g]) NHIP(nd, hipStreamWaitEvent(nd->s0, nd->sh[g].done, 0));
    if (!nd->rec_path) NHIP(nd, launch_route_gather(nd->d_sub_out, nd->d_sub_pos, nd->h_base[G], out, nd->s0));
    NHIP(nd, hipEventRecord(nd->routed, nd->s0));
    NHIP(nd, hipStreamWaitEvent(user, nd->routed, 0));
    NHIP(nd, hipStreamSynchronize(nd->s0));
    for (uint32_t g = 0; g < G; ++g) {
        const int e = *nd->sh[g].h_err;
        if (e) return node_child(nd, nd->shards[g], flow_status(nd->shards[g], e));
    }
    return SG_OK;
}

int sg_node_flow_decide_batch_host(sg_node* nd, const sg_req* req, uint64_t n, sg_result* out) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    return host_batch(nd, nd->devices[0], req, n, out, [&](sg_req* d_req, sg_result* d_out) {
        return sg_node_flow_decide_batch(nd, d_req, n, d_out, nullptr);
    });
}

int sg_node_flow_enqueue(sg_node* nd, const sg_req* req, uint64_t n, sg_result* out, uint64_t* ticket) {
    if (!nd || !ticket) return SG_E_INVAL;
    *ticket = 0;
    if (n == 0) return SG_OK;
    if (!req || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    sg_handle* f = nd->front;
    const uint32_t G = (uint32_t)nd->shards.size();
    NHIP(nd, hipSetDevice(nd->devices[0]));
    int rc = ensure_layout(f);
    if (rc) return node_child(nd, f, rc);
    if (!nd->rec_path) {  // shards on other devices: the synchronous node batch, its status kept for the ticket
        rc = sg_node_flow_decide_batch(nd, req, n, out, nullptr);
        if (rc == SG_E_DEVICE) return rc;
        *ticket = nd->next_ticket++;
        nd->finished[*ticket] = rc;
        return SG_OK;
    }
    rc = pipe_setup(f);
    if (rc) return node_child(nd, f, rc);
    for (sg_handle* h : nd->shards) {
        rc = pipe_setup(h);
        if (rc) return node_child(nd, h, rc);
    }
    const int x = (int)(nd->pseq & 1);
    sg_node::PipeSlot& sl = nd->pipe[x];
    if (!sl.done) {
        if (hipEventCreateWithFlags(sl.done.put(), hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(nd->fdone[x].put(), hipEventDisableTiming) != hipSuccess ||
            !sl.h_err.alloc_bytes(sizeof(int) * kMaxShards) ||
            !sl.h_base.alloc_bytes(sizeof(uint32_t) * (2 * kMaxShards + 1)))
            return nfail(nd, SG_E_NOMEM, "node pipeline slot");
    }
    if (x == 1 && !nd->d_sub_rec2 && !nd->d_sub_rec2.alloc_bytes(sizeof(uint64_t) * (nd->cfg.max_batch + kRecW)))
        return nfail(nd, SG_E_NOMEM, "shard record slices");
    if (sl.ticket) {  // the batch two back used this workspace: complete it (its status waits in `finished`)
        const hipError_t e = hipEventSynchronize(sl.done);
        nd->finished[sl.ticket] = e != hipSuccess ? nfail(nd, SG_E_DEVICE, hipGetErrorString(e)) : node_slot_status(nd, sl);
        sl.ticket = 0;
    }
    // 1. the front on its pipeline stream: validation, the namespace limiter in caller order, the time check against
    // the previous node batch (the front's own last timestamp, in stream order), the period tables, the routing
    sg_handle::FlowWs& w = f->ws[x];
    BatchArgs a = flow_args(f, w, req, n, out);
    const bool direct = G == 1 && nd->shards[0]->K == f->K && nd->shards[0]->kbits == f->kbits;
    if (!direct) a.hist0 = nullptr;
    a.csum0 = nullptr;
    hipStream_t fs = f->s_front;
    if (nd->pseq >= 2) NHIP(nd, hipStreamWaitEvent(fs, sl.done, 0));
    NHIP(nd, hipMemsetAsync(a.err, 0, sizeof(int), fs));
    if (a.hist0 && radix_csum_atomic()) {
        a.csum0 = radix_csum(a.hist0, a.n, a.hist0_bits);
        NHIP(nd, hipMemsetAsync(a.csum0, 0, radix_csum_bytes(a.n, a.hist0_bits), fs));
    }
    NHIP(nd, launch_prep(a, fs));
    rc = flow_limiter(f, a, fs);
    if (rc) return node_child(nd, f, rc);
    NHIP(nd, launch_finish(a, fs));
    uint64_t* sub_rec = x == 0 ? nd->d_sub_rec : nd->d_sub_rec2;
    if (!direct) {
        RouteArgs r{};
        r.req = req;
        r.rec = a.rec;
        r.n = n;
        r.kshift = a.kshift;
        r.abits = a.abits;
        r.imask = a.imask;
        r.K = f->K;
        r.shard_of = nd->d_shard_of;
        r.local_of = nd->d_local_of;
        r.G = (int)G;
        r.tile_cnt = nd->d_tile_cnt;
        r.shard_base = nd->d_base;
        r.shard_tot = nd->d_base + kMaxShards + 1;
        r.sub_req = nd->d_sub_req;
        r.sub_pos = nd->d_sub_pos;
        r.sub_rec = sub_rec;
        r.low_mask = (1ull << a.kshift) - 1;
        for (uint32_t g = 0; g < G; ++g) r.skshift[g] = 64 - nd->shards[g]->kbits;
        NHIP(nd, launch_route(r, fs));
        NHIP(nd, hipMemcpyAsync(sl.h_base, nd->d_base, sizeof(uint32_t) * (2 * kMaxShards + 1), hipMemcpyDeviceToHost, fs));
    }
    NHIP(nd, hipMemcpyAsync(nd->h_front_err, a.err, sizeof(int), hipMemcpyDeviceToHost, fs));
    NHIP(nd, hipEventRecord(nd->fdone[x], fs));
    // the slice sizes are launch parameters of the shards' sorts: wait for the front (the shards' walkers of the
    // previous batch keep the device busy meanwhile)
    NHIP(nd, hipEventSynchronize(nd->fdone[x]));
    const uint64_t t = nd->next_ticket++;
    *ticket = t;
    if (*nd->h_front_err) {  // refused as a whole (nothing reached the shards)
        nd->finished[t] = node_child(nd, f, flow_status(f, *nd->h_front_err));
        NHIP(nd, hipEventRecord(sl.done, fs));
        sl.G_used = 0;
        nd->pseq++;
        return SG_OK;
    }
    if (direct) {
        sl.h_base[0] = 0;
        sl.h_base[kMaxShards + 1] = (uint32_t)n;
    }
    // 2. every shard: its sort on its front stream (beside its walkers of the previous batch), then its walkers, one
    // shard after another from this thread (enqueueing them from one host thread per shard was slower: 3.5 -> 6.0 ms
    // per G = 4 node batch, r06, the HIP runtime serialising the threads' launches)
    std::vector<int> src(G, SG_OK);
    auto enqueue_shard = [&](uint32_t g) {
        sl.h_err[g] = 0;
        const uint32_t base = sl.h_base[g], cnt = sl.h_base[kMaxShards + 1 + g];
        if (cnt == 0) return;
        sg_handle* h = nd->shards[g];
        if (hipSetDevice(h->device) != hipSuccess) {
            src[g] = SG_E_DEVICE;
            return;
        }
        sg_handle::FlowWs& sw = h->ws[x];
        BatchArgs b = flow_args(h, sw, req, cnt, out);
        b.rec = direct ? a.rec : sub_rec + base;
        b.rec_sorted = direct ? sw.rec_sorted : sw.rec;
        b.hist0 = direct ? a.hist0 : nullptr;
        b.hist0_bits = a.hist0_bits;
        b.csum0 = direct ? a.csum0 : nullptr;
        b.n_wl = a.n_wl;
        std::memcpy(b.wl, a.wl, sizeof(b.wl));
        b.bnd = a.bnd;
        b.p0 = a.p0;
        b.np = a.np;
        b.walk_cus = node_walk_cus(nd, g, h->walk_cus);
        if (hipStreamWaitEvent(h->s_front, nd->fdone[x], 0) != hipSuccess) {
            src[g] = SG_E_DEVICE;
            return;
        }
        src[g] = node_shard_rec(h, b, cnt, n, direct ? w.hist : sw.hist, h->s_front, h->s_back, h->s_aux2, h->pfork,
                                h->pjoin, h->front_done[x], &sl.h_err[g]);
        if (src[g] == SG_OK && hipEventRecord(h->back_done[x], h->s_back) != hipSuccess) src[g] = SG_E_DEVICE;
    };
    for (uint32_t g = 0; g < G; ++g) {
        enqueue_shard(g);
        if (src[g] != SG_OK) break;
    }
    NHIP(nd, hipSetDevice(nd->devices[0]));
    for (uint32_t g = 0; g < G; ++g) {
        if (src[g] == SG_OK) continue;
        for (uint32_t q = 0; q < G; ++q) {
            (void)hipStreamSynchronize(nd->shards[q]->s_front);
            (void)hipStreamSynchronize(nd->shards[q]->s_back);
        }
        nd->finished.erase(t);
        *ticket = 0;
        return src[g] == SG_E_DEVICE ? nfail(nd, SG_E_DEVICE, "shard enqueue") : node_child(nd, nd->shards[g], src[g]);
    }
    for (uint32_t g = 0; g < G; ++g)
        if (sl.h_base[kMaxShards + 1 + g]) NHIP(nd, hipStreamWaitEvent(nd->s0, nd->shards[g]->back_done[x], 0));
    NHIP(nd, hipEventRecord(sl.done, nd->s0));
    sl.G_used = G;
    sl.ticket = t;
    nd->pseq++;
    return SG_OK;
}

static int node_collect(sg_node* nd, uint64_t ticket, bool block) {
    if (!nd) return SG_E_INVAL;
    if (ticket == 0) return 1;
    auto it = nd->finished.find(ticket);
    if (it != nd->finished.end()) {
        const int st = it->second;
        nd->finished.erase(it);
        return st == SG_OK ? 1 : st;
    }
    for (auto& sl : nd->pipe) {
        if (sl.ticket != ticket) continue;
        (void)hipSetDevice(nd->devices[0]);
        const hipError_t e = block ? hipEventSynchronize(sl.done) : hipEventQuery(sl.done);
        if (e == hipErrorNotReady) return 0;
        sl.ticket = 0;
        if (e != hipSuccess) return nfail(nd, SG_E_DEVICE, hipGetErrorString(e));
        const int st = node_slot_status(nd, sl);
        return st == SG_OK ? 1 : st;
    }
    return nfail(nd, SG_E_INVAL, "unknown or already collected ticket");
}

// One fetch over several handles, for both logs. Phase 1 asks every handle for its row count with cap 0, which
// changes nothing there (a handle without complete rows answers SG_OK and has handed out its lost totals: they are
// kept in lost[]); the sum, with the rows held from an earlier failed fetch, is what the caller's cap must hold.
// Phase 2 takes each handle's rows into held[]; an error ends the call with the rows taken so far still held.
extern "C++" {
template <class Row, class Fetch>
static int node_log_fetch(sg_node* nd, const std::vector<sg_handle*>& hs, Fetch fetch, std::vector<Row>& held,
                          uint64_t* lost, uint64_t cap, uint64_t* n_rows) {
    std::vector<uint64_t> need(hs.size(), 0);
    uint64_t sum = held.size();
    for (size_t g = 0; g < hs.size(); ++g) {
        uint64_t le = 0, lc = 0;
        const int rc = fetch(hs[g], (Row*)nullptr, 0, &need[g], &le, &lc);
        if (rc == SG_OK) {
            lost[0] += le;
            lost[1] += lc;
        } else if (rc != SG_E_CAPACITY) {
            return node_child(nd, hs[g], rc);
        }
        sum += need[g];
    }
    *n_rows = sum;
    if (sum > cap) return nfail(nd, SG_E_CAPACITY, "log rows exceed cap");
    for (size_t g = 0; g < hs.size(); ++g) {
        if (!need[g]) continue;
        std::vector<Row> tmp((size_t)need[g]);
        uint64_t m = 0, le = 0, lc = 0;
        const int rc = fetch(hs[g], tmp.data(), need[g], &m, &le, &lc);
        if (rc) return node_child(nd, hs[g], rc);
        held.insert(held.end(), tmp.begin(), tmp.begin() + (size_t)m);
        lost[0] += le;
        lost[1] += lc;
    }
    return SG_OK;
}
}  // extern "C++"

static std::vector<sg_handle*> node_log_handles(sg_node* nd, bool with_front) {
    std::vector<sg_handle*> hs;
    if (with_front && nd->front) hs.push_back(nd->front);
    hs.insert(hs.end(), nd->shards.begin(), nd->shards.end());
    return hs;
}

int sg_node_server_log_enable(sg_node* nd, int32_t capacity_log2) {
    if (!nd) return SG_E_INVAL;
    if (!slog_capacity_ok(capacity_log2)) return nfail(nd, SG_E_INVAL, "capacity_log2 outside 4..24");
    if (nd->slog_log2)
        return capacity_log2 == nd->slog_log2 ? SG_OK : nfail(nd, SG_E_INVAL, "the server log has another capacity");
    node_drain(nd);
    for (sg_handle* h : node_log_handles(nd, true)) {  // the front too: it decides param tokens under a limiter
        const int rc = sg_server_log_enable(h, capacity_log2);
        if (rc) return node_child(nd, h, rc);  // the handles before it stay on; the same call again completes the rest
    }
    nd->slog_log2 = capacity_log2;
    return SG_OK;
}

int sg_node_server_log(sg_node* nd, int64_t now_ms, sg_server_row* rows, uint64_t cap, uint64_t* n_rows,
                       uint64_t* lost_events, uint64_t* lost_count) {
    if (!nd || !n_rows || !lost_events || !lost_count || (!rows && cap)) return SG_E_INVAL;
    *n_rows = *lost_events = *lost_count = 0;
    if (!nd->slog_log2) return nfail(nd, SG_E_INVAL, "sg_node_server_log_enable first");
    node_drain(nd);
    const int rc = node_log_fetch<sg_server_row>(
        nd, node_log_handles(nd, true),
        [&](sg_handle* h, sg_server_row* r, uint64_t c, uint64_t* n, uint64_t* le, uint64_t* lc) {
            return sg_server_log(h, now_ms, r, c, n, le, lc);
        },
        nd->slog_held, nd->slog_lost, cap, n_rows);
    if (rc) return rc;
    slog_sort_merge(nd->slog_held);  // a rule served by the front and by a shard stays one row
    *n_rows = nd->slog_held.size();
    std::copy(nd->slog_held.begin(), nd->slog_held.end(), rows);
    nd->slog_held.clear();
    *lost_events = nd->slog_lost[0];
    *lost_count = nd->slog_lost[1];
    nd->slog_lost[0] = nd->slog_lost[1] = 0;
    return SG_OK;
}

int sg_node_local_block_log_enable(sg_node* nd, int32_t capacity_log2) {
    if (!nd) return SG_E_INVAL;
    if (capacity_log2 < 4 || capacity_log2 > 24) return nfail(nd, SG_E_INVAL, "capacity_log2 outside 4..24");
    if (nd->blog_log2)
        return capacity_log2 == nd->blog_log2 ? SG_OK : nfail(nd, SG_E_INVAL, "the block log has another capacity");
    node_drain(nd);
    for (sg_handle* h : nd->shards) {
        const int rc = sg_local_block_log_enable(h, capacity_log2);
        if (rc) return node_child(nd, h, rc);  // the shards before it stay on; the same call again completes the rest
    }
    nd->blog_log2 = capacity_log2;
    return SG_OK;
}

int sg_node_local_block_log(sg_node* nd, int64_t now_ms, sg_block_row* rows, uint64_t cap, uint64_t* n_rows,
                            uint64_t* lost_events, uint64_t* lost_count) {
    if (!nd || !n_rows || !lost_events || !lost_count || (!rows && cap)) return SG_E_INVAL;
    *n_rows = *lost_events = *lost_count = 0;
    if (!nd->blog_log2) return nfail(nd, SG_E_INVAL, "sg_node_local_block_log_enable first");
    node_drain(nd);
    const int rc = node_log_fetch<sg_block_row>(
        nd, node_log_handles(nd, false),
        [&](sg_handle* h, sg_block_row* r, uint64_t c, uint64_t* n, uint64_t* le, uint64_t* lc) {
            return sg_local_block_log(h, now_ms, r, c, n, le, lc);
        },
        nd->blog_held, nd->blog_lost, cap, n_rows);
    if (rc) return rc;
    auto key = [](const sg_block_row& x) {
        return std::tie(x.timestamp, x.resource, x.status, x.app_kind, x.app, x.origin);
    };
    std::sort(nd->blog_held.begin(), nd->blog_held.end(),
              [&](const sg_block_row& x, const sg_block_row& y) { return key(x) < key(y); });
    // a resource has one owner shard, so no key comes from two of them: checked, not trusted (the rows stay held)
    for (size_t i = 1; i < nd->blog_held.size(); ++i)
        if (key(nd->blog_held[i - 1]) == key(nd->blog_held[i]))
            return nfail(nd, SG_E_DEVICE, "a block log key came from two shards: a resource has one owner");
    *n_rows = nd->blog_held.size();
    std::copy(nd->blog_held.begin(), nd->blog_held.end(), rows);
    nd->blog_held.clear();
    *lost_events = nd->blog_lost[0];
    *lost_count = nd->blog_lost[1];
    nd->blog_lost[0] = nd->blog_lost[1] = 0;
    return SG_OK;
}

int sg_node_flow_poll(sg_node* nd, uint64_t ticket) { return node_collect(nd, ticket, false); }

int sg_node_flow_wait(sg_node* nd, uint64_t ticket) {
    const int r = node_collect(nd, ticket, true);
    return r == 1 ? SG_OK : r;
}

int sg_node_flow_read_state(sg_node* nd, uint32_t key, int64_t* starts, int64_t* counters, int64_t* occupy) {
    if (!nd || key >= nd->shard_of.size()) return SG_E_INVAL;
    node_drain(nd);
    sg_handle* h = nd->shards[nd->shard_of[key]];
    return node_child(nd, h, sg_flow_read_state(h, nd->local_of[key], starts, counters, occupy));
}

int sg_node_snapshot_metrics(sg_node* nd, int64_t now_ms, double* out, uint64_t cap) {
    if (!nd || (!out && cap)) return SG_E_INVAL;
    node_drain(nd);
    const uint64_t K = nd->shard_of.size();
    if (cap < 2 * K) return nfail(nd, SG_E_CAPACITY, "snapshot buffer smaller than 2 * rules");
    if (K == 0) return SG_OK;
    // ClusterMetricNodeGenerator.generateCurrentNodeMap (ClusterMetricNodeGenerator.java:39-61) over the node: every
    // shard's {passQps, blockQps} computed on its device, moved to the front's device (peer copies), scattered into
    // node rule order there, one copy to the host
    const uint32_t G = (uint32_t)nd->shards.size();
    NHIP(nd, hipSetDevice(nd->devices[0]));
    if (nd->node_key_stale || nd->d_node_key.size() != G) {
        nd->d_node_key.clear();
        nd->d_node_key.resize(G);
        std::vector<std::vector<uint32_t>> keys(G);
        for (uint64_t k = 0; k < K; ++k) {
            auto& v = keys[nd->shard_of[k]];
            if (v.size() <= nd->local_of[k]) v.resize(nd->local_of[k] + 1);
            v[nd->local_of[k]] = (uint32_t)k;
        }
        for (uint32_t g = 0; g < G; ++g) {
            if (keys[g].empty()) continue;
            if (!nd->d_node_key[g].alloc_bytes(sizeof(uint32_t) * keys[g].size()))
                return nfail(nd, SG_E_NOMEM, "node snapshot keys");
            NHIP(nd, hipMemcpy(nd->d_node_key[g], keys[g].data(), sizeof(uint32_t) * keys[g].size(), hipMemcpyHostToDevice));
        }
        nd->node_key_stale = false;
    }
    uint64_t part_max = 0;
    for (sg_handle* h : nd->shards) part_max = std::max<uint64_t>(part_max, h->K);
    const uint64_t need = 2 * K + 2 * part_max;  // the node's rows, then one shard part staged on the front
    if (!nd->d_snap.reserve(need)) return nfail(nd, SG_E_NOMEM, "node snapshot");
    double* stage = nd->d_snap + 2 * K;
    for (uint32_t g = 0; g < G; ++g) {
        sg_handle* h = nd->shards[g];
        if (h->K == 0) continue;
        const int dev = nd->devices[g];
        double* part = stage;
        if (dev != nd->devices[0]) {  // computed on its device, then copied over xGMI
            NHIP(nd, hipSetDevice(dev));
            // regrown with the rules: a reload may give this shard more of them than the first snapshot saw
            if (!nd->sh[g].r_snap.reserve(2 * part_max)) return nfail(nd, SG_E_NOMEM, "node snapshot part");
            part = nd->sh[g].r_snap;
        }
        NHIP(nd, launch_snapshot(h->d_rules, h->d_ring, h->d_occ, h->K, h->stride, now_ms, part, nd->sh[g].stream));
        NHIP(nd, hipStreamSynchronize(nd->sh[g].stream));
        NHIP(nd, hipSetDevice(nd->devices[0]));
        if (dev != nd->devices[0])
            NHIP(nd, hipMemcpyPeerAsync(stage, nd->devices[0], part, dev, sizeof(double) * 2 * h->K, nd->s0));
        NHIP(nd, launch_nsnap_scatter(stage, nd->d_node_key[g], h->K, nd->d_snap, nd->s0));
        NHIP(nd, hipStreamSynchronize(nd->s0));  // the stage is reused by the next shard
    }
    NHIP(nd, hipMemcpy(out, nd->d_snap, sizeof(double) * 2 * K, hipMemcpyDeviceToHost));
    return SG_OK;
}

// ---- cluster param and concurrent tokens over the node ----

int sg_node_cparam_load_rules(sg_node* nd, const sg_cparam_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                              uint32_t n_hot, int32_t capacity_log2) {
    if (!nd || (!rules && n) || (!hot && n_hot)) return SG_E_INVAL;
    node_drain(nd);
    // ClusterParamFlowRuleManager over the node: a rule (and its hot items) lives on the shard owning its flowId. The
    // shards' loads are validated by each shard; a failing one leaves the earlier shards on the new rules (node-wide
    // all-or-nothing is the flow rules' contract, not this one's: reload after a failure)
    const uint32_t G = (uint32_t)nd->shards.size();
    for (uint32_t i = 0; i < n; ++i)
        if ((uint64_t)rules[i].hot_begin + rules[i].hot_count > n_hot) return nfail(nd, SG_E_INVAL, "hot item range out of bounds");
    std::vector<std::vector<sg_cparam_rule>> part(G);
    std::vector<std::vector<sg_param_hot_item>> hp(G);
    std::vector<uint8_t> so(n);
    std::vector<uint32_t> lo(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = node_owner(rules[i].flow_id, G);
        so[i] = (uint8_t)g;
        lo[i] = (uint32_t)part[g].size();
        sg_cparam_rule r = rules[i];
        r.hot_begin = (uint32_t)hp[g].size();
        hp[g].insert(hp[g].end(), hot + rules[i].hot_begin, hot + rules[i].hot_begin + rules[i].hot_count);
        part[g].push_back(r);
    }
    for (uint32_t g = 0; g < G; ++g) {
        sg_handle* h = nd->shards[g];
        NHIP(nd, hipSetDevice(h->device));
        const int rc = sg_cparam_load_rules(h, part[g].data(), (uint32_t)part[g].size(), hp[g].data(),
                                            (uint32_t)hp[g].size(), capacity_log2);
        if (rc) return node_child(nd, h, rc);
    }
    NHIP(nd, hipSetDevice(nd->devices[0]));
    nd->d_cp_shard_of.reset();
    nd->d_cp_local_of.reset();
    if (n && (!nd->d_cp_shard_of.alloc_bytes(n) || !nd->d_cp_local_of.alloc_bytes(sizeof(uint32_t) * n)))
        return nfail(nd, SG_E_NOMEM, "param routing tables");
    if (n) {
        NHIP(nd, hipMemcpy(nd->d_cp_shard_of, so.data(), n, hipMemcpyHostToDevice));
        NHIP(nd, hipMemcpy(nd->d_cp_local_of, lo.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    }
    nd->cp_rules.assign(rules, rules + n);
    nd->cp_shard_of = so;
    nd->cp_local_of = lo;
    return SG_OK;
}

}  // extern "C"

namespace {

// Scratch of the node's param / concurrent routing, sized for max_batch requests (values: n_values).
int node_nreq_scratch(sg_node* nd, uint64_t n_values) {
    const uint64_t n = nd->cfg.max_batch;
    NHIP(nd, hipSetDevice(nd->devices[0]));
    if (!nd->d_nrec) {
        if (!nd->d_nrec.alloc_bytes(8 * n) || !nd->d_nrec2.alloc_bytes(8 * n) ||
            !nd->d_nhist.alloc_bytes(sizeof(uint32_t) * radix_hist_words(n)) ||
            !nd->d_nvals.alloc_bytes(sizeof(uint32_t) * n) ||
            !nd->d_ncnt.alloc_bytes(sizeof(uint32_t) * 3 * kMaxShards) ||
            !nd->d_ntsum.alloc_bytes(sizeof(uint32_t) * (nreq_tiles(n) + 1)) ||
            !nd->d_nerr.alloc_bytes(sizeof(int)) ||
            !nd->d_sub_nreq.alloc_bytes(std::max(sizeof(sg_cparam_req), sizeof(sg_conc_req)) * n) ||
            !nd->d_sub_nout.alloc_bytes(std::max(sizeof(sg_result), sizeof(sg_conc_result)) * n))
            return nfail(nd, SG_E_NOMEM, "node token routing scratch");
    }
    if (!nd->d_sub_vals.reserve(n_values)) return nfail(nd, SG_E_NOMEM, "node param values");
    return SG_OK;
}

// The node batch's slices (stable by owner): per-shard request bases / counts and value bases / counts on the host.
int node_nreq_route(sg_node* nd, NodeReqArgs q, std::vector<uint64_t>& base, std::vector<uint64_t>& cnt,
                    std::vector<uint64_t>& vbase, std::vector<uint64_t>& vcnt) {
    const uint32_t G = (uint32_t)nd->shards.size();
    hipStream_t st = nd->s0;
    q.G = (int)G;
    q.rec = nd->d_nrec;
    q.nvals = nd->d_nvals;
    q.cnt = nd->d_ncnt;
    q.vcnt = nd->d_ncnt + kMaxShards;
    q.tsum = nd->d_ntsum;
    q.vbase = nd->d_ncnt + 2 * kMaxShards;
    q.sub_vals = nd->d_sub_vals;
    q.sub_pos = nd->d_sub_pos;
    q.err = nd->d_nerr;
    NHIP(nd, hipMemsetAsync(nd->d_ncnt, 0, sizeof(uint32_t) * 2 * kMaxShards, st));
    NHIP(nd, hipMemsetAsync(nd->d_nerr, 0, sizeof(int), st));
    NHIP(nd, launch_nreq_keys(q, st));
    uint32_t h_cnt[2 * kMaxShards];
    int err = 0;
    NHIP(nd, hipMemcpyAsync(h_cnt, nd->d_ncnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    NHIP(nd, hipMemcpyAsync(&err, nd->d_nerr, sizeof(int), hipMemcpyDeviceToHost, st));
    NHIP(nd, hipStreamSynchronize(st));
    if (err & kErrTime)
        return nfail(nd, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than the node's earlier batches");
    if (err & kErrBounds) return nfail(nd, SG_E_INVAL, "a request's values lie outside the value array");
    base.assign(G, 0);
    cnt.assign(G, 0);
    vbase.assign(G, 0);
    vcnt.assign(G, 0);
    uint32_t vb[kMaxShards] = {};
    uint64_t b = 0, v = 0;
    for (uint32_t g = 0; g < G; ++g) {
        base[g] = b;
        cnt[g] = h_cnt[g];
        vbase[g] = v;
        vcnt[g] = h_cnt[kMaxShards + g];
        vb[g] = (uint32_t)v;
        b += cnt[g];
        v += vcnt[g];
    }
    NHIP(nd, hipMemcpyAsync(nd->d_ncnt + 2 * kMaxShards, vb, sizeof(vb), hipMemcpyHostToDevice, st));
    uint64_t* sorted = nullptr;
    NHIP(nd, radix_sort_records(nd->d_nrec, nd->d_nrec2, q.n, 56, nd->d_nhist, &sorted, st, 64));
    NHIP(nd, launch_nreq_gather(q, sorted, st));
    NHIP(nd, hipStreamSynchronize(st));
    return SG_OK;
}

// Buffers for shard g's slice on its own device (shards off the front's device; grown as needed): requests,
// results, values.
int node_slice_alloc(sg_node* nd, uint32_t g, uint64_t nv) {
    const int dev = nd->devices[g];
    if (dev == nd->devices[0]) return SG_OK;
    NHIP(nd, hipSetDevice(dev));
    const uint64_t n = nd->cfg.max_batch;
    if (!nd->sh[g].r_nreq && (!nd->sh[g].r_nreq.alloc_bytes(std::max(sizeof(sg_cparam_req), sizeof(sg_conc_req)) * n) ||
                           !nd->sh[g].r_nout.alloc_bytes(std::max(sizeof(sg_result), sizeof(sg_conc_result)) * n)))
        return nfail(nd, SG_E_NOMEM, "shard slice buffers");
    if (!nd->sh[g].r_vals.reserve(nv)) return nfail(nd, SG_E_NOMEM, "shard values");
    return SG_OK;
}

// Shard g's part of a node token batch, run by `decide(h, req, vals, out, stream)` on the shard's slice [base, base +
// cnt) of the routed requests (req_b / out_b bytes each; nv values from svals): peer copies in and out for a shard
// off the front's device; `decide` gets the shard's index first (what else its slice needs, it moves itself). Every
// shard with work runs in its own host thread — a shard's call waits on the host
// between its own kernels (the param fixed point's rounds, the concurrent batch's error check), so the shards overlap
// whether they share a device or not. The first failure is reported after all have finished.
template <class Decide>
int node_run_shards(sg_node* nd, const std::vector<uint64_t>& base, const std::vector<uint64_t>& cnt,
                    const std::vector<uint64_t>& vbase, const std::vector<uint64_t>& vcnt, size_t req_b, size_t out_b,
                    const void* sub_req, void* sub_out, Decide decide) {
    const uint32_t G = (uint32_t)nd->shards.size();
    for (uint32_t g = 0; g < G; ++g)
        if (cnt[g]) {
            const int rc = node_slice_alloc(nd, g, vcnt[g]);
            if (rc) return rc;
        }
    std::vector<int> rc(G, SG_OK);
    std::vector<char> child(G, 0);
    std::vector<std::string> msg(G);
    auto run = [&](uint32_t g) {
        sg_handle* h = nd->shards[g];
        const int dev = h->device;
        const bool remote = dev != nd->devices[0];
        const char* sreq = static_cast<const char*>(sub_req) + req_b * base[g];
        const uint64_t* svals = nd->d_sub_vals + vbase[g];
        char* sout = static_cast<char*>(sub_out) + out_b * base[g];
        hipError_t e = hipSetDevice(dev);
        const void* req = sreq;
        const uint64_t* vals = svals;
        void* out = sout;
        if (remote) {
            if (e == hipSuccess) e = hipMemcpyPeer(nd->sh[g].r_nreq, dev, sreq, nd->devices[0], req_b * cnt[g]);
            if (e == hipSuccess && vcnt[g]) e = hipMemcpyPeer(nd->sh[g].r_vals, dev, svals, nd->devices[0], 8 * vcnt[g]);
            req = nd->sh[g].r_nreq;
            vals = nd->sh[g].r_vals;
            out = nd->sh[g].r_nout;
        }
        if (e != hipSuccess) {
            rc[g] = SG_E_DEVICE;
            msg[g] = hipGetErrorString(e);
            return;
        }
        const int r = decide(g, h, req, vcnt[g] ? vals : nullptr, vcnt[g], cnt[g], out, nd->sh[g].stream);
        if (r) {
            rc[g] = r;
            child[g] = 1;
            return;
        }
        e = hipStreamSynchronize(nd->sh[g].stream);
        if (e == hipSuccess && remote) e = hipMemcpyPeer(sout, nd->devices[0], out, dev, out_b * cnt[g]);
        if (e != hipSuccess) {
            rc[g] = SG_E_DEVICE;
            msg[g] = hipGetErrorString(e);
        }
    };
    std::vector<uint32_t> work;
    for (uint32_t g = 0; g < G; ++g)
        if (cnt[g]) work.push_back(g);
    if (work.size() == 1) {
        run(work[0]);
    } else {
        std::vector<std::thread> th;
        th.reserve(work.size());
        for (uint32_t g : work) th.emplace_back(run, g);
        for (auto& t : th) t.join();
    }
    (void)hipSetDevice(nd->devices[0]);
    for (uint32_t g : work) {
        if (!rc[g]) continue;
        if (child[g]) return node_child(nd, nd->shards[g], rc[g]);
        return nfail(nd, rc[g], msg[g].c_str());
    }
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_node_cparam_decide_batch(sg_node* nd, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                                uint64_t n_values, sg_result* out, void* stream) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out || (!values && n_values)) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    if (n_values >= (1ull << 32)) return nfail(nd, SG_E_CAPACITY, "more than 2^32 values");
    node_drain(nd);
    // allowProceed (ClusterParamFlowChecker.java:43-45) needs the namespace's limiter in the node's caller order: the
    // node's param path serves namespaces without one
    for (const auto& r : nd->cp_rules)
        if (r.namespace_id >= 0 && (size_t)r.namespace_id < nd->ns.size() && nd->ns[r.namespace_id].limiter_enabled)
            return nfail(nd, SG_E_UNSUPPORTED, "node param tokens with a namespace limiter (use one handle, or the "
                                               "sharded limiter exchange)");
    int rc = node_nreq_scratch(nd, n_values ? n_values : 1);
    if (rc) return rc;
    NodeReqArgs q{};
    q.n = n;
    q.cp = req;
    q.values = values;
    q.n_values = n_values;
    q.K = (uint32_t)nd->cp_rules.size();
    q.shard_of = nd->d_cp_shard_of;
    q.local_of = nd->d_cp_local_of;
    q.sub_cp = reinterpret_cast<sg_cparam_req*>(nd->d_sub_nreq.get());
    q.last_ts = nd->cp_last_ts;
    NHIP(nd, hipStreamSynchronize((hipStream_t)stream));  // the caller's batch is in place (synchronous call)
    std::vector<uint64_t> base, cnt, vbase, vcnt;
    rc = node_nreq_route(nd, q, base, cnt, vbase, vcnt);
    if (rc) return rc;
    sg_result* sub_out = reinterpret_cast<sg_result*>(nd->d_sub_nout.get());
    rc = node_run_shards(nd, base, cnt, vbase, vcnt, sizeof(sg_cparam_req), sizeof(sg_result), q.sub_cp, sub_out,
                         [](uint32_t, sg_handle* h, const void* r, const uint64_t* v, uint64_t nv, uint64_t c, void* o,
                            hipStream_t st) {
                             return sg_cparam_decide_batch(h, static_cast<const sg_cparam_req*>(r), c, v, nv,
                                                           static_cast<sg_result*>(o), st);
                         });
    if (rc) return rc;
    NHIP(nd, hipSetDevice(nd->devices[0]));
    NHIP(nd, launch_route_gather(sub_out, nd->d_sub_pos, n, out, nd->s0));
    int64_t last = 0;
    NHIP(nd, hipMemcpyAsync(&last, &req[n - 1].ts_ms, sizeof(int64_t), hipMemcpyDeviceToHost, nd->s0));
    NHIP(nd, hipStreamSynchronize(nd->s0));
    nd->cp_last_ts = last;
    return SG_OK;
}

int sg_node_cparam_decide_batch_host(sg_node* nd, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                                     uint64_t n_values, sg_result* out) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out || (!values && n_values)) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    NHIP(nd, hipSetDevice(nd->devices[0]));
    node_drain(nd);
    uint64_t* d_vals = nullptr;
    if (!nd->stage.get(2, n_values, d_vals)) return nfail(nd, SG_E_NOMEM, "node host-path values");
    if (n_values) NHIP(nd, hipMemcpy(d_vals, values, 8 * n_values, hipMemcpyHostToDevice));
    return host_batch(nd, nd->devices[0], req, n, out, [&](sg_cparam_req* d_req, sg_result* d_out) {
        return sg_node_cparam_decide_batch(nd, d_req, n, n_values ? d_vals : nullptr, n_values, d_out, nullptr);
    });
}

int sg_node_cparam_read_sum(sg_node* nd, uint32_t rule, uint64_t value, int64_t now_ms, int64_t* sum) {
    if (!nd || !sum || rule >= nd->cp_rules.size()) return SG_E_INVAL;
    node_drain(nd);
    sg_handle* h = nd->shards[nd->cp_shard_of[rule]];
    return node_child(nd, h, sg_cparam_read_sum(h, nd->cp_local_of[rule], value, now_ms, sum));
}

// ClusterParamMetric.getTopValues per node rule (ClusterMetricNodeGenerator.paramToMetricNode :88-104): each rule's
// values come from its owner (its metric lives there), laid out in node rule order as sg_cparam_top_values does.
int sg_node_cparam_top_values(sg_node* nd, int64_t now_ms, uint32_t number, uint64_t* values, double* qps,
                              uint32_t* counts) {
    const uint64_t R = nd ? nd->cp_rules.size() : 0;
    if (!nd || (R && (!values || !qps || !counts))) return SG_E_INVAL;
    node_drain(nd);
    const uint32_t G = (uint32_t)nd->shards.size();
    for (uint32_t g = 0; g < G; ++g) {
        sg_handle* h = nd->shards[g];
        const uint64_t r = h->cprules.size();
        if (!r) continue;
        std::vector<uint64_t> v(r * number);
        std::vector<double> q(r * number);
        std::vector<uint32_t> c(r);
        const int rc = sg_cparam_top_values(h, now_ms, number, v.data(), q.data(), c.data());
        if (rc) return node_child(nd, h, rc);
        for (uint64_t k = 0; k < R; ++k) {
            if (nd->cp_shard_of[k] != g) continue;
            const uint32_t l = nd->cp_local_of[k];
            counts[k] = c[l];
            for (uint32_t j = 0; j < number; ++j) {
                values[k * number + j] = v[(uint64_t)l * number + j];
                qps[k * number + j] = q[(uint64_t)l * number + j];
            }
        }
    }
    return SG_OK;
}

int sg_node_conc_decide_batch(sg_node* nd, const sg_conc_req* req, uint64_t n, sg_conc_result* out, void* stream) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    node_drain(nd);
    int rc = node_nreq_scratch(nd, 1);
    if (rc) return rc;
    const uint32_t G = (uint32_t)nd->shards.size();
    NodeReqArgs q{};
    q.n = n;
    q.cc = req;
    q.K = (uint32_t)nd->shard_of.size();
    q.shard_of = nd->d_shard_of;
    q.local_of = nd->d_local_of;
    q.sub_cc = reinterpret_cast<sg_conc_req*>(nd->d_sub_nreq.get());
    q.last_ts = nd->cc_last_ts;
    NHIP(nd, hipStreamSynchronize((hipStream_t)stream));  // the caller's batch is in place (synchronous call)
    std::vector<uint64_t> base, cnt, vbase, vcnt;
    rc = node_nreq_route(nd, q, base, cnt, vbase, vcnt);
    if (rc) return rc;
    sg_conc_result* sub_out = reinterpret_cast<sg_conc_result*>(nd->d_sub_nout.get());
    rc = node_run_shards(nd, base, cnt, vbase, vcnt, sizeof(sg_conc_req), sizeof(sg_conc_result), q.sub_cc, sub_out,
                         [](uint32_t, sg_handle* h, const void* r, const uint64_t*, uint64_t, uint64_t c, void* o,
                            hipStream_t st) {
                             return sg_conc_decide_batch(h, static_cast<const sg_conc_req*>(r), c,
                                                         static_cast<sg_conc_result*>(o), st);
                         });
    if (rc) return rc;
    NHIP(nd, hipSetDevice(nd->devices[0]));
    for (uint32_t g = 0; g < G; ++g)
        NHIP(nd, launch_nconc_scatter(sub_out, nd->d_sub_pos, q.sub_cc, base[g], cnt[g], g, G, out, nd->s0));
    int64_t last = 0;
    NHIP(nd, hipMemcpyAsync(&last, &req[n - 1].ts_ms, sizeof(int64_t), hipMemcpyDeviceToHost, nd->s0));
    NHIP(nd, hipStreamSynchronize(nd->s0));
    nd->cc_last_ts = last;
    return SG_OK;
}

int sg_node_conc_decide_batch_host(sg_node* nd, const sg_conc_req* req, uint64_t n, sg_conc_result* out) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!req || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    NHIP(nd, hipSetDevice(nd->devices[0]));
    node_drain(nd);
    return host_batch(nd, nd->devices[0], req, n, out, [&](sg_conc_req* d_req, sg_conc_result* d_out) {
        return sg_node_conc_decide_batch(nd, d_req, n, d_out, nullptr);
    });
}

int sg_node_conc_set_rule_timeouts(sg_node* nd, const int64_t* client_offline_ms, const int64_t* resource_timeout_ms,
                                   uint32_t n) {
    if (!nd || (n && (!client_offline_ms || !resource_timeout_ms))) return SG_E_INVAL;
    if (n != nd->shard_of.size()) return nfail(nd, SG_E_INVAL, "one timeout pair per loaded rule");
    node_drain(nd);
    const uint32_t G = (uint32_t)nd->shards.size();
    std::vector<std::vector<int64_t>> off(G), res(G);
    for (uint32_t g = 0; g < G; ++g) {
        off[g].resize(nd->shards[g]->K);
        res[g].resize(nd->shards[g]->K);
    }
    for (uint32_t k = 0; k < n; ++k) {
        off[nd->shard_of[k]][nd->local_of[k]] = client_offline_ms[k];
        res[nd->shard_of[k]][nd->local_of[k]] = resource_timeout_ms[k];
    }
    for (uint32_t g = 0; g < G; ++g) {
        sg_handle* h = nd->shards[g];
        const int rc = sg_conc_set_rule_timeouts(h, off[g].data(), res[g].data(), (uint32_t)off[g].size());
        if (rc) return node_child(nd, h, rc);
    }
    return SG_OK;
}

int sg_node_conc_expire(sg_node* nd, int64_t now_ms, const uint8_t* client_online, uint32_t n_clients, uint64_t* removed) {
    if (!nd || !removed) return SG_E_INVAL;
    node_drain(nd);
    uint64_t total = 0;
    for (sg_handle* h : nd->shards) {
        uint64_t r = 0;
        const int rc = sg_conc_expire(h, now_ms, client_online, n_clients, &r);
        if (rc) return node_child(nd, h, rc);
        total += r;
    }
    *removed = total;
    return SG_OK;
}

int sg_node_conc_read_state(sg_node* nd, uint32_t key, int32_t* now_calls, uint64_t* live_tokens) {
    if (!nd || !now_calls || !live_tokens || key >= nd->shard_of.size()) return SG_E_INVAL;
    node_drain(nd);
    uint64_t live = 0;
    for (uint32_t g = 0; g < (uint32_t)nd->shards.size(); ++g) {
        int32_t nc = 0;
        uint64_t l = 0;
        sg_handle* h = nd->shards[g];
        const bool owner = g == nd->shard_of[key];
        if (!owner && h->K == 0) continue;
        const int rc = sg_conc_read_state(h, owner ? nd->local_of[key] : 0u, &nc, &l);
        if (rc) return node_child(nd, h, rc);
        if (owner) *now_calls = nc;
        live += l;
    }
    *live_tokens = live;
    return SG_OK;
}

}  // extern "C"

// ---- the local slot chain over the node (sg_node_local_*) ----
//
// StatisticSlot → FlowSlot → DegradeSlot (SphU.entry / Entry.exit) for a multi-GPU node from one handle: every shard
// loads the node's whole rule set under the node's resource indices and decides the events of the resources it owns
// (sg_local_owners: a key group lives on one owner), the node routes a batch by owner with a stable multisplit
// (node.hip k_lroute_*), and the node's MetricTimerListener table is the shards' raw rows merged on the device
// (k_merge_*). The front handle carries no local traffic: it is the staging copy of the rules that names the owners.
// The whole chain — AuthoritySlot, and ParamFlowSlot with per-event contexts and arguments (sg_node_slot_decide_batch,
// sg_node_pslot_load_rules) — runs the same way: each event's sg_slot_ext moves with it, and a shard reads the caller's
// argument arrays in place (devices[0]) or its slice's compacted copy (node.hip k_lcmp_*).

namespace {

// a remote shard's slice and results reuse the token batches' per-shard buffers (node_slice_alloc)
static_assert(sizeof(sg_local_event) <= std::max(sizeof(sg_cparam_req), sizeof(sg_conc_req)), "slice buffer");
static_assert(sizeof(sg_local_result) <= std::max(sizeof(sg_result), sizeof(sg_conc_result)), "result buffer");

// The owners the front's loaded rules give (sg_local_owners over the node's G shards).
int node_local_owners(sg_node* nd, std::vector<uint32_t>& own) {
    own.assign(nd->front->ltab.size(), 0);
    const int rc = sg_local_owners(nd->front, (uint32_t)nd->shards.size(), own.data(), (uint32_t)own.size());
    return rc ? node_child(nd, nd->front, rc) : SG_OK;
}

int node_local_set_owners(sg_node* nd, const std::vector<uint32_t>& own) {
    NHIP(nd, hipSetDevice(nd->devices[0]));
    nd->d_l_owner.reset();
    const std::vector<uint8_t> o8(own.begin(), own.end());
    if (!nd->d_l_owner.alloc_bytes(o8.size() ? o8.size() : 1)) return nfail(nd, SG_E_NOMEM, "owner table");
    if (!o8.empty()) NHIP(nd, hipMemcpy(nd->d_l_owner, o8.data(), o8.size(), hipMemcpyHostToDevice));
    nd->l_owner = own;
    return SG_OK;
}

// The handle without param rules, as before its first sg_pslot_load_rules (one handle has no call for this: its
// sg_local_load_rules keeps the param rules; the node's clears them, since the owners of their state may move). The
// next batch takes the param flags off the rule image (local_apply_params).
void pslot_unload(sg_handle* h) {
    if (!h->ps_loaded) return;
    drain_async(h);
    h->ps_loaded = false;
    if (h->ps_cluster) h->l_groups_stale = true;  // the slot chain's key groups included the cluster-mode param rules
    h->ps_cluster = false;
    h->ps_cluster_refs.clear();
    h->ps_res_rules.clear();
    h->ps_groups_stale = true;
    if (h->l_ps_applied == 0) h->l_has_cx_ps = false;
}

// The front back on the rules in force (it holds no statistics: a fresh load of every rule set).
void node_local_front_rollback(sg_node* nd) {
    sg_handle* f = nd->front;
    if (sg_local_load_rules(f, &nd->l_cfg, nd->l_rules.data(), (uint32_t)nd->l_rules.size()) != SG_OK) return;
    if (nd->l_has_frules)
        (void)sg_local_load_flow_rules(f, nd->l_frules.data(), (uint32_t)nd->l_frules.size(), nd->l_n_origins,
                                       nd->l_n_contexts);
    (void)sg_local_load_authority_rules(f, nd->l_arules.data(), (uint32_t)nd->l_arules.size(), nd->l_aorigins.data(),
                                        (uint32_t)nd->l_aorigins.size(), nd->l_n_origins);
    if (nd->l_ps_loaded)
        (void)sg_pslot_load_rules(f, nd->l_prules.data(), (uint32_t)nd->l_prules.size(),
                                  nd->l_phot.empty() ? nullptr : nd->l_phot.data(), (uint32_t)nd->l_phot.size(),
                                  (uint32_t)nd->l_rules.size());
    else
        pslot_unload(f);
}

// k_merge_* over `n` raw rows on devices[0] into d_out (device); *n_out rows. Waits for the result.
int node_merge_rows(sg_node* nd, const sg_metric_node* d_rows, uint64_t n, sg_metric_node* d_out, uint64_t cap,
                    uint64_t* n_out, hipStream_t stream) {
    *n_out = 0;
    MergeArgs m{};
    m.rows = d_rows;
    m.n = n;
    m.K = (uint32_t)nd->l_rules.size();
    m.W = nd->m_words;
    m.bits = nd->d_mbits;
    m.pre = nd->d_mpre;
    m.st = nd->d_mslots;
    m.out = d_out;
    m.cap = cap;
    NHIP(nd, launch_merge_rows(m, stream));
    unsigned long long total = 0;
    int err = 0;
    NHIP(nd, hipMemcpyAsync(&total, &nd->d_mslots.get()->n_out, sizeof(total), hipMemcpyDeviceToHost, stream));
    NHIP(nd, hipMemcpyAsync(&err, &nd->d_mslots.get()->err, sizeof(err), hipMemcpyDeviceToHost, stream));
    NHIP(nd, hipStreamSynchronize(stream));
    if (err & kMergeBad)
        return nfail(nd, SG_E_INVAL, "metric rows outside the merge's contract: timestamps multiples of 1000 within one "
                                     "minute, one row per (timestamp, resource), resources below the resource count");
    *n_out = total;
    if (err & kMergeCap) return nfail(nd, SG_E_CAPACITY, "merged metric table larger than the buffer (*n_out rows)");
    return SG_OK;
}

// MetricTimerListener.run for the node: the shards' row counts, their raw rows one after the other on devices[0],
// the merge into d_out (device) or, with h_out, into the node's own table copied out.
int node_local_metrics(sg_node* nd, int64_t now_ms, sg_metric_node* d_out, sg_metric_node* h_out, uint64_t cap,
                       uint64_t* n_rows) {
    if (!nd || !n_rows || (!d_out && !h_out && cap)) return SG_E_INVAL;
    *n_rows = 0;
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    node_drain(nd);
    const uint32_t G = (uint32_t)nd->shards.size();
    // 1. every shard's count (a capacity of 0 rows: the count alone, no side effect)
    for (uint32_t g = 0; g < G; ++g) {
        sg_handle* h = nd->shards[g];
        NHIP(nd, hipSetDevice(nd->devices[g]));
        if (!nd->sh[g].r_mcnt && !nd->sh[g].r_mcnt.alloc_bytes(sizeof(uint64_t)))
            return nfail(nd, SG_E_NOMEM, "metric row counter");
        const int rc = sg_local_metrics_raw_enqueue(h, now_ms, nullptr, 0, nd->sh[g].r_mcnt, nd->sh[g].stream);
        if (rc) {
            node_sync_shards(nd, g);
            return node_child(nd, h, rc);
        }
    }
    std::vector<uint64_t> cnt(G, 0);
    uint64_t sum = 0;
    for (uint32_t g = 0; g < G; ++g) {
        NHIP(nd, hipSetDevice(nd->devices[g]));
        NHIP(nd, hipMemcpyAsync(&cnt[g], nd->sh[g].r_mcnt, sizeof(uint64_t), hipMemcpyDeviceToHost, nd->sh[g].stream));
        NHIP(nd, hipStreamSynchronize(nd->sh[g].stream));
        sum += cnt[g];
    }
    NHIP(nd, hipSetDevice(nd->devices[0]));
    *n_rows = sum;  // a sufficient capacity: the merged table can only be shorter (ENTRY_NODE rows of a second collapse)
    if (sum > cap) return nfail(nd, SG_E_CAPACITY, "metric row buffer too small (*n_rows rows suffice)");
    if (sum == 0) return SG_OK;
    if (!nd->d_mrows.reserve(sum)) return nfail(nd, SG_E_NOMEM, "node metric rows");
    if (h_out && !nd->d_mout.reserve(sum)) return nfail(nd, SG_E_NOMEM, "node metric table");
    // 2. every shard's rows (its listener state advances), a remote shard's through a buffer on its device
    std::vector<uint64_t> off(G, 0);
    uint64_t at = 0;
    for (uint32_t g = 0; g < G; ++g) {
        off[g] = at;
        at += cnt[g];
        if (!cnt[g]) continue;
        sg_handle* h = nd->shards[g];
        const bool remote = nd->devices[g] != nd->devices[0];
        NHIP(nd, hipSetDevice(nd->devices[g]));
        if (remote && !nd->sh[g].r_mrows.reserve(cnt[g])) {
            node_sync_shards(nd, g);
            return nfail(nd, SG_E_NOMEM, "shard metric rows");
        }
        sg_metric_node* dst = remote ? nd->sh[g].r_mrows : nd->d_mrows + off[g];
        const int rc = sg_local_metrics_raw_enqueue(h, now_ms, dst, cnt[g], nd->sh[g].r_mcnt, nd->sh[g].stream);
        if (rc) {
            node_sync_shards(nd, g);
            return node_child(nd, h, rc);
        }
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (!cnt[g]) continue;
        NHIP(nd, hipSetDevice(nd->devices[g]));
        NHIP(nd, hipStreamSynchronize(nd->sh[g].stream));
        if (nd->devices[g] != nd->devices[0])
            NHIP(nd, hipMemcpyPeer(nd->d_mrows + off[g], nd->devices[0], nd->sh[g].r_mrows, nd->devices[g],
                                   sizeof(sg_metric_node) * cnt[g]));
    }
    // 3. the merge
    NHIP(nd, hipSetDevice(nd->devices[0]));
    uint64_t rows = 0;
    const int rc = node_merge_rows(nd, nd->d_mrows, sum, h_out ? nd->d_mout : d_out, h_out ? sum : cap, &rows, nd->s0);
    if (rc) return rc;
    if (h_out && rows) NHIP(nd, hipMemcpy(h_out, nd->d_mout, sizeof(sg_metric_node) * rows, hipMemcpyDeviceToHost));
    *n_rows = rows;
    return SG_OK;
}

// sg_slot_decide_batch over the node (ext nullable: sg_node_local_decide_batch). Device pointers on devices[0].
int node_slot_decide(sg_node* nd, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n, const sg_pslot_arg* args,
                     uint64_t n_args, const uint64_t* values, uint64_t n_values, sg_local_result* out, void* stream) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!ev || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    if (!args) n_args = 0;
    if (!values) n_values = 0;
    if (n_args >= (1ull << 32) || n_values >= (1ull << 32))
        return nfail(nd, SG_E_CAPACITY, "more than 2^32 argument records or values");
    node_drain(nd);
    NHIP(nd, hipSetDevice(nd->devices[0]));
    const uint32_t G = (uint32_t)nd->shards.size();
    if (!nd->d_lsub_ev && (!nd->d_lsub_ev.alloc_bytes(sizeof(sg_local_event) * nd->cfg.max_batch) ||
                           !nd->d_lsub_out.alloc_bytes(sizeof(sg_local_result) * nd->cfg.max_batch)))
        return nfail(nd, SG_E_NOMEM, "node local slices");
    if (ext && !nd->d_lsub_ext && !nd->d_lsub_ext.alloc(nd->cfg.max_batch))
        return nfail(nd, SG_E_NOMEM, "node ext slices");
    NHIP(nd, hipStreamSynchronize((hipStream_t)stream));  // the caller's batch is in place (synchronous call)
    // 1. the batch validated as a whole and split by owner: a refused batch reaches no shard
    const bool with_args = ext && nd->l_ps_loaded;  // one handle reads the arguments only with param rules loaded
    LRouteArgs r{};
    r.ev = ev;
    r.n = n;
    r.K = (uint32_t)nd->l_rules.size();
    r.owner = nd->d_l_owner;
    r.G = (int)G;
    r.tile_cnt = nd->d_tile_cnt;
    r.shard_base = nd->d_base;
    r.shard_tot = nd->d_base + kMaxShards + 1;
    r.sub_ev = nd->d_lsub_ev;
    r.sub_pos = nd->d_sub_pos;
    r.err = nd->d_lerr;
    r.last_ts = nd->l_last_ts;
    r.n_origins = nd->l_n_origins;
    r.n_wl = std::min(nd->front->l_n_wl, 2);
    for (int w = 0; w < r.n_wl; ++w) r.wl[w] = nd->front->l_wl[w];
    r.ext = ext;
    r.sub_ext = nd->d_lsub_ext;
    r.n_contexts = nd->l_n_contexts;
    r.has_ps = with_args ? 1 : 0;
    r.args = args;
    r.n_args = n_args;
    r.n_values = n_values;
    NHIP(nd, hipMemsetAsync(nd->d_lerr, 0, sizeof(int), nd->s0));
    NHIP(nd, launch_lroute(r, nd->s0));
    int64_t last = 0;
    NHIP(nd, hipMemcpyAsync(nd->h_base, nd->d_base, sizeof(uint32_t) * (2 * kMaxShards + 1), hipMemcpyDeviceToHost, nd->s0));
    NHIP(nd, hipMemcpyAsync(nd->h_front_err, nd->d_lerr, sizeof(int), hipMemcpyDeviceToHost, nd->s0));
    NHIP(nd, hipMemcpyAsync(&last, &ev[n - 1].ts_ms, sizeof(int64_t), hipMemcpyDeviceToHost, nd->s0));
    NHIP(nd, hipStreamSynchronize(nd->s0));
    const int err = *nd->h_front_err;
    if (err & kErrTime)
        return nfail(nd, SG_E_TIME, "timestamps must be >= 0, non-decreasing, and not older than the node's earlier batches");
    if (err & kErrPeriods) return nfail(nd, SG_E_UNSUPPORTED, "batch spans more than 65536 window periods");
    if (err & kErrBounds) return nfail(nd, SG_E_INVAL, "an event's origin id lies outside 0..n_origins");
    if (err & kErrExt)
        return nfail(nd, SG_E_INVAL, "an event's context lies outside 0..n_contexts - 1, or its arguments outside the "
                                     "arg / value arrays");
    std::vector<uint64_t> base(G), cnt(G), zero(G, 0);
    for (uint32_t g = 0; g < G; ++g) {
        base[g] = nd->h_base[g];
        cnt[g] = nd->h_base[kMaxShards + 1 + g];
    }
    // 2. the arguments of the shards that cannot read the caller's arrays (off devices[0]; all under the test aid):
    // their slices' own arrays, counted, refused or allocated before any shard runs, then gathered
    std::vector<char> compact(G, 0);
    std::vector<uint64_t> na(G, 0), nv(G, 0);
    if (ext) {
        bool any = false;
        std::vector<LCompactArgs> ca(G);
        uint64_t tile0 = 0;
        for (uint32_t g = 0; g < G; ++g) {
            compact[g] = cnt[g] && (nd->compact_args || nd->devices[g] != nd->devices[0]);
            if (!compact[g] || !with_args) continue;
            if (!any) {
                const uint64_t words = 2 * (lcompact_tiles(nd->cfg.max_batch) + kMaxShards);
                if (!nd->d_ctsum && (!nd->d_ctsum.alloc(words) || !nd->d_ctot.alloc(2 * kMaxShards)))
                    return nfail(nd, SG_E_NOMEM, "argument compaction scratch");
                any = true;
            }
            LCompactArgs& c = ca[g];
            c.ev = nd->d_lsub_ev + base[g];
            c.ext = nd->d_lsub_ext + base[g];
            c.n = cnt[g];
            c.K = r.K;
            c.args = args;
            c.values = values;
            c.tsum = nd->d_ctsum + 2 * tile0;
            c.tot = nd->d_ctot + 2 * g;
            tile0 += lcompact_tiles(cnt[g]);
            NHIP(nd, launch_lcompact_count(c, nd->s0));
        }
        if (any) {
            unsigned long long tot[2 * kMaxShards];
            NHIP(nd, hipMemcpyAsync(tot, nd->d_ctot, sizeof(tot), hipMemcpyDeviceToHost, nd->s0));
            NHIP(nd, hipStreamSynchronize(nd->s0));
            for (uint32_t g = 0; g < G; ++g) {
                if (!compact[g]) continue;
                na[g] = tot[2 * g];
                nv[g] = tot[2 * g + 1];
                if (na[g] >= (1ull << 32) || nv[g] >= (1ull << 32))
                    return nfail(nd, SG_E_CAPACITY, "a shard's slice carries more than 2^32 argument records or values");
            }
            for (uint32_t g = 0; g < G; ++g) {
                if (!compact[g]) continue;
                if (!nd->d_cargs[g].reserve(na[g] ? na[g] : 1) || !nd->d_cvals[g].reserve(nv[g] ? nv[g] : 1))
                    return nfail(nd, SG_E_NOMEM, "a shard's compacted arguments");
                ca[g].out_args = nd->d_cargs[g];
                ca[g].out_vals = nd->d_cvals[g];
                NHIP(nd, launch_lcompact_gather(ca[g], nd->s0));
            }
            NHIP(nd, hipStreamSynchronize(nd->s0));
        }
        // a remote shard's ext records, arg records and values on its own device
        for (uint32_t g = 0; g < G; ++g) {
            if (!cnt[g] || nd->devices[g] == nd->devices[0]) continue;
            sg_node::Shard& s = nd->sh[g];
            NHIP(nd, hipSetDevice(nd->devices[g]));
            if (!s.r_ext.reserve(cnt[g]) || !s.r_args.reserve(na[g] ? na[g] : 1) || !s.r_vals.reserve(nv[g] ? nv[g] : 1)) {
                (void)hipSetDevice(nd->devices[0]);
                return nfail(nd, SG_E_NOMEM, "shard argument buffers");
            }
        }
        NHIP(nd, hipSetDevice(nd->devices[0]));
    }
    // 3. every shard with work decides its slice (its own host thread and stream; peer copies off devices[0])
    const int d0 = nd->devices[0];
    int rc = node_run_shards(
        nd, base, cnt, zero, zero, sizeof(sg_local_event), sizeof(sg_local_result), nd->d_lsub_ev, nd->d_lsub_out,
        [&](uint32_t g, sg_handle* h, const void* e, const uint64_t*, uint64_t, uint64_t c, void* o, hipStream_t st) {
            const sg_local_event* sev = static_cast<const sg_local_event*>(e);
            sg_local_result* so = static_cast<sg_local_result*>(o);
            if (!ext) return sg_local_decide_batch(h, sev, c, so, st);
            const sg_slot_ext* sx = nd->d_lsub_ext + base[g];
            const sg_pslot_arg* sa = args;  // in place: the caller's arrays, no index changes
            const uint64_t* sv = values;
            uint64_t sna = n_args, snv = n_values;
            if (compact[g]) {
                sa = with_args ? nd->d_cargs[g].get() : nullptr;
                sv = with_args ? nd->d_cvals[g].get() : nullptr;
                sna = na[g];
                snv = nv[g];
            }
            if (h->device != d0) {  // the slice's records go with it
                sg_node::Shard& s = nd->sh[g];
                hipError_t pe = hipMemcpyPeer(s.r_ext, h->device, sx, d0, sizeof(sg_slot_ext) * c);
                if (pe == hipSuccess && sna) pe = hipMemcpyPeer(s.r_args, h->device, sa, d0, sizeof(sg_pslot_arg) * sna);
                if (pe == hipSuccess && snv) pe = hipMemcpyPeer(s.r_vals, h->device, sv, d0, sizeof(uint64_t) * snv);
                if (pe != hipSuccess) return fail(h, SG_E_DEVICE, hipGetErrorString(pe));
                sx = s.r_ext;
                sa = sna ? s.r_args.get() : nullptr;
                sv = snv ? s.r_vals.get() : nullptr;
            }
            return sg_slot_decide_batch(h, sev, sx, c, sa, sna, sv, snv, so, st);
        });
    if (rc) return rc;
    // 4. the results back in caller order
    NHIP(nd, hipSetDevice(nd->devices[0]));
    NHIP(nd, launch_route_gather8(nd->d_lsub_out, nd->d_sub_pos, n, out, nd->s0));
    NHIP(nd, hipStreamSynchronize(nd->s0));
    nd->l_last_ts = last;
    ++nd->l_batches;
    return SG_OK;
}

// The owner shard's handle of a resource / of a param rule's resource (null: no such index).
sg_handle* node_local_owner(sg_node* nd, uint32_t res) {
    return nd->l_loaded && res < nd->l_owner.size() ? nd->shards[nd->l_owner[res]] : nullptr;
}

sg_handle* node_prule_owner(sg_node* nd, uint32_t rule) {
    return nd->l_ps_loaded && rule < nd->l_prules.size() ? node_local_owner(nd, nd->l_prules[rule].resource) : nullptr;
}

}  // namespace

extern "C" {

int sg_node_local_load_rules(sg_node* nd, const sg_local_config* cfg, const sg_local_rule* rules, uint32_t n) {
    if (!nd || !cfg || (!rules && n)) return SG_E_INVAL;
    node_drain(nd);
    const uint32_t G = (uint32_t)nd->shards.size();
    // the front first (validation; the staging copy that names the owners), then every shard: fresh statistics, so
    // the owners may change freely. A shard that fails leaves the node's local chain unloaded (load again).
    int rc = sg_local_load_rules(nd->front, cfg, rules, n);
    if (rc) return node_child(nd, nd->front, rc);
    nd->l_loaded = false;
    nd->l_cfg = *cfg;
    nd->l_rules.assign(rules, rules + n);
    nd->l_frules.clear();
    nd->l_has_frules = false;
    nd->l_arules.clear();
    nd->l_aorigins.clear();
    nd->l_n_origins = nd->l_n_contexts = 0;
    nd->l_last_ts = -1;
    nd->l_batches = 0;
    // the owners may move, and a param rule's state lives on its resource's owner: the node's param rules go too
    // (one handle keeps them over sg_local_load_rules; load them again with sg_node_pslot_load_rules)
    nd->l_ps_loaded = false;
    nd->l_prules.clear();
    nd->l_phot.clear();
    pslot_unload(nd->front);
    std::vector<uint32_t> own;
    rc = node_local_owners(nd, own);
    if (rc) return rc;
    for (uint32_t g = 0; g < G; ++g) {
        rc = sg_local_load_rules(nd->shards[g], cfg, rules, n);
        if (rc) return node_child(nd, nd->shards[g], rc);
        pslot_unload(nd->shards[g]);
    }
    rc = node_local_set_owners(nd, own);
    if (rc) return rc;
    // the merge's scratch: (second, resource) bitmap and its prefix counts, the slots' sums
    const uint32_t W = (n + 63) / 64;
    if (W > nd->m_words || !nd->d_mbits) {
        nd->d_mbits.reset();
        nd->d_mpre.reset();
        nd->m_words = 0;
        const size_t words = (size_t)kMinuteS * (W ? W : 1);
        if (!nd->d_mbits.alloc_bytes(sizeof(unsigned long long) * words) ||
            !nd->d_mpre.alloc_bytes(sizeof(uint32_t) * words))
            return nfail(nd, SG_E_NOMEM, "metric merge scratch");
    }
    nd->m_words = W;
    if (!nd->d_mslots && !nd->d_mslots.alloc_bytes(sizeof(MergeSlots)))
        return nfail(nd, SG_E_NOMEM, "metric merge scratch");
    if (!nd->d_lerr && !nd->d_lerr.alloc_bytes(sizeof(int))) return nfail(nd, SG_E_NOMEM, "error word");
    nd->l_loaded = true;
    return SG_OK;
}

int sg_node_local_load_flow_rules(sg_node* nd, const sg_local_flow_rule* rules, uint32_t n, int32_t n_origins,
                                  int32_t n_contexts) {
    if (!nd || (!rules && n)) return SG_E_INVAL;
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    node_drain(nd);
    // what a shard that has decided a batch refuses, a shard that has not would accept: the node's batches decide
    if (n_contexts > 0 && nd->l_n_contexts == 0 && nd->l_batches > 0)
        return nfail(nd, SG_E_UNSUPPORTED, "context tracking (n_contexts >= 1) starts before the node's first local batch");
    // the front first: validation, and the owners the new key groups give. The resources keep their statistics, so
    // after a batch none may move: checked here, before any shard is touched.
    const int kept = sg_local_load_flow_rules(nd->front, rules, n, n_origins, n_contexts);
    if (kept < 0) return node_child(nd, nd->front, kept);
    std::vector<uint32_t> own;
    int rc = node_local_owners(nd, own);
    if (rc) {
        node_local_front_rollback(nd);
        return rc;
    }
    if (nd->l_batches > 0 && own != nd->l_owner) {
        node_local_front_rollback(nd);
        return nfail(nd, SG_E_UNSUPPORTED, "the new rules' key groups move a resource to another shard after the node "
                                           "decided a local batch (its statistics live on its owner)");
    }
    for (sg_handle* h : nd->shards) {
        rc = sg_local_load_flow_rules(h, rules, n, n_origins, n_contexts);
        if (rc < 0) return node_child(nd, h, rc);
    }
    rc = node_local_set_owners(nd, own);
    if (rc) return rc;
    nd->l_frules.assign(rules, rules + n);
    nd->l_has_frules = true;
    nd->l_n_origins = n_origins;
    nd->l_n_contexts = n_contexts;
    return kept;
}

int sg_node_local_load_authority_rules(sg_node* nd, const sg_authority_rule* rules, uint32_t n, const int32_t* origins,
                                       uint32_t n_origin_ids, int32_t n_origins) {
    if (!nd || (!rules && n) || (!origins && n_origin_ids)) return SG_E_INVAL;
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    node_drain(nd);
    // the front first (validation: a refused load reaches no shard), then every shard. Authority rules form no key
    // groups, so no resource changes its owner.
    const int kept = sg_local_load_authority_rules(nd->front, rules, n, origins, n_origin_ids, n_origins);
    if (kept < 0) return node_child(nd, nd->front, kept);
    for (sg_handle* h : nd->shards) {
        const int rc = sg_local_load_authority_rules(h, rules, n, origins, n_origin_ids, n_origins);
        if (rc < 0) return node_child(nd, h, rc);
    }
    nd->l_arules.assign(rules, rules + n);
    nd->l_aorigins.assign(origins, origins + n_origin_ids);
    if (n_origins > nd->l_n_origins) nd->l_n_origins = n_origins;
    return kept;
}

int sg_node_local_set_entry_types(sg_node* nd, const uint8_t* inbound, uint32_t n) {
    if (!nd || (!inbound && n)) return SG_E_INVAL;
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    node_drain(nd);
    int rc = sg_local_set_entry_types(nd->front, inbound, n);
    if (rc) return node_child(nd, nd->front, rc);
    for (sg_handle* h : nd->shards) {
        rc = sg_local_set_entry_types(h, inbound, n);
        if (rc) return node_child(nd, h, rc);
    }
    NHIP(nd, hipSetDevice(nd->devices[0]));
    return SG_OK;
}

int sg_node_local_owner_of(const sg_node* nd, uint32_t resource, uint32_t* shard) {
    if (!nd || !shard || !nd->l_loaded || resource >= nd->l_owner.size()) return SG_E_INVAL;
    *shard = nd->l_owner[resource];
    return SG_OK;
}

int sg_node_local_decide_batch(sg_node* nd, const sg_local_event* ev, uint64_t n, sg_local_result* out, void* stream) {
    return node_slot_decide(nd, ev, nullptr, n, nullptr, 0, nullptr, 0, out, stream);
}

int sg_node_local_decide_batch_host(sg_node* nd, const sg_local_event* ev, uint64_t n, sg_local_result* out) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!ev || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    NHIP(nd, hipSetDevice(nd->devices[0]));
    node_drain(nd);
    return host_batch(nd, nd->devices[0], ev, n, out, [&](sg_local_event* d_ev, sg_local_result* d_out) {
        return sg_node_local_decide_batch(nd, d_ev, n, d_out, nullptr);
    });
}

int sg_node_local_read_state(sg_node* nd, uint32_t res, int64_t* second, int64_t* borrow, int64_t* minute, int64_t* head) {
    if (!nd) return SG_E_INVAL;
    if (!nd->l_loaded || res >= nd->l_owner.size()) return nfail(nd, SG_E_INVAL, "no such resource");
    node_drain(nd);
    sg_handle* h = nd->shards[nd->l_owner[res]];
    const int rc = node_child(nd, h, sg_local_read_state(h, res, second, borrow, minute, head));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_pslot_load_rules(sg_node* nd, const sg_pslot_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                             uint32_t n_hot, uint32_t n_resources) {
    if (!nd || (!rules && n) || (!hot && n_hot)) return SG_E_INVAL;
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    if (n_resources != nd->l_rules.size()) return nfail(nd, SG_E_INVAL, "n_resources differs from the node's resource count");
    node_drain(nd);
    // the front first (validation: a refused load reaches no shard, and the front goes back to the rules in force),
    // then every shard: the whole rule set under the node's rule and resource indices. Param rules form no key
    // groups here (the shards are in SG_CLUSTER_NOT_STARTED), so no resource changes its owner; a rule's state —
    // token buckets, throttle times, thread counts, a resolved negative paramIdx — lives on its resource's owner.
    int rc = sg_pslot_load_rules(nd->front, rules, n, hot, n_hot, n_resources);
    if (rc) {
        nd->err = nd->front->err;
        node_local_front_rollback(nd);
        (void)hipSetDevice(nd->devices[0]);
        return rc;
    }
    for (sg_handle* h : nd->shards) {
        rc = sg_pslot_load_rules(h, rules, n, hot, n_hot, n_resources);
        if (rc) {
            node_child(nd, h, rc);
            (void)hipSetDevice(nd->devices[0]);
            return rc;
        }
    }
    nd->l_prules.assign(rules, rules + n);
    nd->l_phot.assign(hot, hot + n_hot);
    nd->l_ps_loaded = true;
    NHIP(nd, hipSetDevice(nd->devices[0]));
    return SG_OK;
}

int sg_node_slot_decide_batch(sg_node* nd, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                              const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                              sg_local_result* out, void* stream) {
    return node_slot_decide(nd, ev, ext, n, args, n_args, values, n_values, out, stream);
}

int sg_node_slot_decide_batch_host(sg_node* nd, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                                   const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                                   sg_local_result* out) {
    if (!nd) return SG_E_INVAL;
    if (n == 0) return SG_OK;
    if (!ev || !out) return nfail(nd, SG_E_INVAL, "null buffer");
    if (n > nd->cfg.max_batch) return nfail(nd, SG_E_CAPACITY, "batch larger than max_batch");
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    if (!args) n_args = 0;
    if (!values) n_values = 0;
    if (n_args >= (1ull << 32) || n_values >= (1ull << 32))
        return nfail(nd, SG_E_CAPACITY, "more than 2^32 argument records or values");
    NHIP(nd, hipSetDevice(nd->devices[0]));
    node_drain(nd);
    // the events and the results through host_batch (slots 0, 1); ext and the arguments in slots 2, 3; the values,
    // of any length, in a buffer of this call (as sg_slot_decide_batch_host)
    sg_slot_ext* d_ext = nullptr;
    sg_pslot_arg* d_args = nullptr;
    DevBuf<uint64_t> d_vals;
    if ((ext && !nd->stage.get(2, nd->cfg.max_batch, d_ext)) || (n_args && !nd->stage.get(3, n_args, d_args)) ||
        (n_values && !d_vals.alloc(n_values)))
        return nfail(nd, SG_E_NOMEM, "host-path buffers");
    if (ext) NHIP(nd, hipMemcpy(d_ext, ext, sizeof(sg_slot_ext) * n, hipMemcpyHostToDevice));
    if (n_args) NHIP(nd, hipMemcpy(d_args, args, sizeof(sg_pslot_arg) * n_args, hipMemcpyHostToDevice));
    if (n_values) NHIP(nd, hipMemcpy(d_vals, values, sizeof(uint64_t) * n_values, hipMemcpyHostToDevice));
    return host_batch(nd, nd->devices[0], ev, n, out, [&](sg_local_event* d_ev, sg_local_result* d_out) {
        return node_slot_decide(nd, d_ev, d_ext, n, d_args, n_args, d_vals, n_values, d_out, nullptr);
    });
}

int sg_node_local_read_origin_state(sg_node* nd, uint32_t res, int32_t origin, int64_t* second, int64_t* borrow,
                                    int64_t* minute, int64_t* head) {
    if (!nd) return SG_E_INVAL;
    sg_handle* h = node_local_owner(nd, res);
    if (!h) return nfail(nd, SG_E_INVAL, "no such resource");
    node_drain(nd);
    const int rc = node_child(nd, h, sg_local_read_origin_state(h, res, origin, second, borrow, minute, head));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_local_read_context_state(sg_node* nd, uint32_t res, int32_t context, int64_t* second, int64_t* borrow,
                                     int64_t* minute, int64_t* head) {
    if (!nd) return SG_E_INVAL;
    sg_handle* h = node_local_owner(nd, res);
    if (!h) return nfail(nd, SG_E_INVAL, "no such resource");
    node_drain(nd);
    const int rc = node_child(nd, h, sg_local_read_context_state(h, res, context, second, borrow, minute, head));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_local_read_controller(sg_node* nd, uint32_t rule, int64_t* state3) {
    if (!nd) return SG_E_INVAL;
    if (!nd->l_loaded || !nd->l_has_frules || rule >= nd->l_frules.size())
        return nfail(nd, SG_E_INVAL, "no such flow rule");
    sg_handle* h = node_local_owner(nd, nd->l_frules[rule].resource);
    if (!h) h = nd->shards[0];  // a rule of no resource of the node: any shard answers it as one handle does
    node_drain(nd);
    const int rc = node_child(nd, h, sg_local_read_controller(h, rule, state3));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_pslot_thread_count(sg_node* nd, uint32_t resource, int32_t param_idx, uint64_t value, int64_t* count) {
    if (!nd) return SG_E_INVAL;
    sg_handle* h = nd->l_ps_loaded ? node_local_owner(nd, resource) : nullptr;
    if (!h) return nfail(nd, SG_E_INVAL, "no such resource (or no param rules on the node)");
    node_drain(nd);
    const int rc = node_child(nd, h, sg_pslot_thread_count(h, resource, param_idx, value, count));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_pslot_param_idx(sg_node* nd, uint32_t rule, int32_t* param_idx) {
    if (!nd) return SG_E_INVAL;
    sg_handle* h = node_prule_owner(nd, rule);
    if (!h) return nfail(nd, SG_E_INVAL, "no such param rule");
    node_drain(nd);
    const int rc = node_child(nd, h, sg_pslot_param_idx(h, rule, param_idx));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_param_read_state(sg_node* nd, uint32_t rule, uint64_t value, int64_t* last_time, int64_t* tokens) {
    if (!nd) return SG_E_INVAL;
    sg_handle* h = node_prule_owner(nd, rule);
    if (!h) return nfail(nd, SG_E_INVAL, "no such param rule");
    node_drain(nd);
    const int rc = node_child(nd, h, sg_param_read_state(h, rule, value, last_time, tokens));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_local_metrics(sg_node* nd, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows) {
    return node_local_metrics(nd, now_ms, nullptr, out, cap, n_rows);
}

int sg_node_local_metrics_device(sg_node* nd, int64_t now_ms, sg_metric_node* d_out, uint64_t cap, uint64_t* n_rows) {
    return node_local_metrics(nd, now_ms, d_out, nullptr, cap, n_rows);
}

int sg_node_local_merge_rows(sg_node* nd, const sg_metric_node* d_rows, uint64_t n, sg_metric_node* d_out, uint64_t cap,
                             uint64_t* n_out, void* stream) {
    if (!nd || !n_out || (!d_rows && n) || (!d_out && cap)) return SG_E_INVAL;
    *n_out = 0;
    if (!nd->l_loaded) return nfail(nd, SG_E_INVAL, "sg_node_local_load_rules first");
    node_drain(nd);
    NHIP(nd, hipSetDevice(nd->devices[0]));
    return node_merge_rows(nd, d_rows, n, d_out, cap, n_out, (hipStream_t)stream);
}

// The front and every shard hold the whole param rule set under the node's rule indices (sg_node_pslot_load_rules),
// so all of them grow: the front first (it refuses what any shard would, before one has changed), then the shards in
// order. Each handle's growth is all or nothing; the node's is not — a shard that fails (SG_E_NOMEM) leaves the front
// and the shards before it grown, which decides nothing differently (a table's size is invisible) and is completed by
// calling again: sizes already reached are kept.
int sg_node_param_resize(sg_node* nd, const int32_t* capacity_log2, uint32_t n) {
    if (!nd) return SG_E_INVAL;
    if (!nd->l_ps_loaded) return nfail(nd, SG_E_INVAL, "sg_node_pslot_load_rules first");
    node_drain(nd);
    int rc = node_child(nd, nd->front, sg_param_resize(nd->front, capacity_log2, n));
    for (size_t g = 0; !rc && g < nd->shards.size(); ++g)
        rc = node_child(nd, nd->shards[g], sg_param_resize(nd->shards[g], capacity_log2, n));
    for (uint32_t i = 0; !rc && i < n; ++i)  // what a front rollback loads again (node_local_front_rollback)
        if (capacity_log2[i]) nd->l_prules[i].rule.capacity_log2 = capacity_log2[i];
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

int sg_node_param_table_used(sg_node* nd, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity) {
    if (!nd) return SG_E_INVAL;
    sg_handle* h = node_prule_owner(nd, rule);
    if (!h) return nfail(nd, SG_E_INVAL, "no such param rule");
    node_drain(nd);
    const int rc = node_child(nd, h, sg_param_table_used(h, rule, used, live, capacity));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

// Every shard that owns cluster param rules grows its tables, in shard order; the first refusal is returned with the
// shards before it grown (as sg_node_cparam_load_rules: not node-wide all or nothing; call again to complete).
int sg_node_cparam_resize(sg_node* nd, int32_t capacity_log2) {
    if (!nd) return SG_E_INVAL;
    if (nd->cp_rules.empty()) return nfail(nd, SG_E_INVAL, "no cluster param rules loaded");
    node_drain(nd);
    int rc = SG_OK;
    for (size_t g = 0; !rc && g < nd->shards.size(); ++g) {
        sg_handle* h = nd->shards[g];
        if (h->cptab.empty()) continue;  // owns no flowId
        rc = node_child(nd, h, sg_cparam_resize(h, capacity_log2));
    }
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

namespace {
void sweep_stats_add(sg_sweep_stats& sum, const sg_sweep_stats& s) {
    sum.values_removed += s.values_removed;
    sum.claims_dropped += s.claims_dropped;
    sum.threads_removed += s.threads_removed;
    sum.values_kept += s.values_kept;
}
}  // namespace

// As sg_node_param_resize: the front first (it refuses what any shard would, before one has changed), then the shards
// in order; a swept entry is invisible, so a shard that fails leaves nothing to undo — call again to complete. The
// node's own time order comes first: a node batch validates against l_last_ts before any shard sees it.
int sg_node_param_sweep(sg_node* nd, int64_t now_ms, sg_sweep_stats* out) {
    if (!nd) return SG_E_INVAL;
    if (!nd->l_ps_loaded) return nfail(nd, SG_E_INVAL, "sg_node_pslot_load_rules first");
    if (now_ms < 0 || now_ms < nd->l_last_ts) return nfail(nd, SG_E_TIME, "now_ms lies before the node's earlier local batches");
    node_drain(nd);
    sg_sweep_stats sum{}, one{};
    int rc = node_child(nd, nd->front, sg_param_sweep(nd->front, now_ms, nullptr));
    // a swept handle refuses batches before now_ms: from the first one on, so does the node, also when a later shard fails
    if (!rc) nd->l_last_ts = std::max(nd->l_last_ts, now_ms);
    for (size_t g = 0; !rc && g < nd->shards.size(); ++g) {
        rc = node_child(nd, nd->shards[g], sg_param_sweep(nd->shards[g], now_ms, &one));
        if (!rc) sweep_stats_add(sum, one);
    }
    (void)hipSetDevice(nd->devices[0]);
    if (rc) return rc;
    if (out) *out = sum;
    return SG_OK;
}

int sg_node_cparam_sweep(sg_node* nd, int64_t now_ms, sg_sweep_stats* out) {
    if (!nd) return SG_E_INVAL;
    if (nd->cp_rules.empty()) return nfail(nd, SG_E_INVAL, "no cluster param rules loaded");
    if (now_ms < 0 || now_ms < nd->cp_last_ts) return nfail(nd, SG_E_TIME, "now_ms lies before the node's earlier param batches");
    node_drain(nd);
    sg_sweep_stats sum{}, one{};
    int rc = SG_OK;
    for (size_t g = 0; !rc && g < nd->shards.size(); ++g) {
        sg_handle* h = nd->shards[g];
        if (h->cptab.empty()) continue;  // owns no flowId
        rc = node_child(nd, h, sg_cparam_sweep(h, now_ms, &one));
        if (rc) break;
        sweep_stats_add(sum, one);
        nd->cp_last_ts = std::max(nd->cp_last_ts, now_ms);  // with the first swept shard, also when a later one fails
    }
    (void)hipSetDevice(nd->devices[0]);
    if (rc) return rc;
    if (out) *out = sum;
    return SG_OK;
}

int sg_node_cparam_table_used(sg_node* nd, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity) {
    if (!nd || rule >= nd->cp_rules.size()) return SG_E_INVAL;
    node_drain(nd);
    sg_handle* h = nd->shards[nd->cp_shard_of[rule]];
    const int rc = node_child(nd, h, sg_cparam_table_used(h, nd->cp_local_of[rule], used, live, capacity));
    (void)hipSetDevice(nd->devices[0]);
    return rc;
}

}  // extern "C"
