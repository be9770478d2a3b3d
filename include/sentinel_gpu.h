/*
 * sentinel_gpu.h — C ABI of the MI355X batched flow-decision engine.
 *
 * This is the drop-in boundary for Sentinel's cluster token service hot path.
 * Every entry point below replaces a piece of the Java reference
 * (paths relative to /root/reference; see INTEGRATION.md for the JNI / Panama
 * bindings a Sentinel maintainer would add):
 *
 *   sg_flow_decide_batch      ← TokenService.requestToken(Long,int,boolean)
 *                               sentinel-core/.../cluster/TokenService.java:36, implemented by
 *                               DefaultTokenService.requestToken
 *                               sentinel-cluster/sentinel-cluster-server-default/.../flow/DefaultTokenService.java:39-50
 *                               → ClusterFlowChecker.acquireClusterToken (…/flow/ClusterFlowChecker.java:55-112),
 *                               evaluated for a whole batch of requests in (timestamp, arrival) order.
 *   sg_load_flow_rules        ← ClusterFlowRuleManager.loadRules / applyClusterFlowRule
 *                               (…/flow/rule/ClusterFlowRuleManager.java:254-260, 325-375); metrics of a
 *                               flowId that survives a reload are kept (putMetricIfAbsent :361).
 *   sg_set_namespaces         ← ClusterServerConfigManager (exceedCount / maxOccupyRatio / maxAllowedQps,
 *                               …/server/config/ClusterServerConfigManager.java:303-346) +
 *                               GlobalRequestLimiter.initIfAbsent (…/statistic/limit/GlobalRequestLimiter.java:32-37)
 *                               + ConnectionManager.getConnectedCount (…/server/connection/ConnectionManager.java:47-51)
 *   sg_flow_read_state        ← ClusterMetric window contents (…/statistic/metric/ClusterMetric.java) — read back
 *                               for parity checks and the metric snapshot.
 *   sg_snapshot_metrics       ← ClusterMetricNodeGenerator.generateCurrentNodeMap passQps/blockQps per flowId
 *                               (…/flow/statistic/ClusterMetricNodeGenerator.java:39-105).
 *
 * Conventions: plain C types only, no exceptions across the ABI, 0 = success, negative SG_E* on error
 * (the Java shim then answers TokenResult(FAIL) so FlowRuleChecker.fallbackToLocalOrPass applies,
 * sentinel-core/.../slots/block/flow/FlowRuleChecker.java:166-209). One handle = one submitter.
 */
#ifndef SENTINEL_GPU_H
#define SENTINEL_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---- */
#define SG_OK              0
#define SG_E_INVAL        -1   /* bad argument / invalid rule / bad request record layout          */
#define SG_E_DEVICE       -2   /* HIP runtime error                                               */
#define SG_E_NOMEM        -3   /* device allocation failed                                        */
#define SG_E_UNSUPPORTED  -4   /* configuration outside the device path (e.g. sampleCount > 64)   */
#define SG_E_TIME         -5   /* timestamps negative or not non-decreasing (batch or vs. state)  */
#define SG_E_CAPACITY     -6   /* batch larger than sg_config.max_batch                           */

/* ---- TokenResultStatus (sentinel-core/.../cluster/TokenResultStatus.java:27-53) ---- */
#define SG_STATUS_BAD_REQUEST      (-4)
#define SG_STATUS_TOO_MANY_REQUEST (-2)
#define SG_STATUS_FAIL             (-1)
#define SG_STATUS_OK                 0
#define SG_STATUS_BLOCKED            1
#define SG_STATUS_SHOULD_WAIT        2
#define SG_STATUS_NO_RULE_EXISTS     3

/* ---- ClusterRuleConstant (sentinel-core/.../slots/block/ClusterRuleConstant.java:27-28) ---- */
#define SG_THRESHOLD_AVG_LOCAL 0
#define SG_THRESHOLD_GLOBAL    1

/* ---- ClusterFlowEvent ordinals (…/flow/statistic/data/ClusterFlowEvent.java:22-52) ---- */
#define SG_EV_PASS           0
#define SG_EV_BLOCK          1
#define SG_EV_PASS_REQUEST   2
#define SG_EV_BLOCK_REQUEST  3
#define SG_EV_OCCUPIED_PASS  4
#define SG_EV_OCCUPIED_BLOCK 5
#define SG_EV_WAITING        6
#define SG_NUM_EVENTS        7

/* ---- request key encoding ----
 * key = dense rule index assigned by sg_load_flow_rules (position in the rule array),
 * OR-ed with SG_KEY_PRIO for prioritized requests. Two reserved values let the host shim
 * submit requests it has already classified without splitting the batch:
 *   SG_KEY_BAD     → BAD_REQUEST   (DefaultTokenService.notValidRequest, id null/<=0, :87-89)
 *   SG_KEY_NO_RULE → NO_RULE_EXISTS (rule lookup miss, DefaultTokenService.java:44-47)
 * Any other index >= number of loaded rules also answers NO_RULE_EXISTS. */
#define SG_KEY_PRIO    0x80000000u
#define SG_KEY_INDEX   0x7FFFFFFFu
#define SG_KEY_NO_RULE 0x7FFFFFFFu
#define SG_KEY_BAD     0x7FFFFFFEu

/* sg_config.flags: force one walker for every flowId segment (testing both walkers on any trace). */
#define SG_FLAG_SERIAL_ONLY 1   /* one lane per flowId, however long its segment */
#define SG_FLAG_WAVE_ONLY   2   /* one wave per flowId, however short its segment */
#define SG_FLAG_RING_REREAD 4   /* short walker without the register ring snapshot (re-reads the ring)   */

/* Largest sampleCount the device walker keeps in a wave (one bucket per lane). */
#define SG_MAX_SAMPLE_COUNT 64

typedef struct sg_handle sg_handle;

typedef struct sg_config {
    int32_t  device;            /* HIP device ordinal                                   */
    int32_t  flags;             /* SG_FLAG_* (0 = default walker selection)             */
    double   exceed_count;      /* ServerFlowConfig.exceedCount, default 1.0 (:26)      */
    double   max_occupy_ratio;  /* ServerFlowConfig.maxOccupyRatio, default 1.0 (:27)  */
    uint64_t max_batch;         /* largest n accepted by sg_flow_decide_batch           */
} sg_config;

/* One cluster-mode QPS FlowRule with its ClusterFlowConfig
 * (FlowRule.java:52-95, ClusterFlowConfig.java:29-74). */
typedef struct sg_flow_rule {
    int64_t flow_id;            /* ClusterFlowConfig.flowId (must be > 0)                      */
    double  count;              /* FlowRule.count (threshold, >= 0)                            */
    int32_t threshold_type;     /* SG_THRESHOLD_AVG_LOCAL / SG_THRESHOLD_GLOBAL                */
    int32_t sample_count;       /* ClusterFlowConfig.sampleCount, default 10                   */
    int32_t window_interval_ms; /* ClusterFlowConfig.windowIntervalMs, default 1000            */
    int32_t namespace_id;       /* index into the sg_set_namespaces array                      */
} sg_flow_rule;

/* Per-namespace server settings. */
typedef struct sg_namespace {
    int32_t limiter_enabled;    /* GlobalRequestLimiter has a RequestLimiter for this namespace */
    int32_t connected_count;    /* ConnectionManager.getConnectedCount(namespace)               */
    double  max_allowed_qps;    /* ServerFlowConfig.maxAllowedQps, default 30000 (:31)          */
} sg_namespace;

/* One token request: requestToken(flowId→key, acquireCount, prioritized) at time ts_ms. */
typedef struct sg_req {
    int64_t  ts_ms;             /* explicit TimeUtil.currentTimeMillis() of the call          */
    uint32_t key;               /* rule index | SG_KEY_PRIO, or SG_KEY_BAD / SG_KEY_NO_RULE     */
    int32_t  acquire;           /* acquireCount; <= 0 → BAD_REQUEST                            */
} sg_req;

/* TokenResult (sentinel-core/.../cluster/TokenResult.java:26-35) minus tokenId/attachments. */
typedef struct sg_result {
    int32_t status;
    int32_t remaining;
    int32_t wait_ms;
} sg_result;

/* ---- hot-parameter flow control (ParamFlowChecker, sentinel-extension/sentinel-parameter-flow-control) ---- */

/* One QPS ParamFlowRule (ParamFlowRule.java:45-83). The parameter value itself is a u64 chosen by the
 * caller (a Long argument as is, other types through the shim's value dictionary). */
typedef struct sg_param_rule {
    double   count;             /* ParamFlowRule.count (token count per duration)                 */
    int64_t  duration_sec;      /* durationInSec, default 1                                       */
    int32_t  burst;             /* burstCount, default 0                                          */
    int32_t  behavior;          /* CONTROL_BEHAVIOR_DEFAULT 0 (token bucket) / RATE_LIMITER 2      */
    int32_t  max_queueing_ms;   /* maxQueueingTimeMs (throttle), default 0                        */
    uint32_t hot_begin;         /* this rule's hot items: hot[hot_begin .. hot_begin + hot_count) */
    uint32_t hot_count;
    int32_t  capacity_log2;     /* device table: 2^capacity_log2 distinct values (0 = 2^20)        */
} sg_param_rule;

/* ParamFlowItem → parsed hot item: value-specific threshold (ParamFlowRuleUtil.parseHotItems :188-209). */
typedef struct sg_param_hot_item {
    uint64_t value;
    int32_t  threshold;
    int32_t  reserved;
} sg_param_hot_item;

/* One single-value check: passSingleValueCheck(rule, acquireCount, value) at ts_ms. */
typedef struct sg_param_req {
    int64_t  ts_ms;
    uint64_t value;
    uint32_t rule;              /* index into the loaded param rules                               */
    int32_t  acquire;           /* acquireCount                                                    */
} sg_param_req;

/* ---- ParamFlowSlot: every param rule of a resource, collection/array arguments, THREAD grade ----
 * SphU.entry(resource, count, args...) through ParamFlowSlot.checkFlow (ParamFlowSlot.java:66-93): the resource's
 * rules in load order (the first failing one throws ParamFlowException), each on args[paramIdx]
 * (ParamFlowChecker.passCheck :48-73): no argument or a null one passes, a collection / array is checked element by
 * element in order with the state changes of the elements before a failing one kept (passLocalCheck :75-104),
 * QPS rules through the token bucket / throttle of sg_param_*, THREAD rules against the per-(resource, paramIdx,
 * value) thread counts (passSingleValueCheck :114-122) that ParamFlowStatisticEntryCallback / ExitCallback keep
 * (ParameterMetric.addThreadCount / decreaseThreadCount :125-239). Rules are sg_param_rule plus the fields below;
 * a negative paramIdx is resolved against the first call's argument count and then kept (applyRealParamIdx
 * :57-64). Resources with several rules and collection arguments are walked one event at a time per resource. */
#define SG_ARG_NULL        0
#define SG_ARG_VALUE       1
#define SG_ARG_COLLECTION  2
/* ParamFlowRule.clusterMode with its ParamFlowClusterConfig (cluster_mode: SG_CLUSTER_MODE_* as for flow rules,
 * below). passCheck sends a clusterMode QPS rule to passClusterCheck (ParamFlowChecker.java:71-73, :278-303): on a
 * node that is neither token client nor server (sg_local_set_cluster_state, NOT_STARTED the default) pickClusterService
 * is null and fallbackToLocalOrPass (:305-313) applies — SG_CLUSTER_MODE_FALLBACK checks the rule locally,
 * SG_CLUSTER_MODE_NO_FALLBACK passes it. On a node whose embedded token server runs on this handle (SERVER) the rule
 * requests a param token for all of the argument's values (toCollection) from the handle's cluster param state
 * (sg_cparam_load_rules, the namespace limiter included: DefaultTokenService.requestParamToken →
 * ClusterParamFlowChecker.acquireClusterToken) in event order: OK passes, BLOCKED throws ParamFlowException,
 * NO_RULE_EXISTS / BAD_REQUEST / TOO_MANY_REQUEST go to fallbackToLocalOrPass. THREAD-grade cluster rules are checked
 * locally (passCheck's condition). SG_CLUSTER_MODE_INVALID (ParamFlowRuleUtil.checkCluster :54-66 failed: no config,
 * an invalid window or flowId <= 0) drops the rule at load, as ParamFlowRuleManager does. A token client (CLIENT)
 * with cluster-mode QPS rules loaded is SG_E_UNSUPPORTED. */
typedef struct sg_pslot_rule {
    sg_param_rule rule;          /* token bucket / throttle parameters, hot items                          */
    uint32_t      resource;      /* resource index                                                         */
    int32_t       param_idx;     /* ParamFlowRule.paramIdx                                                 */
    int32_t       grade;         /* 0 FLOW_GRADE_THREAD, 1 FLOW_GRADE_QPS                                 */
    int32_t       cluster_mode;  /* SG_CLUSTER_MODE_* (0: a local rule)                                     */
    uint32_t      cluster_key;   /* SERVER: ParamFlowClusterConfig.flowId as a rule index of this handle's
                                    sg_cparam_load_rules (SG_KEY_NO_RULE: the server has no rule for it)     */
    int32_t       reserved;
} sg_pslot_rule;
typedef struct sg_pslot_arg {    /* one argument: null, a value, or a collection / array of values        */
    uint32_t value_begin;
    uint32_t value_count;
    int32_t  kind;               /* SG_ARG_*                                                              */
    int32_t  reserved;           /* SG_ARG_COLLECTION: the caller's label id of the collection's String.valueOf, read
                                    only by the block log (sg_local_block_log, SG_BLOCK_APP_LABEL); 0 = unlabelled */
} sg_pslot_arg;
typedef struct sg_pslot_event {  /* an entry (SphU.entry) or the exit of a passed entry (its own arguments) */
    int64_t  ts_ms;
    uint32_t resource;
    int32_t  count;              /* acquireCount                                                          */
    int32_t  kind;               /* SG_LOCAL_ENTRY / SG_LOCAL_EXIT                                         */
    uint32_t arg_begin;          /* args[arg_begin .. + arg_count)                                         */
    uint32_t arg_count;
    int32_t  args_null;          /* 1: the Object[] args itself is null (checkFlow returns at once)         */
} sg_pslot_event;
typedef struct sg_pslot_result {
    int32_t pass;                /* entries: 1 pass / 0 ParamFlowException; exits: 1                       */
    int32_t rule;                /* the rule that threw (index into the loaded rules), else -1              */
} sg_pslot_result;
/* Loads the rules (state of sg_param_* starts empty, as for sg_param_load_rules). */
int sg_pslot_load_rules(sg_handle* h, const sg_pslot_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                        uint32_t n_hot, uint32_t n_resources);
/* A time-ordered batch; events, args, values and results are DEVICE pointers (asynchronous on stream). A batch
 * rejected from its events alone (SG_E_TIME, SG_E_INVAL) changes no state, the value tables' free slots included. A
 * table found full while the batch is walked — a param rule's values, the thread counts, or the embedded token
 * server's cluster param values — is SG_E_CAPACITY and can leave the batch partly applied: the state then holds
 * the events decided up to there, and the last timestamp does not advance. */
int sg_pslot_decide_batch(sg_handle* h, const sg_pslot_event* ev, uint64_t n, const sg_pslot_arg* args,
                          uint64_t n_args, const uint64_t* values, uint64_t n_values, sg_pslot_result* out, void* stream);
int sg_pslot_decide_batch_host(sg_handle* h, const sg_pslot_event* ev, uint64_t n, const sg_pslot_arg* args,
                               uint64_t n_args, const uint64_t* values, uint64_t n_values, sg_pslot_result* out);
/* ParameterMetric.getThreadCount(paramIdx, value) of a resource, and a rule's current paramIdx. */
int sg_pslot_thread_count(sg_handle* h, uint32_t resource, int32_t param_idx, uint64_t value, int64_t* count);
int sg_pslot_param_idx(sg_handle* h, uint32_t rule, int32_t* param_idx);

/* ---- pace controller: FlowRule with CONTROL_BEHAVIOR_RATE_LIMITER (RateLimiterController) ---- */

/* One FlowRule whose controller is RateLimiterController(maxQueueingTimeMs, count)
 * (sentinel-core/.../slots/block/flow/controller/RateLimiterController.java:35-38). Each rule owns one
 * latestPassedTime, initially -1. */
typedef struct sg_pace_rule {
    double   count;             /* FlowRule.count (requests per second), >= 0                      */
    int32_t  max_queueing_ms;   /* FlowRule.maxQueueingTimeMs, default 500                         */
    int32_t  reserved;
} sg_pace_rule;

/* canPass(node, acquireCount) at ts_ms (RateLimiterController.java:46-91). */
typedef struct sg_pace_req {
    int64_t  ts_ms;
    uint32_t rule;              /* index into the loaded pace rules; >= n passes (no rule)         */
    int32_t  acquire;           /* acquireCount                                                    */
} sg_pace_req;

#define SG_PACE_BLOCKED (-1)    /* result: canPass false; >= 0: passes after sleeping that many ms */

/* ---- cluster hot-parameter tokens (TokenService.requestParamToken → ClusterParamFlowChecker) ---- */

/* One cluster-mode ParamFlowRule with its ParamFlowClusterConfig (ParamFlowRule.java, ParamFlowClusterConfig.java). */
typedef struct sg_cparam_rule {
    int64_t  flow_id;            /* ParamFlowClusterConfig.flowId (> 0)                                   */
    double   count;              /* ParamFlowRule.count (threshold of values without a hot item)         */
    int32_t  threshold_type;     /* SG_THRESHOLD_AVG_LOCAL / SG_THRESHOLD_GLOBAL                           */
    int32_t  sample_count;       /* ParamFlowClusterConfig.sampleCount, default 10                         */
    int32_t  window_interval_ms; /* windowIntervalMs, default 1000                                         */
    int32_t  namespace_id;       /* index into the sg_set_namespaces array                                 */
    uint32_t hot_begin;          /* this rule's hot items (exclusive item counts): hot[hot_begin ..)     */
    uint32_t hot_count;
} sg_cparam_rule;

/* requestParamToken(ruleId→key, acquireCount, params) at ts_ms; the parameter values are
 * values[value_begin .. value_begin + value_count) of the batch's u64 value array. */
typedef struct sg_cparam_req {
    int64_t  ts_ms;
    uint32_t key;                /* rule index, or SG_KEY_BAD / SG_KEY_NO_RULE                             */
    int32_t  acquire;
    uint32_t value_begin;
    uint32_t value_count;        /* 0 → BAD_REQUEST (params empty, DefaultTokenService.java:54)            */
} sg_cparam_req;

/* ---- concurrent (thread-grade) cluster tokens: TokenService.requestConcurrentToken / releaseConcurrentToken ----
 * DefaultTokenService.java:66-85 → ConcurrentClusterFlowChecker.acquireConcurrentToken / releaseConcurrentToken
 * (srv/flow/ConcurrentClusterFlowChecker.java:48-101) over the loaded cluster flow rules: one nowCalls counter per
 * flowId (CurrentConcurrencyManager; kept for flowIds that survive a rule reload, ClusterFlowRuleManager.java:
 * 356-358) and a token table (TokenCacheNodeManager). Token ids are deterministic instead of UUID bits: an acquire
 * that passes gets id 1 + (number of concurrent requests this handle decided before it). */
#define SG_CONC_ACQUIRE 0
#define SG_CONC_RELEASE 1
#define SG_STATUS_RELEASE_OK      6   /* TokenResultStatus.RELEASE_OK      */
#define SG_STATUS_ALREADY_RELEASE 7   /* TokenResultStatus.ALREADY_RELEASE */
typedef struct sg_conc_req {
    int64_t  ts_ms;
    uint64_t token_id;           /* release: the token (0 = null → BAD_REQUEST); acquire: ignored          */
    uint32_t key;                /* acquire: rule index (or SG_KEY_BAD / SG_KEY_NO_RULE); release: ignored   */
    int32_t  acquire;            /* acquire: acquireCount (<= 0 → BAD_REQUEST)                              */
    uint32_t client;             /* acquire: client address id, 0 = null / "" (→ BAD_REQUEST)               */
    int32_t  kind;               /* SG_CONC_*                                                              */
} sg_conc_req;
typedef struct sg_conc_result {
    int32_t  status;             /* OK / BLOCKED / BAD_REQUEST / NO_RULE_EXISTS / RELEASE_OK / ALREADY_RELEASE */
    int32_t  reserved;
    uint64_t token_id;           /* acquire OK: the new token                                               */
} sg_conc_result;

/* Per-rule ClusterFlowConfig.clientOfflineTime / resourceTimeout (ms) for the token expiry, rule index order;
 * defaults 2000 / 2000 (ClusterFlowConfig.java); reset to the defaults by sg_load_flow_rules. */
int sg_conc_set_rule_timeouts(sg_handle* h, const int64_t* client_offline_ms, const int64_t* resource_timeout_ms,
                              uint32_t n);
/* A time-ordered batch of acquires and releases (DEVICE pointers; asynchronous on stream). */
int sg_conc_decide_batch(sg_handle* h, const sg_conc_req* req, uint64_t n, sg_conc_result* out, void* stream);
int sg_conc_decide_batch_host(sg_handle* h, const sg_conc_req* req, uint64_t n, sg_conc_result* out);
/* RegularExpireStrategy.clearToken (…/statistic/concurrent/expire/RegularExpireStrategy.java:94-123) at now_ms:
 * removes tokens whose client is offline past clientOfflineTime, or held more than 2 x resourceTimeout, and gives
 * their counts back. client_online[c] = ConnectionManager.isClientOnline(client c) (ids >= n_clients: offline).
 * Every token is examined (the reference stops after 1000 keys in ConcurrentHashMap order). *removed = count. */
int sg_conc_expire(sg_handle* h, int64_t now_ms, const uint8_t* client_online, uint32_t n_clients, uint64_t* removed);
/* nowCalls of rule `key` and the number of live tokens. */
int sg_conc_read_state(sg_handle* h, uint32_t key, int32_t* now_calls, uint64_t* live_tokens);

/* ---- local slot chain: StatisticSlot → FlowSlot (DefaultController) → DegradeSlot (circuit breakers) ---- */

/* DegradeRule (sentinel-core/.../slots/block/degrade/DegradeRule.java). A rule that DegradeRuleManager.isValidRule
 * (DegradeRuleManager.java:183-202) drops must not be sent: sg_local_load_rules refuses the whole load with
 * SG_E_INVAL ("invalid degrade rule") for a grade outside SG_DEGRADE_*, count < 0 or NaN, time_window_sec <= 0,
 * min_request_amount <= 0, stat_interval_ms <= 0, an RT slow_ratio_threshold outside [0, 1] (NaN included) or an
 * exception ratio count > 1. The bounds themselves are valid (window 1, amount 1, ratios 0.0 and 1.0). */
#define SG_DEGRADE_RT              0
#define SG_DEGRADE_EXCEPTION_RATIO 1
#define SG_DEGRADE_EXCEPTION_COUNT 2
typedef struct sg_degrade_rule {
    int32_t grade;                /* SG_DEGRADE_*                                            */
    int32_t time_window_sec;      /* timeWindow: recovery timeout in seconds                  */
    double  count;                /* RT: max allowed RT (rounded); else ratio / count         */
    double  slow_ratio_threshold; /* RT only (default 1.0)                                    */
    int32_t min_request_amount;   /* default 5                                               */
    int32_t stat_interval_ms;     /* default 1000                                            */
} sg_degrade_rule;

/* One resource: its FlowRule with the default controller (limitApp "default", DIRECT strategy, read
 * from the resource's ClusterNode) and up to two DegradeRules, checked in order. sg_local_load_flow_rules
 * below replaces the flow rules with any number per resource. */
typedef struct sg_local_rule {
    double  flow_count;           /* FlowRule.count                                           */
    int32_t flow_grade;           /* 0 FLOW_GRADE_THREAD, 1 FLOW_GRADE_QPS, -1 no flow rule    */
    int32_t n_breakers;           /* 0..2                                                     */
    sg_degrade_rule breakers[2];
} sg_local_rule;

#define SG_LOCAL_ENTRY      0     /* SphU.entry(resource, count, prioritized)                 */
#define SG_LOCAL_EXIT       1     /* Entry.exit() of a passed entry                           */
#define SG_LOCAL_EXIT_ERROR 2     /* Entry.exit() after Tracer.traceEntry(business exception) */
typedef struct sg_local_event {
    int64_t  ts_ms;               /* TimeUtil time of the entry or exit                        */
    int64_t  create_ts;           /* exit: the entry's createTimestamp                         */
    uint32_t resource;            /* resource index | SG_KEY_PRIO (prioritized entry)          */
    int32_t  count;               /* acquireCount of the entry (also the exit's batchCount)    */
    int32_t  kind;                /* SG_LOCAL_*                                               */
    int32_t  origin;              /* Context origin: 0 = none (""), 1..n_origins = an origin id   */
} sg_local_event;

#define SG_LOCAL_PASS          0  /* passes; wait_ms > 0: after the rate limiter's sleep        */
#define SG_LOCAL_BLOCK_FLOW    1  /* FlowException                                            */
#define SG_LOCAL_BLOCK_DEGRADE 2  /* DegradeException                                         */
#define SG_LOCAL_PASS_WAIT     3  /* PriorityWaitException: passes after wait_ms              */
                                  /* 4: SG_LOCAL_BLOCK_PARAM (sg_slot_decide_batch, below)     */
                                  /* 5: SG_LOCAL_BLOCK_AUTHORITY (sg_local_load_authority_rules) */
typedef struct sg_local_result {
    int32_t status;               /* entries: SG_LOCAL_*; exits: 0                            */
    int32_t wait_ms;
} sg_local_result;

/* Node-wide statistic settings of the local chain (static properties in the reference). */
typedef struct sg_local_config {
    int32_t sample_count;         /* SampleCountProperty.SAMPLE_COUNT, default 2 (1..60)          */
    int32_t interval_ms;          /* IntervalProperty.INTERVAL, default 1000                      */
    int32_t occupy_timeout_ms;    /* OccupyTimeoutProperty.occupyTimeout, default 500              */
    int32_t cold_factor;          /* ColdFactorProperty.coldFactor (SentinelConfig, default 3; <= 1 → 3) */
} sg_local_config;

/* ---- the flow rules of the local chain: FlowRuleManager.loadRules → FlowRuleChecker.checkFlow ----
 * FlowRule (core/.../slots/block/flow/FlowRule.java) of one resource, with its traffic-shaping controller
 * (FlowRuleUtil.generateRater, FlowRuleUtil.java:132-149) and limitApp node selection
 * (FlowRuleChecker.selectNodeByRequesterAndStrategy, FlowRuleChecker.java:115-145). Origins are the caller's
 * dense ids for the Context origin strings (never "default" / "other"). */
#define SG_CONTROL_DEFAULT               0  /* DefaultController (THREAD rules always use it)        */
#define SG_CONTROL_WARM_UP               1  /* WarmUpController                                       */
#define SG_CONTROL_RATE_LIMITER          2  /* RateLimiterController                                  */
#define SG_CONTROL_WARM_UP_RATE_LIMITER  3  /* WarmUpRateLimiterController                            */
#define SG_LIMIT_APP_DEFAULT   0            /* limitApp "default": the resource's ClusterNode         */
#define SG_LIMIT_APP_OTHER   (-1)           /* limitApp "other": origins no rule of the resource names */
#define SG_STRATEGY_DIRECT     0            /* RuleConstant.STRATEGY_DIRECT: the node limitApp selects      */
#define SG_STRATEGY_RELATE     1            /* STRATEGY_RELATE: the ClusterNode of resource ref_resource     */
#define SG_STRATEGY_CHAIN      2            /* STRATEGY_CHAIN: the resource's DefaultNode of context ref_resource,
                                               only for entries in that context                             */
/* FlowRule.clusterMode with its ClusterFlowConfig (FlowRuleChecker.passClusterCheck :147-164). On a node that is
 * neither token client nor server (CLUSTER_NOT_STARTED, the default) pickClusterService() is null, so
 * fallbackToLocalOrPass (:166-175) applies. On a node whose embedded token server runs on this handle
 * (sg_local_set_cluster_state(SERVER), DefaultEmbeddedTokenServer.requestToken → DefaultTokenService, :46-51) a
 * cluster-mode rule requests a token for its flowId from the handle's own cluster flow state (sg_load_flow_rules,
 * the namespace limiter included) in the batch's event order, and applyTokenResult (:186-209) maps the answer: OK
 * passes, SHOULD_WAIT passes after wait_ms (added to the entry's wait), BLOCKED throws FlowException, and
 * NO_RULE_EXISTS / BAD_REQUEST / FAIL / TOO_MANY_REQUEST go to fallbackToLocalOrPass. */
#define SG_CLUSTER_MODE_OFF         0       /* a local rule                                                 */
#define SG_CLUSTER_MODE_FALLBACK    1       /* clusterMode, fallbackToLocalWhenFail: checked as a local rule  */
#define SG_CLUSTER_MODE_NO_FALLBACK 2       /* clusterMode without fallback: the rule is not activated (pass) */
#define SG_CLUSTER_MODE_INVALID   (-1)      /* clusterMode with an invalid ClusterFlowConfig
                                               (FlowRuleUtil.checkClusterField :197-215): ignored at load   */
typedef struct sg_local_flow_rule {
    uint32_t resource;            /* resource index (sg_local_load_rules order)                    */
    int32_t  grade;               /* 0 FLOW_GRADE_THREAD, 1 FLOW_GRADE_QPS                        */
    double   count;
    int32_t  control_behavior;    /* SG_CONTROL_*                                                 */
    int32_t  limit_app;           /* SG_LIMIT_APP_DEFAULT, SG_LIMIT_APP_OTHER or an origin id > 0   */
    int32_t  strategy;            /* SG_STRATEGY_*                                                */
    int32_t  warm_up_period_sec;  /* warmUpPeriodSec, default 10                                  */
    int32_t  max_queueing_ms;     /* maxQueueingTimeMs, default 500                               */
    int32_t  ref_resource;        /* RELATE: resource index; CHAIN: context id; < 0: refResource blank */
    int32_t  cluster_mode;        /* SG_CLUSTER_MODE_*                                            */
    int32_t  cluster_config;      /* the caller's id of the ClusterFlowConfig value (FlowRule.equals
                                     compares it; 0 = none)                                       */
    uint32_t cluster_key;         /* cluster mode on an embedded server: ClusterFlowConfig.flowId as a rule
                                     index of this handle's sg_load_flow_rules (SG_KEY_NO_RULE: the server
                                     has no rule for it, as sg_req.key)                           */
} sg_local_flow_rule;

/* ClusterStateManager state of the node (ClusterStateManager.java: CLUSTER_CLIENT 0, CLUSTER_SERVER 1,
 * CLUSTER_NOT_STARTED -1). NOT_STARTED and SERVER (the embedded token server on this handle, see above) are
 * decided on the device. In SERVER state the resources whose cluster-mode rules share a flowId, or name flowIds of
 * one limiter-enabled namespace, walk together in event order (one key group), and a local batch with such rules
 * must not precede the handle's flow batches in time (SG_E_TIME), nor they it. CLIENT sends tokens over the
 * network, which a batch cannot call in order: loading cluster-mode rules in CLIENT state (or entering it while they
 * are loaded) is SG_E_UNSUPPORTED, as is SERVER on a sharded handle (sg_set_shard) whose cluster
 * rules name a limiter-enabled namespace. The state is the handle's (one ClusterStateManager per node): it also decides
 * the cluster-mode ParamFlowRules of sg_pslot_load_rules, in sg_pslot_decide_batch and in the slot chain
 * (sg_slot_decide_batch). In SERVER state the resources whose cluster-mode param rules share a flowId (a cluster param
 * rule of sg_cparam_load_rules) or a limiter-enabled namespace walk as one key group, and the batch's events may not
 * precede the handle's cluster param batches in time (SG_E_TIME), nor they it. */
#define SG_CLUSTER_CLIENT        0
#define SG_CLUSTER_SERVER        1
#define SG_CLUSTER_NOT_STARTED (-1)
int sg_local_set_cluster_state(sg_handle* h, int32_t state);

/* Per-call timing of the last sg_flow_decide_batch (device time, HIP events on the call's stream). */
typedef struct sg_batch_stats {
    float    total_ms;          /* whole pipeline                                         */
    float    walk_ms;           /* per-flowId walk kernels                                */
    float    sort_ms;           /* key partition (radix sort)                             */
    uint64_t touched_keys;      /* distinct flowIds that received >= 1 request            */
    uint64_t long_segments;     /* flowIds walked by a whole wave                         */
    uint64_t skipped_ranges;    /* all-BLOCKED period tails the wave walker jumped over   */
} sg_batch_stats;

int         sg_create(const sg_config* cfg, sg_handle** out);
void        sg_destroy(sg_handle* h);
const char* sg_last_error(const sg_handle* h);

int sg_set_namespaces(sg_handle* h, const sg_namespace* ns, uint32_t n);

/* Marks the handle as one of `world` shards of a node's flowIds (flowIds hashed over the GPUs,
 * no collective on the decision path). GlobalRequestLimiter's per-namespace QPS limiter counts every request of
 * the namespace in node order (GlobalRequestLimiter.java:46-55, ClusterFlowChecker.allowProceed :45-51), which a
 * shard does not see on its own: with world > 1 and limiter-enabled namespaces every flow batch of the shard goes
 * through the exchange below — synchronous, pipelined (sg_flow_enqueue) and host-pipelined (sg_flow_submit) flow
 * batches and cluster param batches (sg_cparam_decide_batch) alike; a batch without an armed exchange is refused
 * with SG_E_UNSUPPORTED. */
int sg_set_shard(sg_handle* h, int32_t rank, int32_t world);

/* Sharded namespace limiter exchange (replaces GlobalRequestLimiter.tryPass's node-wide counting):
 *   1. sg_lim_arrivals (flow batches) / sg_lim_arrivals_param (cluster param batches, ClusterParamFlowChecker
 *      .java:43-45 shares the limiter): this shard's valid requests of limited namespaces per (limiter slot,
 *      millisecond), counts_out[slot * n_ms + (ts_ms - t_base)] (DEVICE, n_lim * n_ms uint32; slots = the
 *      limiter-enabled namespaces in sg_set_namespaces order). [t_base, t_base + n_ms) is node-wide and must hold
 *      every shard's limited requests of the node batch (SG_E_INVAL otherwise); n_ms <= 65536. `req` is device
 *      memory (or pinned host memory the device can read). Synchronous on `stream`; batches in flight on the
 *      pipeline go on.
 *   2. the node all-gathers the counts of its `world` shards (RCCL) into gathered[world][n_lim][n_ms] (DEVICE);
 *   3. sg_lim_exchange arms the handle's next flow or param batch with them: sg_flow_decide_batch / _host,
 *      sg_flow_enqueue, sg_flow_submit or sg_cparam_decide_batch / _host consumes it. The buffer must stay valid
 *      until that call returns (the pipelined calls copy it before returning).
 * The node's arrival order is (ts_ms, shard rank, position in the shard's batch). Every shard walks the same
 * per-100 ms node arrivals, so each keeps an identical replica of the namespace windows, and admits its request
 * iff its node-wide rank in the period is below the period's quota: the results equal one handle deciding the
 * merged batch. A shard with no requests in a node batch still calls sg_lim_exchange and sg_flow_decide_batch
 * with n = 0 (its replica advances). A shard batch rejected by an error (SG_E_TIME, SG_E_INVAL, SG_E_CAPACITY …)
 * still walks the armed node arrivals, so its replica stays equal to the other shards' (the node counted that shard's
 * requests as limiter arrivals; their flow decisions did not happen). */
int sg_lim_arrivals(sg_handle* h, const sg_req* req, uint64_t n, int64_t t_base, uint32_t n_ms, uint32_t* counts_out,
                    uint64_t counts_words, void* stream);
int sg_lim_arrivals_param(sg_handle* h, const sg_cparam_req* req, uint64_t n, int64_t t_base, uint32_t n_ms,
                          uint32_t* counts_out, uint64_t counts_words, void* stream);
int sg_lim_exchange(sg_handle* h, const uint32_t* gathered, uint64_t gathered_words, int64_t t_base, uint32_t n_ms);
/* The handle's limiter-slot count n_lim (limiter-enabled namespaces of sg_set_namespaces): counts_words of
 * sg_lim_arrivals must equal n_lim * n_ms and gathered_words of sg_lim_exchange world * n_lim * n_ms (SG_E_INVAL). */
int sg_lim_slots(const sg_handle* h, uint32_t* n_lim);
int sg_load_flow_rules(sg_handle* h, const sg_flow_rule* rules, uint32_t n);

/* Decide a batch. req/out are DEVICE pointers (HBM-resident); stream is a hipStream_t (NULL = default).
 * Requests must be ordered by (ts_ms, arrival); ts_ms must be >= 0 and >= every ts of earlier batches. */
int sg_flow_decide_batch(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, void* stream);

/* Same with HOST buffers (H2D + D2H included; synchronous). */
int sg_flow_decide_batch_host(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out);

/* Asynchronous host pipeline — what a token server's request loop calls: sg_flow_submit
 * enqueues H2D of req, the decision pipeline and D2H into out, and returns at once with a ticket; up to 3
 * batches are in flight (H2D of batch i+1 and D2H of batch i-1 overlap the compute of batch i; compute runs in
 * submission order, so batches must still be time-ordered). A 4th submit first completes the oldest batch.
 * req/out are HOST memory and must stay untouched until the ticket completes; allocate them with sg_host_alloc
 * (pinned) for the copies to run asynchronously. sg_flow_poll: 1 done and OK, 0 still running, < 0 that batch's
 * error (the batch was rejected, as sg_flow_decide_batch would); sg_flow_wait blocks and returns SG_OK or that
 * error. Every other call on the handle first completes the batches in flight. Ticket 0 (empty batch) is done.
 * Batches in flight are pipelined on the device: the front half of batch i+1 (validation, sort by flowId,
 * segment lists) runs beside the walkers of batch i, two batch workspaces alternating; a batch that fails the
 * cross-batch time check is still rejected as a whole (checked before its walkers). */
int   sg_flow_submit(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, uint64_t* ticket);
/* The same pipeline for DEVICE buffers (ClusterFlowChecker over HBM-resident batches back to back: the
 * DefaultTokenService request loop at full rate): enqueues the batch and returns a ticket for
 * sg_flow_poll / sg_flow_wait. req/out must stay allocated and untouched until the ticket completes (each batch
 * in flight needs its own out buffer); up to 4 batches in flight (a 5th enqueue first completes the oldest). */
int   sg_flow_enqueue(sg_handle* h, const sg_req* req, uint64_t n, sg_result* out, uint64_t* ticket);
int   sg_flow_poll(sg_handle* h, uint64_t ticket);
int   sg_flow_wait(sg_handle* h, uint64_t ticket);
void* sg_host_alloc(sg_handle* h, uint64_t bytes);   /* pinned (page-locked) host memory, NULL on failure */
void  sg_host_free(sg_handle* h, void* p);

/* Opt-in per-call timing (adds HIP events; off by default). */
int sg_enable_stats(sg_handle* h, int on);
int sg_get_stats(const sg_handle* h, sg_batch_stats* out);

/* Read one flowId's window: starts[sample_count] (INT64_MIN = never-created bucket),
 * counters[sample_count * SG_NUM_EVENTS], occupy[2] = {occupied PASS, occupied PASS_REQUEST}. */
int sg_flow_read_state(sg_handle* h, uint32_t key, int64_t* starts, int64_t* counters, int64_t* occupy);

/* Bulk copy of every flowId's window to / from HOST memory — the checkpoint of the cluster flow state (the
 * reference keeps it only in memory; SURVEY §5 "checkpoint / resume") and the parity harness's state dump.
 * ring: n_rules * stride * 8 int64 = per flowId `stride` buckets {start, PASS, BLOCK, PASS_REQUEST,
 * BLOCK_REQUEST, OCCUPIED_PASS, OCCUPIED_BLOCK, WAITING} (start INT64_MIN = never-created slot; slots >= the
 * flow's sampleCount are unused and stay INT64_MIN), occ: n_rules * 2 int64 = {occupied PASS, occupied
 * PASS_REQUEST} (ClusterMetricLeapArray.occupyCounter). stride = the largest sampleCount of the loaded rules
 * (written to *stride; with ring == NULL only *stride is written). Import expects the same layout and the same
 * loaded rules; it is synchronous. */
int sg_flow_export_state(sg_handle* h, int64_t* ring, uint64_t ring_words, int64_t* occ, uint64_t occ_words,
                         int32_t* stride);
int sg_flow_import_state(sg_handle* h, const int64_t* ring, uint64_t ring_words, const int64_t* occ,
                         uint64_t occ_words);

/* Per-flowId {passQps, blockQps} at time now_ms (ClusterMetric.getAvg(PASS/BLOCK) without the
 * currentWindow side effect); out has 2*n_rules doubles, HOST memory. */
int sg_snapshot_metrics(sg_handle* h, int64_t now_ms, double* out, uint64_t cap);

/* Same into DEVICE memory (2*n_rules doubles, {passQps, blockQps} per flowId), asynchronous on `stream`:
 * the per-GPU input of the node-wide RCCL metric rollup. */
int sg_snapshot_metrics_device(sg_handle* h, int64_t now_ms, double* out_dev, uint64_t cap, void* stream);
/* sg_snapshot_metrics_device ordered after every batch enqueued so far on the pipeline (sg_flow_enqueue /
 * sg_flow_submit), without draining it: completes with the returned ticket (sg_flow_poll / sg_flow_wait). */
int sg_snapshot_metrics_enqueue(sg_handle* h, int64_t now_ms, double* out_dev, uint64_t cap, uint64_t* ticket);

/* Hot-parameter rules (replaces ParamFlowRuleManager.loadRules → ParameterMetric maps). A reload starts
 * every rule's value table empty. Hot items of a rule may be given in any order. */
int sg_param_load_rules(sg_handle* h, const sg_param_rule* rules, uint32_t n,
                        const sg_param_hot_item* hot, uint32_t n_hot);
/* passSingleValueCheck for a time-ordered batch: pass[i] = 1 admitted / 0 blocked. req/pass are DEVICE
 * pointers. Requests naming a rule index >= n pass (no rule). A rejected batch (SG_E_TIME; SG_E_CAPACITY: a rule
 * met more distinct values than its 2^capacity_log2 table holds) changes no state, the value tables' free slots
 * included: a value the batch was the first to name is absent afterwards and counts against no rule's capacity. */
int sg_param_decide_batch(sg_handle* h, const sg_param_req* req, uint64_t n, int32_t* pass, void* stream);
int sg_param_decide_batch_host(sg_handle* h, const sg_param_req* req, uint64_t n, int32_t* pass);
/* State of (rule, value): returns flags (bit0 time counter, bit1 token counter; 0 = absent) or < 0. */
int sg_param_read_state(sg_handle* h, uint32_t rule, uint64_t value, int64_t* last_time, int64_t* tokens);
/* Growing the value tables in place (the reference's CacheMaps simply grow). Every sg_*_resize / sg_vdict_grow call:
 *   bit-exact       afterwards the handle decides every batch and answers every state read exactly as a handle that
 *                   had the larger capacity from the start and saw the same history: no time, token, window bucket
 *                   or id moves;
 *   all or nothing  the new tables are allocated and filled beside the old ones and swapped in at the end: when the
 *                   allocation fails the call returns SG_E_NOMEM and the handle is as it was, and so after any other
 *                   refusal;
 *   ordered         enqueued work drains first, as in the rule loads.
 * sg_param_resize: capacity_log2[n], one entry per loaded rule (n = the loaded rule count; the tables of sg_param_*,
 * sg_pslot_* and the slot chain): 0 keeps the rule's size, any other value is the new capacity_log2, at least the
 * current one and at most 30. Every rule is re-inserted, also one whose size is kept, so a call that changes no size
 * compacts: a value whose slot was claimed and never counted (a batch found another table full inside a walker)
 * gives its slot back. SG_E_INVAL: no rules loaded, n differs from the rule count, a size out of range, a shrink.
 * SG_E_UNSUPPORTED: 2^32 slots or more in all, or a total at which a batch's record layout would overflow (slot bits
 * + 8 + the bits of max_batch - 1 above 64 for sg_param_decide_batch; slots above 0xFFFFFFFC with sg_pslot_load_rules
 * in force, the slot chain's 32-bit lookups) — a resize that succeeds never leaves a handle whose next batch is
 * refused for width. The thread-count table is not part of this.
 * sg_param_table_used: counted on the device over rule's sub-table. used = slots whose value word is taken — what a
 * capacity refusal goes by; live = those some walker has counted (flags != 0); capacity = 2^capacity_log2. The side
 * slot of the value 0xFFFF…FFFF is in none of them. Null outputs are skipped. A caller grows when used nears
 * capacity, ahead of the refusal. */
int sg_param_resize(sg_handle* h, const int32_t* capacity_log2, uint32_t n);
int sg_param_table_used(sg_handle* h, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity);
/* Sweeping idle values out of the value tables. The reference's CacheMaps evict, ParameterMetric removes a thread
 * count that reaches 0 and an aged-out ClusterParamMetric bucket holds nothing; here a sweep gives back exactly the
 * entries that no request at or after now_ms can tell from absence (sentinel_amd/csrc/table_sweep.h):
 *   token bucket   both counters present, tokenCount > 0, now_ms - time > durationInSec * 1000 and the refill
 *                  (now_ms - time) * tokenCount / duration + tokens above tokenCount + burstCount, in arithmetic that
 *                  does not wrap: the next request refills to the maximum, as the first sight of a value does;
 *   throttle       (RATE_LIMITER behaviour) never: a recorded time can queue or block a large acquireCount at any
 *                  distance, where a fresh value passes;
 *   cparam ring    every written bucket has now_ms - start > windowIntervalMs (LeapArray.isWindowDeprecated);
 *   thread count   0 (sg_param_sweep only, with sg_pslot_load_rules in force).
 * A value whose slot was claimed and never counted goes too, as in a resize. The side slot of the value 0xFFFF…FFFF
 * is cleared when idle; it is in none of the counts, as it is in none of sg_*_table_used.
 *   ordered and all or nothing   enqueued work drains first; fresh tables of the same size are filled beside the ones
 *                  in force and swapped in at the end, so SG_E_NOMEM and every other refusal leave the handle as it was
 *                  (a device failure, SG_E_DEVICE, leaves the tables as they were and may leave some of the last
 *                  timestamps below raised to now_ms, which only refuses more);
 *   time order     now_ms must not lie before the last timestamp of any path that reads the swept tables (the param
 *                  tables: sg_param_*, sg_pslot_* and the slot chain; the cluster param tables: sg_cparam_* and the
 *                  slot chain's embedded token server), else SG_E_TIME and nothing is swept. After a sweep each of
 *                  those last timestamps is max(itself, now_ms): a later batch that starts before now_ms is refused
 *                  as any out-of-order batch is. Without this the equivalence could break silently;
 *   arguments      SG_E_INVAL with no rules loaded; a null `out` is allowed;
 *   afterwards     every later batch decides exactly as on a handle that was never swept; sg_cparam_read_sum,
 *                  sg_cparam_top_values and sg_pslot_thread_count for now >= now_ms are unchanged. The one visible
 *                  difference: sg_param_read_state of a removed value answers 0 (absent). sg_*_table_used's `used`
 *                  drops by values_removed + claims_dropped. Capacities, rule indices, dictionary ids and the value
 *                  dictionary are untouched. */
typedef struct sg_sweep_stats {
    uint64_t values_removed;   /* idle entries given back                          */
    uint64_t claims_dropped;   /* claimed, never counted (what a resize also drops) */
    uint64_t threads_removed;  /* thread-count entries at 0 (sg_param_sweep only)   */
    uint64_t values_kept;
} sg_sweep_stats;
int sg_param_sweep(sg_handle* h, int64_t now_ms, sg_sweep_stats* out);   /* PSlot tables + thread counts */
int sg_cparam_sweep(sg_handle* h, int64_t now_ms, sg_sweep_stats* out);

/* ---- pace controller ----
 *   sg_pace_load_rules    ← FlowRuleUtil.generateRater for CONTROL_BEHAVIOR_RATE_LIMITER rules
 *                           (core/.../flow/FlowRuleUtil.java:132-145): fresh controllers, latestPassedTime -1.
 *   sg_pace_decide_batch  ← RateLimiterController.canPass (RateLimiterController.java:46-91) for a
 *                           time-ordered batch; wait[i] = SG_PACE_BLOCKED or the sleep in ms (the caller
 *                           sleeps; the reference sleeps inside canPass). req/wait are DEVICE pointers.
 *   sg_pace_read_state    ← latestPassedTime.get() of a rule's controller. */
int sg_pace_load_rules(sg_handle* h, const sg_pace_rule* rules, uint32_t n);
int sg_pace_decide_batch(sg_handle* h, const sg_pace_req* req, uint64_t n, int32_t* wait, void* stream);
int sg_pace_decide_batch_host(sg_handle* h, const sg_pace_req* req, uint64_t n, int32_t* wait);
int sg_pace_read_state(sg_handle* h, uint32_t rule, int64_t* latest_passed_time);

/* ---- cluster hot-parameter tokens ----
 *   sg_cparam_load_rules    ← ClusterParamFlowRuleManager.loadRules → applyClusterParamRules
 *                             (…/flow/rule/ClusterParamFlowRuleManager.java:337-360): a surviving flowId keeps its
 *                             ClusterParamMetric; each rule owns an exact 2^capacity_log2 value table (0 = 2^16).
 *   sg_cparam_decide_batch  ← TokenService.requestParamToken(Long, int, Collection<Object>)
 *                             (DefaultTokenService.java:53-64 → ClusterParamFlowChecker.acquireClusterToken,
 *                             ClusterParamFlowChecker.java:42-87), time-ordered; values[] holds every request's
 *                             parameter values (u64; other types through the shim's value dictionary). Request i's
 *                             values are values[value_begin, value_begin + value_count): the ranges of the valid
 *                             requests must not overlap and must follow request order (value_begin increasing with
 *                             i, as a packer appending each request's values produces) — else SG_E_INVAL.
 *                             allowProceed goes through the namespace's QPS limiter, the same state the flow-token
 *                             path uses (GlobalRequestLimiter is per namespace): keep flow and param batches that
 *                             share a limiter in time order. A rejected batch changes no state, the value tables'
 *                             free slots included: a value the batch was the first to name is absent afterwards
 *                             and counts against no rule's capacity (SG_E_CAPACITY: a rule met more distinct
 *                             values than its table holds). A batch wrong in several ways reports what is wrong
 *                             with the batch itself before what the tables could not take of it: SG_E_TIME, then
 *                             SG_E_INVAL (value ranges), then SG_E_UNSUPPORTED (more than 65536 window periods),
 *                             then SG_E_CAPACITY (it comes last for sg_param_* and sg_slot_* batches too). The slots
 *                             go back by rebuilding the tables from a scratch copy; with no device memory for the
 *                             copy the call still returns the batch's own code and only the free slots stay
 *                             taken (until a later refusal rebuilds, or a reload).
 *   sg_cparam_last_rounds   fixed-point rounds the last batch needed (1 = single pass; requests with several values
 *                           may need more; max_rounds + 1 = it was decided serially). Tuning / tests.
 *   sg_cparam_read_sum      ← ClusterParamMetric.getSum(value) at now_ms (without currentWindow's side effect). */
int sg_cparam_load_rules(sg_handle* h, const sg_cparam_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                         uint32_t n_hot, int32_t capacity_log2);
int sg_cparam_decide_batch(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                           uint64_t n_values, sg_result* out, void* stream);
int sg_cparam_decide_batch_host(sg_handle* h, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                                uint64_t n_values, sg_result* out);
int sg_cparam_read_sum(sg_handle* h, uint32_t rule, uint64_t value, int64_t now_ms, int64_t* sum);
int sg_cparam_last_rounds(const sg_handle* h, uint32_t* rounds);
/*   sg_cparam_top_values ← ClusterParamMetric.getTopValues(number) (…/metric/ClusterParamMetric.java:90-133), the
 *                          topParams of ClusterMetricNodeGenerator.paramToMetricNode (:88-104): per rule up to
 *                          `number` values with the largest window sums at now_ms (count / intervalSec), zero sums
 *                          excluded; ties by ascending value (the reference's order among equal counts is HashMap
 *                          order). values / qps: n_rules * number entries, HOST memory; counts[r] = entries of rule
 *                          r. Without currentWindow's side effect. Like sg_cparam_read_sum, exact for now_ms at or
 *                          after the latest decided request (the metricList task's current time): the device keeps a
 *                          ring per (rule, value), which equals the reference's bucket maps from that time on. */
int sg_cparam_top_values(sg_handle* h, int64_t now_ms, uint32_t number, uint64_t* values, double* qps, uint32_t* counts);
/*   sg_cparam_resize     the (rule, value) tables grown in place, under the contract of sg_param_resize (bit-exact, all
 *                          or nothing, ordered): one capacity_log2 for all rules, at least the current one and at most
 *                          28 (SG_E_INVAL otherwise, or with no rules loaded). Keys and rings of every value with a
 *                          written bucket move to their slot under the new mask; a value with none is dropped, as by a
 *                          refused batch's rebuild. SG_E_UNSUPPORTED, nothing changed: 2^32 slots or more, or a
 *                          total whose value records no longer fit max_batch ids. The embedded token server of the slot
 *                          chain sees the new tables. A later sg_cparam_load_rules keeps surviving flowIds when it
 *                          names the new capacity; any other capacity stays SG_E_UNSUPPORTED.
 *   sg_cparam_table_used used = slots of rule's sub-table that hold a value, live = those with at least one written
 *                          bucket, capacity = 2^capacity_log2; the side slot is in none. */
int sg_cparam_resize(sg_handle* h, int32_t capacity_log2);
int sg_cparam_table_used(sg_handle* h, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity);

/* ---- local slot chain (the ProcessorSlot chain's statistic / flow / degrade slots, batched) ----
 *   sg_local_load_rules    ← FlowRuleManager.loadRules + DegradeRuleManager.loadRules for one resource each
 *                            (one DefaultController QPS/thread rule per resource, limitApp "default",
 *                            DIRECT strategy; up to two circuit breakers), with fresh StatisticNodes.
 *                            A degrade rule that isValidRule drops (see sg_degrade_rule) is refused with
 *                            SG_E_INVAL and the rules loaded before stay in force: the caller filters, as
 *                            DegradeRuleManager does, before it sends.
 *   sg_local_decide_batch  ← SphU.entry(resource, count, prioritized) → StatisticSlot.entry around
 *                            FlowSlot.checkFlow (DefaultController.canPass, DefaultController.java:49-76) and
 *                            DegradeSlot.performChecking (DegradeSlot.java:43-81); Entry.exit() →
 *                            StatisticSlot.exit (StatisticSlot.java:124-165) + DegradeSlot.exit →
 *                            onRequestComplete. Events in (timestamp, arrival) order; exits only for entries
 *                            that passed (the caller holds no Entry for a blocked one).
 * Event/result types: sg_local_event / sg_local_result above. */
int sg_local_load_rules(sg_handle* h, const sg_local_config* cfg, const sg_local_rule* rules, uint32_t n);
int sg_local_decide_batch(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out, void* stream);
int sg_local_decide_batch_host(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out);
/* sg_local_decide_batch on the device pipeline (DEVICE buffers, like sg_flow_enqueue): enqueues the batch and
 * returns at once with a ticket for sg_local_poll / sg_local_wait (same meaning as sg_flow_poll / _wait; tickets
 * are shared with the flow pipeline). The front half of batch i+1 (validation, sort by resource, segment and exit
 * lists) runs beside the walkers of batch i; the walkers run in enqueue order, so batches must be time-ordered as
 * for sg_local_decide_batch, and a batch older than the one before is rejected as a whole (checked before its
 * walkers). ev/out must stay allocated and untouched until the ticket completes (each batch in flight needs its
 * own out buffer); up to 4 batches in flight. A batch the pipeline does not take — origin or context nodes tracked,
 * the embedded token server, or rules loaded since the last batch — first completes the batches in flight and is
 * decided synchronously (its status still comes with its ticket). Every other call on the handle first completes
 * the batches in flight. */
int sg_local_enqueue(sg_handle* h, const sg_local_event* ev, uint64_t n, sg_local_result* out, uint64_t* ticket);
int sg_local_poll(sg_handle* h, uint64_t ticket);
int sg_local_wait(sg_handle* h, uint64_t ticket);
/* Resource state: second window [S][8] {start, PASS, BLOCK, EXCEPTION, SUCCESS, RT, OCCUPIED_PASS, minRt},
 * borrow array [S][2] {start, PASS}, minute window [60][8] (start INT64_MIN = never created; counters of
 * such slots read 0), head[14] = {curThreadNum, then per breaker: state, nextRetry, stat start, slow/error
 * count, total count, 0}. */
int sg_local_read_state(sg_handle* h, uint32_t res, int64_t* second, int64_t* borrow, int64_t* minute, int64_t* head);
/*   sg_local_load_flow_rules ← FlowRuleManager.loadRules (FlowRuleManager.java, FlowRuleUtil.buildFlowRuleMap
 *                              :83-130): replaces every resource's flow rules. Invalid rules are ignored as the
 *                              reference ignores them (FlowRuleUtil.isValidRule :167-251), duplicates are dropped
 *                              (its HashSet), and each resource's rules are stably sorted by FlowRuleComparator
 *                              (FlowRuleComparator.java:30-55: local rules before cluster-mode ones, specific /
 *                              other limitApps before "default"). Fresh controllers (warm-up tokens 0,
 *                              latestPassedTime -1); resource statistics are kept. Returns the number of rules kept
 *                              (>= 0) or an error.
 *                              n_origins: the largest origin id events may carry; n_contexts: context ids events may
 *                              carry are 0 .. n_contexts - 1 (sg_slot_ext.context; 0 when no ext). Origin and context
 *                              ids are the caller's dense ids of the Context origin / name strings and must keep
 *                              their meaning across loads (neither count may shrink).
 *                              Nodes besides the ClusterNodes, created at the first event that needs them whatever
 *                              the rules say, as the reference does, and kept for the life of the resources (rule
 *                              reloads keep them): every event from an origin (id > 0) updates the resource's origin
 *                              StatisticNode (ClusterBuilderSlot.java:99-102 → ClusterNode.getOrCreateOriginNode), and,
 *                              with context tracking on (n_contexts >= 1), every event updates the resource's DefaultNode
 *                              of its context (NodeSelectorSlot.java:156-170). Nodes live in a device pool that grows
 *                              with the (resource, origin / context) pairs seen. Context tracking (needed by CHAIN rules,
 *                              whose context ids must be < n_contexts) starts before the first batch: raising n_contexts
 *                              from 0 after a batch is SG_E_UNSUPPORTED (the DefaultNodes would miss earlier entries).
 *                              With it, every resource is walked by the full-chain walker. A RELATE rule joins its
 *                              resource and ref_resource into one key group walked in event order (the read of
 *                              another resource's ClusterNode, FlowRuleChecker.selectReferenceNode :96-112); a
 *                              resource never entered has no ClusterNode yet (ClusterBuilderSlot), and the rule
 *                              then passes.
 *   sg_local_read_origin_state  ← that origin node: same layout as sg_local_read_state (head[0] = curThreadNum);
 *                              returns 1 when the node exists, 0 when no event created it yet (the dumps of an empty
 *                              node).
 *   sg_local_read_context_state ← the DefaultNode of (resource, context): same layout and return values.
 *   sg_local_read_controller   ← the controller of input rule i: {storedTokens, lastFilledTime, latestPassedTime};
 *                              SG_E_INVAL for an ignored rule. */
int sg_local_load_flow_rules(sg_handle* h, const sg_local_flow_rule* rules, uint32_t n, int32_t n_origins,
                             int32_t n_contexts);

/* ---- AuthoritySlot: origin black and white lists ----
 *   sg_local_load_authority_rules ← AuthorityRuleManager.loadRules (loadAuthorityConf, AuthorityRuleManager.java
 *     :108-139): replaces every authority rule (n == 0 clears them). Rules are taken in array order; a rule with
 *     strategy < 0 or no limitApp item is invalid and ignored (isValidRule :147-150), and the first valid rule of a
 *     resource wins: later ones are ignored as the reference ignores "redundant" rules. Returns the number of rules
 *     kept (>= 0) or an error; a failed load leaves the previous rules in force. Statistics, nodes, flow controllers
 *     and param tables are kept. sg_local_load_rules (fresh resources) drops the authority rules as it drops the
 *     flow rules.
 *     The check (AuthorityRuleChecker.passCheck, AuthorityRuleChecker.java:30-65) per entry: an entry without origin
 *     (origin 0) passes; SG_AUTHORITY_BLACK blocks an origin that equals one of the rule's items, SG_AUTHORITY_WHITE
 *     one that equals none; any other strategy >= 0 never blocks but still holds the resource's single rule.
 *     origins[] holds the limitApp items as the caller's origin ids: any id >= 1, an id above the handle's origin
 *     count simply never matches (the id a shim gives a limitApp item that is not in its origin dictionary: a white
 *     list of unknown names still blocks every origin). An id <= 0, a range outside origins[0 .. n_origin_ids) or a
 *     resource index >= the resource count is SG_E_INVAL, as is a call before sg_local_load_rules. n_origins: as in
 *     sg_local_load_flow_rules; the handle's origin count becomes the larger of the two and never shrinks.
 *     AuthoritySlot (@Spi order -6000, AuthoritySlot.java:39-43) runs after ClusterBuilderSlot and before
 *     ParamFlowSlot, FlowSlot and DegradeSlot: a rejected entry (SG_LOCAL_BLOCK_AUTHORITY, wait_ms 0, whatever its
 *     prioritized flag) has created the resource's ClusterNode, its origin node and its context's DefaultNode and
 *     adds BLOCK to them (StatisticSlot.java:96-116), and reaches nothing else: no param metric, token or thread
 *     count, no flow controller (warm-up sync, latestPassedTime, occupied window), no token of the embedded server,
 *     no breaker. It raises no thread count and has no exit event. */
#define SG_AUTHORITY_WHITE 0
#define SG_AUTHORITY_BLACK 1
#define SG_LOCAL_BLOCK_AUTHORITY 5   /* AuthorityException; wait_ms 0 */
typedef struct sg_authority_rule {
    uint32_t resource;      /* resource index (sg_local_load_rules order)                      */
    int32_t  strategy;      /* RuleConstant.AUTHORITY_*; < 0: invalid, ignored                 */
    uint32_t origin_begin;  /* the limitApp items: origins[origin_begin .. + origin_count)     */
    uint32_t origin_count;  /* 0: blank limitApp, invalid, ignored                             */
} sg_authority_rule;
int sg_local_load_authority_rules(sg_handle* h, const sg_authority_rule* rules, uint32_t n, const int32_t* origins,
                                  uint32_t n_origin_ids, int32_t n_origins);

/* ---- SystemSlot: system rules over Constants.ENTRY_NODE ----
 *   sg_local_load_system_rules ← SystemRuleManager.loadRules (SystemPropertyListener.configUpdate and loadSystemConf,
 *     SystemRuleManager.java:183-282): the defaults are restored, then every rule in array order lowers the threshold of
 *     each field that is >= 0 (the minimum wins; highest_cpu_usage > 1 is ignored), and every rule SETS
 *     checkSystemStatus: the last rule decides it — a list whose last rule sets nothing switches checking off although
 *     earlier thresholds were stored — and an empty list switches it off. Returns checkSystemStatus (0 / 1) or an
 *     error.
 *     The first call starts ENTRY_NODE tracking on the handle: a second window [S] in the handle's sample_count /
 *     interval_ms plus curThreadNum, updated by every event of an inbound resource (sg_local_set_entry_types) as
 *     StatisticSlot does (StatisticSlot.java:71-75, 88-91, 106-109, 139-141): PASS adds the count and a thread, a
 *     PriorityWaitException a thread only, any BlockException (authority and system included) BLOCK; an exit adds
 *     SUCCESS, RT = ts - create_ts, minRt, takes a thread, and EXCEPTION when it carries an error. That first call must
 *     come after sg_local_load_rules and before the first local batch (SG_E_UNSUPPORTED later: the node would miss
 *     the earlier entries — as n_contexts). sg_local_load_rules (fresh resources) drops the rules, the
 *     ENTRY_NODE and the tracking. A handle that never calls it launches no kernel of this section.
 *     The check (checkSystem :290-340) runs, with checking on, for every inbound entry AuthoritySlot did not reject,
 *     before ParamFlowSlot, in this order: passQps + count > qps; curThreadNum > maxThread; avgRt > maxRt; load set and
 *     load > highestSystemLoad and curThread > 1 and curThread > maxSuccessQps * minRt / 1000; cpu set and cpu >
 *     highestCpuUsage. A blocked entry returns {SG_LOCAL_BLOCK_SYSTEM, wait_ms = SG_SYSTEM_*} whatever its prioritized
 *     flag; like an authority-rejected entry it adds BLOCK to its ClusterNode, origin node and DefaultNode (and to
 *     ENTRY_NODE) and reaches nothing else.
 *     Each batch first runs a scan that tries to prove that no entry of it can block (sg_local_system_last_path = 1):
 *     such a batch keeps the parallel walkers and ENTRY_NODE is updated from its results afterwards. Any other batch
 *     with checking on walks every inbound resource in event order on one lane (= 2; env SG_SYS_SERIAL=1 forces
 *     this). Both leave the same results and state. A sharded handle (sg_set_shard, world > 1) with tracking on
 *     refuses local batches (SG_E_UNSUPPORTED): ENTRY_NODE spans the shards; the node handle has no system rules.
 *   sg_local_set_system_status ← SystemStatusListener's system load average and CPU usage (both -1 until set).
 *   sg_local_read_entry_node   ← ENTRY_NODE's second window ([S][8], layout of sg_local_read_state) and curThreadNum;
 *     SG_E_INVAL without tracking.
 *   sg_local_system_last_path  ← the last local batch: 0 tracking off (or no batch), 1 proven clear, 2 serial. */
typedef struct sg_system_rule {   /* SystemRule.java; every field -1 = not set (its defaults) */
    double  highest_system_load, highest_cpu_usage, qps;
    int64_t avg_rt, max_thread;
} sg_system_rule;
#define SG_LOCAL_BLOCK_SYSTEM 6   /* SystemBlockException; wait_ms = the limit type below */
#define SG_SYSTEM_QPS    0        /* "qps"    */
#define SG_SYSTEM_THREAD 1        /* "thread" */
#define SG_SYSTEM_RT     2        /* "rt"     */
#define SG_SYSTEM_LOAD   3        /* "load"   */
#define SG_SYSTEM_CPU    4        /* "cpu"    */
int sg_local_load_system_rules(sg_handle* h, const sg_system_rule* rules, uint32_t n);
int sg_local_set_system_status(sg_handle* h, double load, double cpu_usage);
int sg_local_read_entry_node(sg_handle* h, int64_t* second, int64_t* cur_thread_num);
int sg_local_system_last_path(const sg_handle* h, uint32_t* path);
/* The index of the first entry the last scan could not prove clear (0xFFFFFFFF: none, or no scan ran). */
int sg_local_system_first_unproven(const sg_handle* h, uint32_t* index);

/* ---- the whole slot chain in one batch (the ProcessorSlot chain's SPI order, Constants.java:76-83 and
 * ParamFlowSlot @Spi(order = -3000)): StatisticSlot.entry around AuthoritySlot → SystemSlot → ParamFlowSlot →
 * FlowSlot → DegradeSlot. SystemSlot reads Constants.ENTRY_NODE, which depends on every earlier decision of every
 * inbound resource: with system rules loaded (above) a batch is first proven clear of system blocks from its arrivals
 * and exits alone, or else walks its inbound resources in event order.
 *   sg_slot_decide_batch ← SphU.entry(resource, count, prioritized, args...) / Entry.exit(count, args...) for a
 *     time-ordered batch. Per entry: AuthoritySlot (the authority rules above; an AuthorityException ends the chain
 *     before any other slot, SG_LOCAL_BLOCK_AUTHORITY); ParamFlowSlot.checkFlow (the param rules sg_pslot_load_rules loaded for the
 *     resource, args of the event; args_null or no rules: nothing) — a ParamFlowException ends the chain
 *     (SG_LOCAL_BLOCK_PARAM, wait_ms = the index of the param rule that threw); FlowSlot (the flow rules above);
 *     DegradeSlot; then StatisticSlot (StatisticSlot.java:55-122): a pass raises curThreadNum and PASS on the
 *     ClusterNode, the origin node and the DefaultNode and runs ParamFlowStatisticEntryCallback.onPass (the param
 *     thread counts of the args, ParameterMetric.addThreadCount); a PriorityWaitException raises the thread counts
 *     and runs onPass; any BlockException — ParamFlowException included — adds BLOCK to those nodes. Exit
 *     (StatisticSlot.exit :124-165, passed entries only): RT / success / exception and curThreadNum on the nodes,
 *     ParamFlowStatisticExitCallback (decreaseThreadCount of the exit's args), DegradeSlot.exit.
 *     ext[i] (nullable: every event in context 0 with null args) carries the event's context and arguments; args,
 *     values and ext are DEVICE pointers like ev and out. sg_local_decide_batch = this call with ext = NULL.
 *     A batch rejected from its events alone (SG_E_TIME, SG_E_INVAL, SG_E_UNSUPPORTED) changes no state, the param
 *     value tables' free slots included: a value only its entries named is absent afterwards and counts against no
 *     rule's capacity. A table found full while the batch is walked (an entry with a collection argument or of a
 *     resource with several param rules, the thread counts, the embedded token server's cluster param values) is
 *     SG_E_CAPACITY and can leave the batch partly applied: the statistics then hold the events decided up to
 *     there, and the last timestamp does not advance. */
typedef struct sg_slot_ext {
    uint32_t context;             /* Context name id (0 .. n_contexts - 1); CHAIN rules select by it              */
    uint32_t arg_begin;           /* the event's args: args[arg_begin .. + arg_count)                           */
    uint32_t arg_count;
    int32_t  args_null;           /* 1: Object[] args is null (ParamFlowSlot.checkFlow returns at once)          */
} sg_slot_ext;
#define SG_LOCAL_BLOCK_PARAM   4  /* ParamFlowException (result wait_ms: the index of the param rule that threw) */
int sg_slot_decide_batch(sg_handle* h, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                         const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                         sg_local_result* out, void* stream);
int sg_slot_decide_batch_host(sg_handle* h, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                              const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                              sg_local_result* out);
int sg_local_read_context_state(sg_handle* h, uint32_t res, int32_t context, int64_t* second, int64_t* borrow,
                                int64_t* minute, int64_t* head);

/* ---- metric snapshots ----
 *   sg_local_metrics ← MetricTimerListener.run (core/.../node/metric/MetricTimerListener.java:40-69) over every
 *                      resource's ClusterNode: StatisticNode.metrics() (StatisticNode.java:116-133) at now_ms — the
 *                      minute window's buckets (ArrayMetric.details, :156-204, with currentWindow's side effect) newer
 *                      than the node's lastFetchTime and older than now's second, non-empty; lastFetchTime advances.
 *                      Rows sorted by (timestamp, resource) into HOST memory; *n_rows = the number of rows (with
 *                      SG_E_CAPACITY and no side effect when cap is too small). The host formats them as metrics.log
 *                      lines (MetricNode.toFatString, MetricNode.java:213-229; sentinel_amd/metrics.py). After
 *                      the resources, Constants.ENTRY_NODE (__total_inbound_traffic__, MetricTimerListener.java:46):
 *                      rows with resource = SG_ENTRY_NODE_RESOURCE, the sums of the inbound resources' buckets of each
 *                      second (StatisticSlot adds every EntryType.IN entry / exit to it, StatisticSlot.java:71-75,
 *                      :139-141) less their occupied passes (StatisticNode.addOccupiedPass raises only the selected
 *                      node's PASS, StatisticNode.java:333-336), occupied_pass_qps 0, with the ENTRY_NODE's own
 *                      lastFetchTime. Exact when rows are fetched at least once a minute and at a time not behind the
 *                      latest decided event, as MetricTimerListener does (a resource's bucket of a second outlives
 *                      the ENTRY_NODE's by up to the minute window).
 *   sg_local_set_entry_types ← the EntryType of each resource's SphU.entry calls (1 = IN; default OUT, as
 *                      SphU.entry(name)). */
#define SG_ENTRY_NODE_RESOURCE 0xFFFFFFFFu
typedef struct sg_metric_node {
    int64_t  timestamp;
    int64_t  pass_qps, block_qps, success_qps, exception_qps;
    int64_t  rt;                  /* rt / success when success != 0, else the raw rt sum (ArrayMetric.fromBucket) */
    int64_t  occupied_pass_qps;
    uint32_t resource;
    int32_t  concurrency;         /* 0, as fromBucket leaves it */
} sg_metric_node;
int sg_local_metrics(sg_handle* h, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows);
/* sg_local_metrics with `rt` as the bucket's raw sum in every row (not divided by success): one GPU's share of a node's
 * rows, which the node's rollup merges (sentinel_amd/cluster.py LocalMetricRollup: the ENTRY_NODE rows of the same
 * second are summed over the GPUs, then rt = Σrt / Σsuccess), with the same side effects as sg_local_metrics. */
int sg_local_metrics_raw(sg_handle* h, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows);
/* sg_local_metrics_raw into DEVICE memory (d_out on the handle's device), rows unsorted, complete on return: the
 * node's device rollup (cluster.DeviceLocalMetricRollup: RCCL all_gather of the rows, ENTRY_NODE sums and the
 * (timestamp, resource) order on the GPU). Same side effects, same SG_E_CAPACITY contract. */
int sg_local_metrics_raw_device(sg_handle* h, int64_t now_ms, sg_metric_node* d_out, uint64_t cap, uint64_t* n_rows);
/* sg_local_metrics_raw_device enqueued, no host wait: the rows of now_ms after every local batch enqueued so far
 * (sg_local_enqueue) and after the caller's earlier work on `stream`, before every batch enqueued later; `stream` is
 * made to wait for them. *d_count (DEVICE memory) receives the row count; when it exceeds cap, no row is written and
 * nothing changes (the listener's state included). A cap of at least 59 rows per resource + 60 skips the counting
 * pass. Rows unsorted, as sg_local_metrics_raw_device. */
int sg_local_metrics_raw_enqueue(sg_handle* h, int64_t now_ms, sg_metric_node* d_out, uint64_t cap, uint64_t* d_count,
                                 void* stream);
/* The local chain sharded over a node's GPUs (one process per GPU): every GPU loads the same rules and
 * decides the entries and exits of the resources it owns — owner[r] = splitmix64(g(r)) mod world, g(r) the smallest
 * resource of r's key group (RELATE references; on an embedded token server also the resources sharing a flowId or
 * a limited namespace), so every state a decision reads (ClusterNode, origin and context nodes, breakers, flow
 * controllers, param tables) lives on one GPU. The caller routes each event to owner[event.resource] in arrival order;
 * the per-GPU metric rows merge by sg_local_metrics_raw. SG_E_UNSUPPORTED: an embedded token server with namespace
 * limiters (its GlobalRequestLimiter sees the whole node). Replaces nothing in the reference (one JVM, one chain):
 * the node-level deployment of StatisticSlot / FlowSlot / DegradeSlot. */
int sg_local_owners(sg_handle* h, uint32_t world, uint32_t* owner, uint32_t n);
int sg_local_set_entry_types(sg_handle* h, const uint8_t* inbound, uint32_t n);
int sg_local_read_origin_state(sg_handle* h, uint32_t res, int32_t origin, int64_t* second, int64_t* borrow,
                               int64_t* minute, int64_t* head);
int sg_local_read_controller(sg_handle* h, uint32_t rule, int64_t* state3);

/* ---- LogSlot: sentinel-block.log (core/slots/logger/LogSlot.java:35-47, EagleEyeLogUtil.java:31-45) ----
 * LogSlot.entry catches every BlockException of the slots behind it and calls statLogger.stat(resource,
 * exception class, e.getRuleLimitApp(), context origin).count(count): a per-second rollup (StatLogger /
 * StatRollingData, time slot t - t % 1000) with one COUNT_SUM entry per key, written as one line per entry
 * `time|1|resource,ExceptionName,ruleLimitApp,origin|count,0` (StatLogWriteTask.run). PriorityWaitException and exits
 * never reach it. The device keeps that rollup across batches in an exact table in device memory and hands out rows.
 *   sg_local_block_log_enable ← the StatLogger's creation: a table of 2^capacity_log2 rows (4..24), and every local
 *     batch decided from then on (sg_local_decide_batch, sg_slot_decide_batch, their _host forms, sg_local_enqueue) adds
 *     its blocked entries behind its walkers. Allowed at any time, before or after the rules and the first batches
 *     (rows record only what was decided after it); a second call with the same capacity does nothing, with another
 *     SG_E_INVAL. The table outlives every rule reload (pending rows keep the caller's ids). A handle that never calls
 *     it runs exactly the kernels it ran before.
 *   sg_local_block_log ← the rolling task (StatLogWriteTask) at now_ms: every row whose second is complete
 *     (timestamp + 1000 <= now_ms - now_ms % 1000) into HOST memory, sorted by (timestamp, resource, status, app_kind,
 *     app, origin), and removed from the table. cap too small: SG_E_CAPACITY, *n_rows = the rows needed, nothing
 *     changes (the lost totals included). now_ms may lie behind the latest decided event: only complete seconds leave.
 *     SG_E_INVAL before sg_local_block_log_enable. A blocked entry whose key found no free row is not logged and never
 *     changes a decision: it is counted in *lost_events and its count in *lost_count, reported by the next successful
 *     call and cleared by it. One row per key and second (the reference's maxEntryCount = 6000 rolls the map early,
 *     so a key can have several lines in a second: summed per key and second they equal the row).
 * ruleLimitApp by class (app_kind says how to read app):
 *   FlowException     SG_BLOCK_APP_LIMIT_APP  limit_app of the rule that failed (int32 in the low word:
 *                                             SG_LIMIT_APP_DEFAULT, SG_LIMIT_APP_OTHER or an origin id)
 *   DegradeException  SG_BLOCK_APP_LIMIT_APP  always SG_LIMIT_APP_DEFAULT: sg_degrade_rule carries no limitApp
 *   AuthorityException SG_BLOCK_APP_ORIGIN    the entry's origin id (0 = "")
 *   SystemBlockException SG_BLOCK_APP_SYSTEM  SG_SYSTEM_* (the two-argument constructor passes the limit type on as
 *                                             ruleLimitApp, SystemBlockException.java)
 *   ParamFlowException (ParamFlowSlot.java:81-91: String.valueOf(args[rule.getParamIdx()]) after applyRealParamIdx)
 *                     SG_BLOCK_APP_VALUE      a scalar argument's value id
 *                     SG_BLOCK_APP_NULL_ARG   a null argument: "null"
 *                     SG_BLOCK_APP_NO_ARG     args.length <= paramIdx: ""
 *                     SG_BLOCK_APP_LABEL      a collection / array argument: sg_pslot_arg.reserved, the caller's id of
 *                                             the collection's String.valueOf (0 = unlabelled) */
#define SG_BLOCK_APP_LIMIT_APP 0
#define SG_BLOCK_APP_ORIGIN    1
#define SG_BLOCK_APP_SYSTEM    2
#define SG_BLOCK_APP_VALUE     3
#define SG_BLOCK_APP_NULL_ARG  4
#define SG_BLOCK_APP_NO_ARG    5
#define SG_BLOCK_APP_LABEL     6
typedef struct sg_block_row {
    int64_t  timestamp;           /* the second: t - t % 1000                                   */
    int64_t  count;               /* sum of the blocked entries' acquireCount                   */
    uint64_t app;                 /* ruleLimitApp, read by app_kind                             */
    uint32_t resource;
    int32_t  origin;              /* Context origin id, 0 = ""                                  */
    int32_t  status;              /* SG_LOCAL_BLOCK_*: the exception class                      */
    int32_t  app_kind;            /* SG_BLOCK_APP_*                                             */
} sg_block_row;
int sg_local_block_log_enable(sg_handle* h, int32_t capacity_log2);
int sg_local_block_log(sg_handle* h, int64_t now_ms, sg_block_row* rows, uint64_t cap, uint64_t* n_rows,
                       uint64_t* lost_events, uint64_t* lost_count);

/* ---- the node handle: one token server over G shard handles (SURVEY §8(b) "multi-GPU fan-out is internal to the
 * handle", §8(e) flowIds hashed over the GPUs) ----
 * The reference serves every flowId from one TokenService (DefaultTokenService.requestToken, DefaultTokenService
 * .java:39-50) for all Netty workers (NettyTransportServer.java:53-54). A node handle owns G shard handles (shard g on
 * devices[g]; one device may hold several shards) and a front handle on devices[0]. A node batch in caller order is
 * validated and passed through the namespace limiters by the front (GlobalRequestLimiter over the whole batch in
 * caller order: the node's arrival order), split by owner — splitmix64(flowId) mod G — with a stable device multisplit,
 * decided by every shard concurrently on its own stream (slices copied peer to peer for shards on other devices),
 * and gathered back into caller order: the results equal one handle deciding the batch.
 *   sg_node_create          ← G shards (1..64) on devices[0..G-1], each with cfg (max_batch per shard and node)
 *   sg_node_set_namespaces  ← sg_set_namespaces (the front keeps the limiters)
 *   sg_node_load_flow_rules ← sg_load_flow_rules for the node's rule set (keys = rule indices of this array);
 *                             a surviving flowId keeps its owner, hence its ClusterMetric
 *   sg_node_flow_decide_batch(_host) ← sg_flow_decide_batch over the node (device buffers on devices[0] / host)
 *   sg_node_flow_enqueue / _poll / _wait ← sg_flow_enqueue / _poll / _wait over the node (pipelined)
 *   sg_node_flow_read_state, sg_node_snapshot_metrics ← per node rule, as the single-handle calls
 *   sg_node_shard_of        owner shard and local rule index of node rule `key` */
typedef struct sg_node sg_node;
int         sg_node_create(const sg_config* cfg, const int32_t* devices, uint32_t n_shards, sg_node** out);
void        sg_node_destroy(sg_node* nd);
const char* sg_node_last_error(const sg_node* nd);
int         sg_node_set_namespaces(sg_node* nd, const sg_namespace* ns, uint32_t n);
int         sg_node_load_flow_rules(sg_node* nd, const sg_flow_rule* rules, uint32_t n);
int         sg_node_flow_decide_batch(sg_node* nd, const sg_req* req, uint64_t n, sg_result* out, void* stream);
int         sg_node_flow_decide_batch_host(sg_node* nd, const sg_req* req, uint64_t n, sg_result* out);
/* sg_flow_enqueue / _poll / _wait over the node (DEVICE buffers on devices[0], same ticket meaning): with every shard
 * on devices[0] the node batches are pipelined — the front's validation, limiter and routing of batch i+1 and the
 * shards' sorts run beside the shards' walkers of batch i, two node workspaces alternating; the host waits only for
 * the front of the batch it enqueues (the slice sizes). Batches must be time-ordered; a batch the front refuses
 * (validation, time order) reaches no shard and its ticket carries the error. With shards on other devices a node
 * batch is decided synchronously and its status kept for the ticket. Every other sg_node_* call first completes
 * the batches in flight. */
int         sg_node_flow_enqueue(sg_node* nd, const sg_req* req, uint64_t n, sg_result* out, uint64_t* ticket);
int         sg_node_flow_poll(sg_node* nd, uint64_t ticket);
int         sg_node_flow_wait(sg_node* nd, uint64_t ticket);
int         sg_node_flow_read_state(sg_node* nd, uint32_t key, int64_t* starts, int64_t* counters, int64_t* occupy);
int         sg_node_snapshot_metrics(sg_node* nd, int64_t now_ms, double* out, uint64_t cap);
int         sg_node_shard_of(const sg_node* nd, uint32_t key, uint32_t* shard, uint32_t* local_key);
/* The node's front handle (devices[0]; owned by the node, not to be destroyed): it holds the namespace limiters, so
 * cluster param tokens whose rules sit under an enabled GlobalRequestLimiter (ClusterParamFlowChecker.java:43-45
 * shares the limiter in caller order) are decided on it with sg_cparam_*; every other param and concurrent token
 * goes through the sharded sg_node_cparam_* / sg_node_conc_* below. Its own sg_flow_* entry points must not be
 * called. */
sg_handle*  sg_node_front(sg_node* nd);
/* Cluster param and concurrent tokens sharded over the node (DefaultTokenService.requestParamToken /
 * requestConcurrentToken / releaseConcurrentToken, DefaultTokenService.java:53-85): a param rule (with its hot items)
 * lives on the shard owning its flowId; a concurrent acquire goes to the owner of its flow rule's flowId, a release
 * to the shard its token id names (node token id = (shard token id - 1) * G + shard + 1). A node batch in caller order
 * is checked for time order and the value-range contract of sg_cparam_decide_batch over the whole batch (the valid
 * requests' ranges inside the value array, in request order, not overlapping) on devices[0] (refused whole, nothing
 * decided), split stably by owner
 * with one 8-bit radix pass, decided shard by shard in the node's order and gathered back: the statuses, counters and
 * metrics equal one handle deciding the batch; token ids are the node's own (unique, as the reference's are only
 * unique). Param batches whose rules name a namespace with the GlobalRequestLimiter enabled are refused
 * (SG_E_UNSUPPORTED): allowProceed (ClusterParamFlowChecker.java:43-45) takes the limiter in caller order, which the
 * front handle serves (sg_node_front). Device buffers are on devices[0]; the _host forms take host buffers.
 *   sg_node_cparam_load_rules      ← sg_cparam_load_rules for the node's param rule set (rule = index of this array)
 *   sg_node_cparam_read_sum / _top_values ← per node param rule, as the single-handle calls
 *   sg_node_conc_*                 ← sg_conc_* with node flow rule indices (timeouts per node rule) */
int sg_node_cparam_load_rules(sg_node* nd, const sg_cparam_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                              uint32_t n_hot, int32_t capacity_log2);
int sg_node_cparam_decide_batch(sg_node* nd, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                                uint64_t n_values, sg_result* out, void* stream);
int sg_node_cparam_decide_batch_host(sg_node* nd, const sg_cparam_req* req, uint64_t n, const uint64_t* values,
                                     uint64_t n_values, sg_result* out);
int sg_node_cparam_read_sum(sg_node* nd, uint32_t rule, uint64_t value, int64_t now_ms, int64_t* sum);
int sg_node_cparam_top_values(sg_node* nd, int64_t now_ms, uint32_t number, uint64_t* values, double* qps,
                              uint32_t* counts);
/* sg_cparam_resize on every shard that owns a flowId, in shard order. Each shard's growth is all or nothing; the
 * node's is not: the first refusal is returned with the shards before it grown (which changes no answer; call again
 * to complete — a shard already at the size is rehashed at that size). sg_node_cparam_table_used: the node's rule
 * index, answered by the rule's owner. */
int sg_node_cparam_resize(sg_node* nd, int32_t capacity_log2);
int sg_node_cparam_table_used(sg_node* nd, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity);
int sg_node_conc_set_rule_timeouts(sg_node* nd, const int64_t* client_offline_ms, const int64_t* resource_timeout_ms,
                                   uint32_t n);
int sg_node_conc_decide_batch(sg_node* nd, const sg_conc_req* req, uint64_t n, sg_conc_result* out, void* stream);
int sg_node_conc_decide_batch_host(sg_node* nd, const sg_conc_req* req, uint64_t n, sg_conc_result* out);
int sg_node_conc_expire(sg_node* nd, int64_t now_ms, const uint8_t* client_online, uint32_t n_clients, uint64_t* removed);
int sg_node_conc_read_state(sg_node* nd, uint32_t key, int32_t* now_calls, uint64_t* live_tokens);
/* The local slot chain over the node: StatisticSlot → FlowSlot → DegradeSlot (sg_local_*) for a multi-GPU node from one
 * handle — the sharded deployment described at sg_local_owners, composed inside the library. Every shard loads the whole
 * rule set under the node's resource indices and decides the entries and exits of the resources it owns (a key group on
 * one owner); it never sees events of other resources, whose state stays empty and yields no rows. The front handle
 * carries no local traffic: it is the staging copy of the rules and names the owners. Same conventions as the calls
 * above: 0 or SG_E_*, the message in sg_node_last_error, pipelined node batches completed first, device buffers on
 * devices[0], the shards in SG_CLUSTER_NOT_STARTED.
 *   sg_node_local_load_rules      ← sg_local_load_rules on the front, then on every shard: fresh statistics, so owners
 *                                   may change freely. A shard that fails leaves the local chain unloaded (load again).
 *                                   It also clears the node's param rules (sg_node_pslot_load_rules) on the front and on
 *                                   every shard — a param rule's state lives on its resource's owner, which may move —
 *                                   where one handle's sg_local_load_rules keeps them: load them again after it.
 *   sg_node_local_load_flow_rules ← sg_local_load_flow_rules (returns the rules kept). The resources keep their
 *                                   statistics, which live on their owner, so after the node has decided a local batch no
 *                                   resource may move: rules whose key groups (RELATE references) give any resource
 *                                   another owner are refused with SG_E_UNSUPPORTED. The check runs on the front before
 *                                   any shard is touched (the front goes back to the rules in force); before the first
 *                                   batch every rule set is accepted. n_contexts >= 1 starts before the node's first
 *                                   batch (SG_E_UNSUPPORTED after it). A shard that fails midway (allocation, device)
 *                                   leaves the earlier shards on the new rules: load again.
 *   sg_node_local_load_authority_rules ← sg_local_load_authority_rules on the front (validation: a refused load
 *                                   reaches no shard), then on every shard; returns the rules kept. Routing and owners
 *                                   do not change: a rejected entry is an ordinary event of its resource's owner.
 *   sg_node_local_set_entry_types ← sg_local_set_entry_types on every shard
 *   sg_node_local_owner_of        owner shard of a resource
 *   sg_node_local_decide_batch(_host) ← sg_local_decide_batch over the node, synchronous. Before any shard is touched the
 *                                   node refuses the batch for everything one handle refuses from the events alone, over
 *                                   the whole batch (a slice of an unsorted batch can itself be sorted, and spans less
 *                                   time): timestamps negative, decreasing, or older than the node's previous local batch
 *                                   (SG_E_TIME); origin outside 0..n_origins (SG_E_INVAL); more than 65536 window periods
 *                                   (SG_E_UNSUPPORTED); n > max_batch (SG_E_CAPACITY); null buffers, rules not loaded
 *                                   (SG_E_INVAL). A batch refused so leaves every shard unchanged. The events are then
 *                                   split stably by owner on the device (arrival order kept within a shard; an event
 *                                   whose resource index is not below the resource count goes to shard 0, which answers
 *                                   it as one handle does), every shard with work decides its slice concurrently (peer
 *                                   copies for shards off devices[0]), and the results are gathered into caller order:
 *                                   they equal one handle deciding the batch. A failure inside a shard — SG_E_DEVICE,
 *                                   SG_E_NOMEM (its origin / context node pool cannot grow), SG_E_CAPACITY (a table of
 *                                   its own is full) — is reported after every shard has finished and can leave the
 *                                   other shards' slices applied: the node's statistics then hold part of the batch, and
 *                                   its last timestamp does not advance. The same holds for sg_node_cparam_* and
 *                                   sg_node_conc_* batches, which run their shards the same way.
 *   sg_node_local_read_state      ← sg_local_read_state of the resource on its owner
 *   sg_node_local_metrics(_device) ← MetricTimerListener.run for the node, the final table ordered by (timestamp,
 *                                   resource) as sg_local_metrics gives it (into HOST memory / device memory on
 *                                   devices[0]): the shards' raw rows are counted, laid out one after the other on
 *                                   devices[0] and merged on the device — a resource's rows come from its owner (rt = rt /
 *                                   success when success != 0), the ENTRY_NODE rows of one second are summed over the
 *                                   shards (rt = Σrt / Σsuccess, kept when isValidMetricNode holds for the sums). When the
 *                                   sum of the shards' row counts exceeds cap: SG_E_CAPACITY, *n_rows = that sum (a
 *                                   sufficient capacity: the merged table can only be shorter) and no row is consumed: the
 *                                   same call with that capacity returns the whole table (a shard with no new row has
 *                                   then run its empty fetch, whose one effect is currentWindow(now_ms)).
 *   sg_node_local_merge_rows      the merge alone, on n raw rows (sg_local_metrics_raw_device of every GPU, fetched at one
 *                                   now_ms) in device memory on devices[0]: what a deployment with one process per GPU
 *                                   calls after its all-gather. Contract: timestamps multiples of 1000 less than 60 s
 *                                   apart, one row per (timestamp, resource), resources below the loaded resource count
 *                                   or SG_ENTRY_NODE_RESOURCE — else SG_E_INVAL and d_out untouched. More rows than cap:
 *                                   SG_E_CAPACITY, *n_out = the rows needed, d_out untouched. Runs on `stream` and waits
 *                                   for it.
 *   sg_node_pslot_load_rules      ← sg_pslot_load_rules on the front (validation: a refused load reaches no shard and the
 *                                   front goes back to the rules in force), then on every shard: the whole rule set under
 *                                   the node's rule and resource indices. SG_E_INVAL before sg_node_local_load_rules or
 *                                   when n_resources differs from the node's resource count. Param rules form no key
 *                                   groups on a node that is no embedded server, so no resource changes its owner; a
 *                                   rule's state (token buckets, throttle times, thread counts, a resolved negative
 *                                   paramIdx) lives on the owner of its resource. A flow-rule reload refused by the
 *                                   front leaves the front on these rules too. A shard that fails midway (allocation,
 *                                   device) leaves the earlier shards on the new rules: load again.
 *   sg_node_slot_decide_batch(_host) ← sg_slot_decide_batch over the node, synchronous; sg_node_local_decide_batch is
 *                                   this call with ext = NULL, and the two share the node's last timestamp and batch
 *                                   count. Besides that call's refusals, before any shard is touched: a context >=
 *                                   max(n_contexts, 1), and — with param rules on the node, for an event with args_null
 *                                   == 0 of a resource below the resource count — arg_begin + arg_count > n_args or an
 *                                   argument's value_begin + m > n_values (m: value_count of a COLLECTION, 1 of a VALUE,
 *                                   0 of a null argument; 64-bit sums; a record outside [0, n_args) is never read):
 *                                   SG_E_INVAL. n_args or n_values >= 2^32: SG_E_CAPACITY. Each event's ext record moves
 *                                   with it. A shard on devices[0] reads the caller's args and values in place (ranges
 *                                   may be shared between events and may overlap: nothing is copied, no index changes).
 *                                   A shard on another device gets its slice's own arrays, compacted on devices[0] and
 *                                   peer-copied with the slice: with param rules on the node, every event of the slice
 *                                   with args_null == 0 and a resource below the resource count brings its arg records
 *                                   (value_begin rebased, value_count and kind as given) and their values, at the
 *                                   exclusive scans over slice order, its ext.arg_begin rebased; a range several events
 *                                   share is copied once per event. Without param rules no argument is copied and the
 *                                   shard gets null arrays (one handle never reads them then). An event of a resource
 *                                   not below the resource count goes to shard 0 and is answered as one handle answers
 *                                   it; its argument range is neither validated nor read. A slice whose compacted args
 *                                   or values reach 2^32: SG_E_CAPACITY; a buffer that cannot grow: SG_E_NOMEM — both
 *                                   before any shard runs. Test aid: env SG_NODE_COMPACT_ARGS=1 (read at sg_node_create)
 *                                   compacts for every shard, so one GPU exercises that path. Failures inside a shard:
 *                                   as sg_node_local_decide_batch.
 *   sg_node_local_read_origin_state, sg_node_local_read_context_state, sg_node_local_read_controller,
 *   sg_node_pslot_thread_count, sg_node_pslot_param_idx, sg_node_param_read_state
 *                                 ← the single-handle calls (same arguments, layouts and return values; the node's rule
 *                                   and resource indices) on the owner of the resource, or of the rule's resource.
 * Out of scope here: the embedded token server over the node, a pipelined sg_node_local_enqueue. Cross-device shards
 * are built (peer copies, per-shard buffers) and unmeasured on hardware, as the rest of the node handle. */
int sg_node_local_load_rules(sg_node* nd, const sg_local_config* cfg, const sg_local_rule* rules, uint32_t n);
int sg_node_local_load_flow_rules(sg_node* nd, const sg_local_flow_rule* rules, uint32_t n, int32_t n_origins,
                                  int32_t n_contexts);
int sg_node_local_load_authority_rules(sg_node* nd, const sg_authority_rule* rules, uint32_t n, const int32_t* origins,
                                       uint32_t n_origin_ids, int32_t n_origins);
int sg_node_local_set_entry_types(sg_node* nd, const uint8_t* inbound, uint32_t n);
int sg_node_local_owner_of(const sg_node* nd, uint32_t resource, uint32_t* shard);
int sg_node_local_decide_batch(sg_node* nd, const sg_local_event* ev, uint64_t n, sg_local_result* out, void* stream);
int sg_node_local_decide_batch_host(sg_node* nd, const sg_local_event* ev, uint64_t n, sg_local_result* out);
int sg_node_local_read_state(sg_node* nd, uint32_t res, int64_t* second, int64_t* borrow, int64_t* minute, int64_t* head);
int sg_node_local_metrics(sg_node* nd, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n_rows);
int sg_node_local_metrics_device(sg_node* nd, int64_t now_ms, sg_metric_node* d_out, uint64_t cap, uint64_t* n_rows);
int sg_node_local_merge_rows(sg_node* nd, const sg_metric_node* d_rows, uint64_t n, sg_metric_node* d_out, uint64_t cap,
                             uint64_t* n_out, void* stream);
int sg_node_pslot_load_rules(sg_node* nd, const sg_pslot_rule* rules, uint32_t n, const sg_param_hot_item* hot,
                             uint32_t n_hot, uint32_t n_resources);
int sg_node_slot_decide_batch(sg_node* nd, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                              const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                              sg_local_result* out, void* stream);
int sg_node_slot_decide_batch_host(sg_node* nd, const sg_local_event* ev, const sg_slot_ext* ext, uint64_t n,
                                   const sg_pslot_arg* args, uint64_t n_args, const uint64_t* values, uint64_t n_values,
                                   sg_local_result* out);
int sg_node_local_read_origin_state(sg_node* nd, uint32_t res, int32_t origin, int64_t* second, int64_t* borrow,
                                    int64_t* minute, int64_t* head);
int sg_node_local_read_context_state(sg_node* nd, uint32_t res, int32_t context, int64_t* second, int64_t* borrow,
                                     int64_t* minute, int64_t* head);
int sg_node_local_read_controller(sg_node* nd, uint32_t rule, int64_t* state3);
int sg_node_pslot_thread_count(sg_node* nd, uint32_t resource, int32_t param_idx, uint64_t value, int64_t* count);
int sg_node_pslot_param_idx(sg_node* nd, uint32_t rule, int32_t* param_idx);
int sg_node_param_read_state(sg_node* nd, uint32_t rule, uint64_t value, int64_t* last_time, int64_t* tokens);
/* sg_param_resize over the node (sg_node_pslot_load_rules' rule indices): the front and every shard hold the whole
 * rule set, so the front grows first — it refuses what any shard would, before one has changed — then the shards in
 * order. Not node-wide all or nothing: a shard that fails (SG_E_NOMEM) leaves the front and the shards before it grown,
 * which changes no answer; call again to complete. sg_node_param_table_used is answered by the owner of the rule's
 * resource, where the rule's state lives. */
int sg_node_param_resize(sg_node* nd, const int32_t* capacity_log2, uint32_t n);
int sg_node_param_table_used(sg_node* nd, uint32_t rule, uint64_t* used, uint64_t* live, uint64_t* capacity);
/* sg_param_sweep / sg_cparam_sweep over the node, under their contract with the node's own last timestamps (the
 * node's local batches for the param tables, its param-token batches for the cluster param tables) checked first and
 * raised to max(themselves, now_ms) afterwards. The param sweep takes the front first and then the shards in order,
 * the cluster param sweep every shard that owns a flowId; `out` is summed over the shards. Each handle's sweep is all
 * or nothing; the node's is not — a shard that fails (SG_E_NOMEM) leaves the handles before it swept, which changes
 * no answer (a swept entry is invisible), and the node's last timestamp raised to now_ms as theirs are; call again to
 * complete. */
int sg_node_param_sweep(sg_node* nd, int64_t now_ms, sg_sweep_stats* out);   /* summed over shards */
int sg_node_cparam_sweep(sg_node* nd, int64_t now_ms, sg_sweep_stats* out);

/* ---------- token-server wire codec ----------
 * The default token server frames every message with a 2-byte big-endian length
 * (LengthFieldBasedFrameDecoder(1024, 0, 2, 0, 2) / LengthFieldPrepender(2),
 * srv/server/NettyTransportServer.java:89-92). A request payload is [i32 xid][u8 type][data]
 * (DefaultRequestEntityDecoder.java:36-58); MSG_TYPE_FLOW data is [i64 flowId][i32 count][bool priority?]
 * (FlowRequestDataDecoder.java:31-43). A response frame is [u16 len = 14][i32 xid][u8 type][u8 status]
 * [i32 remaining][i32 waitInMs] (DefaultResponseEntityWriter.java:32-51, FlowResponseDataWriter.java:28-32),
 * all big-endian (Netty ByteBuf). The batching front-end that a Netty handler feeds appends each frame's
 * payload (length prefix stripped) to one buffer and records where it starts.
 *
 * sg_codec_decode_flow: payload bytes + offsets[n + 1] (frame i = [offsets[i], offsets[i+1])) + arrival
 * timestamps → sg_req records for sg_flow_decide_batch (flowId → rule index through the handle's device
 * table: unknown → SG_KEY_NO_RULE, flowId <= 0 → SG_KEY_BAD, as DefaultTokenService.requestToken would
 * answer), the xid of every frame and its kind (SG_FRAME_*). Frames that are not decodable flow requests
 * get key SG_KEY_BAD and acquire 0 (a harmless BAD_REQUEST slot in the batch). All pointers are device
 * memory (payload 4-byte aligned); the call is asynchronous on `stream`. offsets must be non-decreasing and
 * offsets[n] <= the payload's size, and the payload allocation must reach the next 4-byte multiple past offsets[n]
 * (staged loads read whole aligned words; hipMalloc'd buffers always do): the kernel does not know the payload's
 * size, so an offset past it is read as given. A frame whose end lies before its start decodes as SG_FRAME_SHORT.
 * sg_codec_encode_flow: one 16-byte response frame per request at frames_out + 16 * i (zero-filled for
 * frames whose kind is not SG_FRAME_FLOW: the Java server sends nothing for those). */
#define SG_MSG_TYPE_PING       0
#define SG_MSG_TYPE_FLOW       1
#define SG_MSG_TYPE_PARAM_FLOW 2
#define SG_FRAME_FLOW     0   /* a flow token request, decoded                                          */
#define SG_FRAME_SHORT    1   /* fewer than 5 bytes: DefaultRequestEntityDecoder returns null            */
#define SG_FRAME_NO_DATA  2   /* MSG_TYPE_FLOW without a decodable body (fewer than 12 data bytes)       */
#define SG_FRAME_OTHER    3   /* another message type (ping, param, concurrent): the host's own path     */
#define SG_RESPONSE_FRAME_BYTES 16
int sg_codec_decode_flow(sg_handle* h, const uint8_t* payload, const uint32_t* offsets, const int64_t* ts_ms,
                         uint64_t n, sg_req* req_out, int32_t* xid_out, uint8_t* kind_out, void* stream);
int sg_codec_encode_flow(sg_handle* h, const int32_t* xid, const uint8_t* kind, const sg_result* res, uint64_t n,
                         uint8_t* frames_out, void* stream);

/* ---------- param-flow wire codec and the value dictionary ----------
 * MSG_TYPE_PARAM_FLOW data is [i64 flowId][i32 count][i32 amount] and then `amount` parameters, each one type byte
 * (ClusterConstants.PARAM_TYPE_*) and its payload (ParamFlowRequestDataDecoder.java:35-90, written by
 * ParamFlowRequestDataWriter.java:48-125): INTEGER i32, LONG i64, BYTE 1 byte, DOUBLE 8 bytes, FLOAT 4 bytes,
 * SHORT i16, BOOLEAN 1 byte (non-zero is true), STRING [i32 length][bytes]; big-endian. Any other type byte takes
 * that one byte and adds no parameter. Fewer than 16 data bytes or amount <= 0 decode to null data; a read past the
 * frame's end or a negative string length throws in the Java decoder and no request reaches the service
 * (SG_FRAME_MALFORMED; amount > the bytes left is answered so without looping, every parameter takes a byte). Unread
 * trailing bytes are ignored. The response is the flow response frame with type 2 and waitInMs always 0
 * (ParamFlowRequestProcessor.toResponse).
 *
 * Value dictionary (one per handle; the ValueDictionary of INTEGRATION.md §4c on the device). sg_cparam_* identify a
 * parameter value by a u64; ClusterParamMetric identifies it by Java equals on the boxed object. The dictionary maps
 * key = (type tag, canonical payload bytes) to dense ids 1, 2, 3, …: the payload as on the wire, except BOOLEAN
 * 00 / 01, every DOUBLE NaN 7FF8000000000000 and every FLOAT NaN 7FC00000 (Double.equals / Float.equals compare
 * doubleToLongBits / floatToIntBits: one NaN, +0.0 and -0.0 apart). Integer 5, Long 5, Short 5, Byte 5, "5",
 * Float 5.0 and Double 5.0 are seven values. Strings are compared as their bytes: Java decodes them with the
 * platform charset and folds malformed UTF-8 onto U+FFFD, so two malformed byte strings that Java would find equal
 * are two values here. Ids are assigned in order of first appearance — frame order, then position in the frame; array
 * order for sg_vdict_intern — and never change for the life of the handle, so they are a pure function of the input
 * history. Lookups are exact (hash, then a byte compare).
 *   sg_vdict_init    capacity 2^capacity_log2 values (1..28), arena_bytes for the payloads longer than 8 bytes,
 *                    max_batch_values = the most values one sg_vdict_intern / sg_codec_decode_param call may carry
 *                    (< 2^31). Once per handle: a second call is SG_E_UNSUPPORTED; a dictionary does not grow.
 *   sg_vdict_intern  n values in HOST memory: types[n] (SG_PARAM_TYPE_*), offsets[n + 1] into bytes (the payload as
 *                    on the wire, a STRING's bytes without the length; fixed types must have their size, else
 *                    SG_E_INVAL) → ids_out[n]. How the shim names hot-item values (ParamFlowRuleUtil.parseHotItems,
 *                    typed by classType) before sg_cparam_load_rules. It runs the decoder's device pipeline.
 *   sg_vdict_lookup  ids[n] → types_out[n], offsets_out[n + 1], bytes_out (canonical payloads), HOST memory; for
 *                    sg_cparam_top_values reporting. An id of 0, above the highest id handed out, or given back by
 *                    sg_vdict_sweep and not handed out again is SG_E_INVAL; bytes_cap too small is SG_E_CAPACITY with
 *                    offsets_out filled.
 *   sg_vdict_size    live values and arena bytes in use.
 *   sg_vdict_grow    a larger dictionary in place: capacity_log2 (at most 28) and arena_bytes both at least what they
 *                    are (SG_E_INVAL otherwise, or before sg_vdict_init). Entries and the used arena bytes are copied
 *                    and the lookup table is rebuilt on the device from the entries; every id, sg_vdict_size,
 *                    sg_vdict_lookup and the ids handed out next (count + 1, …) are as in a dictionary that was this
 *                    large from the start. max_batch_values is unchanged. All or nothing: SG_E_NOMEM leaves the
 *                    dictionary as it was. After a sweep the ids given back stay given back, the free list carries over
 *                    and the next ids are what they would have been without the growth.
 *   sg_vdict_sweep   gives back the ids that nothing names any more. Ids stay array positions and are never renumbered
 *                    (the value tables hash them, hot items carry them, the shim caches them): an id in [1, high] —
 *                    high = the largest id ever handed out, it never decreases — that is not free already stays live
 *                    iff it appears in at least one of
 *                      1. the value word of a taken slot of a table sg_param_sweep / sg_cparam_sweep read on this
 *                         handle: the sg_param_* table, the ParamFlowSlot chain's tables, the cluster param keys
 *                         (the embedded token server's included);
 *                      2. a thread-count entry of the ParamFlowSlot chain whose owner word is taken;
 *                      3. a hot item of a rule set in force (sg_param_load_rules, sg_cparam_load_rules,
 *                         sg_pslot_load_rules — the gateway's converted rules are loaded through the last);
 *                      4. the gateway's "$NM" and "$D" ids, once sg_gateway_load_rules has run;
 *                      5. a row not yet fetched from the block log with app_kind SG_BLOCK_APP_VALUE or _LABEL;
 *                      6. a row not yet fetched from the server log of the param family (the caller resolves 5 and 6
 *                         with sg_vdict_lookup after it fetches them: they still mean the same value);
 *                      7. keep_ids[0 .. n_keep) (HOST memory): the ids the shim holds outside the handle.
 *                    A table word that is no dictionary id (outside [1, high], the ~0 of a side slot) is ignored: a
 *                    table keyed by the caller's own numbering can only keep too much. Everything else is freed: its
 *                    entry is dead, sg_vdict_lookup of it is SG_E_INVAL, its arena bytes are reclaimed (the live long
 *                    payloads are compacted in id order, arena_used = the sum of their lengths), n_values counts the
 *                    live values, and the capacity refusals compare live + fresh values with the capacity and the
 *                    compacted arena bytes + new bytes with the arena size. A live id looks up to the same type and
 *                    bytes as before. New values then take ids as follows: the fresh values of a batch are ranked by
 *                    first appearance, as ever; rank r takes the r-th free id in ascending order while free ids last,
 *                    then high + 1, high + 2, …. With no free id every id is what it always was.
 *                    No decision changes: a freed value has no entry in any table, so the request that brings it back
 *                    is decided as a first-seen value under whatever id it gets — what the table sweeps guarantee for
 *                    the table side.
 *                    IN FLIGHT: an id from sg_codec_decode_param, sg_gateway_parse_batch or sg_vdict_intern that has not
 *                    been sent through a decide call yet is in no table: list it in keep_ids, or sweep after the
 *                    decide call. The same holds for ids the shim caches for hot items it has not loaded yet.
 *                    The call completes enqueued work first. All or nothing: the new entries, lookup table, arena and
 *                    free list are built beside the ones in force and swapped at the end; SG_E_NOMEM and every other
 *                    refusal leave the handle as it was. SG_E_INVAL before anything changes: before sg_vdict_init;
 *                    n_keep > 0 with null keep_ids; a keep_ids entry that is 0, above high or already free. No
 *                    timestamp is involved, so there is no SG_E_TIME. *out (may be null): live, removed (by this
 *                    call), free_ids (after the call, earlier sweeps' unused ids included), high, arena_before,
 *                    arena_after. The shim's cycle: sweep the tables at the current time, sweep the dictionary with
 *                    the ids it still holds, and grow only if live is still near the capacity.
 * All or nothing: a batch whose new values would exceed the capacity, or whose new long payloads the arena, returns
 * SG_E_CAPACITY and leaves the dictionary as it was — size, ids and arena.
 *
 * sg_codec_decode_param: inputs as sg_codec_decode_flow (DEVICE payload, offsets[n + 1], ts_ms[n]; n <= max_batch);
 * outputs DEVICE req_out[n], values_out[values_cap], xid_out[n], kind_out[n] and HOST *n_values. A
 * SG_FRAME_PARAM frame gets key = the rule index of its flowId in the handle's sg_cparam_load_rules (unknown →
 * SG_KEY_NO_RULE, flowId <= 0 → SG_KEY_BAD), acquire = count, and value_begin / value_count = the dictionary ids of
 * its valid parameters, appended to values_out in frame order (the range contract of sg_cparam_decide_batch); a
 * frame with no valid parameter keeps value_count 0 (BAD_REQUEST). Every other kind — under 5 bytes SG_FRAME_SHORT,
 * null data SG_FRAME_NO_DATA, a throw SG_FRAME_MALFORMED, another message type (flow included) SG_FRAME_OTHER —
 * gets key SG_KEY_BAD, acquire 0, value_count 0 and interns nothing; value_begin is the running total for every
 * frame. A mixed stream is decoded by calling both decoders over the same payload. The call runs on `stream` and
 * returns after it completed (it needs the total and the capacity verdict). *n_values is the number of values of
 * the batch; when it exceeds values_cap or max_batch_values the call returns SG_E_CAPACITY with *n_values set and
 * nothing interned. SG_E_CAPACITY from the dictionary: as above (the outputs are then undefined). A payload that is
 * not 4-byte aligned is SG_E_INVAL.
 * sg_codec_encode_param: as sg_codec_encode_flow for SG_FRAME_PARAM kinds, waitInMs 0 whatever res.wait_ms holds.
 *
 * Not covered: the node handle (sg_node_*), the concurrent-token message types 3 / 4 (the default server registers
 * no decoder for them). */
#define SG_FRAME_PARAM     4   /* a param-flow token request, decoded                                    */
#define SG_FRAME_MALFORMED 5   /* MSG_TYPE_PARAM_FLOW whose decoder would throw: no request is made       */
#define SG_PARAM_TYPE_INTEGER 0
#define SG_PARAM_TYPE_LONG    1
#define SG_PARAM_TYPE_BYTE    2
#define SG_PARAM_TYPE_DOUBLE  3
#define SG_PARAM_TYPE_FLOAT   4
#define SG_PARAM_TYPE_SHORT   5
#define SG_PARAM_TYPE_BOOLEAN 6
#define SG_PARAM_TYPE_STRING  7
typedef struct sg_vdict_config {
    int32_t  capacity_log2;     /* 2^capacity_log2 values                                */
    int32_t  reserved;
    uint64_t arena_bytes;       /* bytes of payloads longer than 8 bytes                 */
    uint64_t max_batch_values;  /* values per intern / decode call                       */
} sg_vdict_config;
int sg_vdict_init(sg_handle* h, const sg_vdict_config* cfg);
int sg_vdict_intern(sg_handle* h, const uint8_t* types, const uint32_t* offsets, const uint8_t* bytes, uint64_t n,
                    uint64_t* ids_out);
int sg_vdict_lookup(sg_handle* h, const uint64_t* ids, uint64_t n, uint8_t* types_out, uint32_t* offsets_out,
                    uint8_t* bytes_out, uint64_t bytes_cap);
int sg_vdict_size(sg_handle* h, uint64_t* n_values, uint64_t* arena_used);
int sg_vdict_grow(sg_handle* h, int32_t capacity_log2, uint64_t arena_bytes);
typedef struct sg_vdict_sweep_stats {
    uint64_t live;           /* values after the call                                              */
    uint64_t removed;        /* ids this call freed                                                */
    uint64_t free_ids;       /* free ids after the call: removed + earlier sweeps' not yet reused  */
    uint64_t high;           /* the largest id ever handed out                                     */
    uint64_t arena_before;   /* arena bytes in use before                                          */
    uint64_t arena_after;    /* ... and after: the sum of the live payloads longer than 8 bytes    */
} sg_vdict_sweep_stats;
int sg_vdict_sweep(sg_handle* h, const uint64_t* keep_ids, uint64_t n_keep, sg_vdict_sweep_stats* out);
int sg_codec_decode_param(sg_handle* h, const uint8_t* payload, const uint32_t* offsets, const int64_t* ts_ms,
                          uint64_t n, sg_cparam_req* req_out, uint64_t* values_out, uint64_t values_cap,
                          uint64_t* n_values, int32_t* xid_out, uint8_t* kind_out, void* stream);
int sg_codec_encode_param(sg_handle* h, const int32_t* xid, const uint8_t* kind, const sg_result* res, uint64_t n,
                          uint8_t* frames_out, void* stream);

/* ---- GatewayFlowSlot (sentinel-api-gateway-adapter-common): gateway rules and the request parameter parser ----
 * GatewayFlowSlot.checkGatewayParamFlow (slot/GatewayFlowSlot.java:47-71) is ParamFlowChecker.passCheck over the
 * ParamFlowRules GatewayRuleManager converted from the gateway rules, on the Object[] GatewayParamParser built for the
 * request. The check itself is sg_pslot_* / sg_slot_decide_batch; these calls are the two parts in front of it.
 *
 * Rules. sg_gateway_rule is a GatewayFlowRule with its GatewayParamFlowItem flattened (has_item = 0: no paramItem).
 * The resource is the caller's resource index (route id or custom API name, resource_mode says which), the field name
 * stays with the caller (field_blank = StringUtil.isBlank(fieldName)), the pattern is bytes [pattern_off, + pattern_len)
 * of one blob (pattern_null = 1: null). capacity_log2 is handed to the converted rule's value table.
 *   sg_gateway_load_rules  needs sg_vdict_init (else SG_E_INVAL); completes enqueued work; drops what
 *     GatewayRuleManager.isValidRule drops (rule/GatewayRuleManager.java:117-145), silently; converts as
 *     applyGatewayRuleInternal (:179-237) per resource in the caller's order: rules with an item get paramIdx 0, 1, 2, …
 *     and, when the pattern is non-null, the hot item ("$NM", 10,000,000) of GatewayRuleConverter
 *     .generateNonMatchPassParamItem; every rule without an item gets paramIdx = the number of item rules, and item-less
 *     rules whose converted rules are equal collapse into the first (the reference keeps them in a HashSet). "$NM" and
 *     then "$D" are interned as SG_PARAM_TYPE_STRING values (known strings keep their ids). The parser's per-resource
 *     tables go to the device. A resource >= n_resources or a pattern range outside the blob is SG_E_INVAL; a failed
 *     load leaves the rules loaded before in force. Rules of one resource with different resource modes are legal.
 *   sg_gateway_converted  the converted rules sorted by (resource, paramIdx, caller order), their hot items and
 *     source_out[i] = the index of the gateway rule behind converted rule i. The reference's order within a resource is a
 *     HashSet's iteration order; this one is fixed. The caller puts them IN FRONT OF its ordinary
 *     ParamFlowRules (hot_begin of those shifted by *n_hot) and calls sg_pslot_load_rules once: per resource the walkers
 *     then check the gateway rules first and the ordinary ones after, on the same args — GatewayFlowSlot (order -4000)
 *     before ParamFlowSlot (-3000). A cap too small: SG_E_CAPACITY with *n_rules / *n_hot set. Null outputs with cap 0
 *     ask for the counts.
 *   sg_gateway_param_rule_count  a resource's number of item rules and whether it has an item-less rule (0 / 0 for a
 *     resource without valid gateway rules or >= n_resources).
 *   sg_gateway_parse_batch  GatewayParamParser.parseParameterFor (param/GatewayParamParser.java:51-84, :156-174) for n
 *     requests; every pointer but h, n_args and n_values is a DEVICE pointer. req[i].resource_mode is the adapter's
 *     predicate (rule.getResourceMode() == resource_mode). Item k of a request — items[item_begin + k] — is what the
 *     caller's RequestItemParser returned for the resource's item rule with paramIdx k (remote address, Host, header,
 *     URL parameter or cookie by the rule's parse strategy): bytes [off, off + len) of `bytes`, or SG_GW_ITEM_NULL.
 *     SG_GW_ITEM_REGEX_MATCH is java.util.regex's verdict for a REGEX rule (Pattern.matcher(value).matches()), also to
 *     be set when the pattern did not compile (GatewayRegexCache null keeps the value). No item may belong to two
 *     requests. Per request: a resource without valid gateway rules or >= n_resources gets arg_count 0; an item rule
 *     whose resource_mode differs from the request's gives arg_count 0 (item-less rules are not asked); otherwise one
 *     arg per item rule and a last "$D" arg when the resource has an item-less rule. An arg is SG_ARG_NULL (value_count
 *     0) for a null item or a parse strategy above 4, else SG_ARG_VALUE with one value: the dictionary id of the item's
 *     string when gw_match keeps it (no or empty pattern; EXACT equal bytes; CONTAINS a byte substring; REGEX the
 *     verdict bit; PREFIX and every other strategy keep the value, the reference's default branch), else the id of
 *     "$NM". args_out / values_out are in request order, then arg index; value_begin of every arg is the running value
 *     count. ext_inout (sg_slot_ext[n]) and pev_inout (sg_pslot_event[n]), where non-null, get arg_begin, arg_count and
 *     args_null = 0, their other fields are left: the result feeds sg_slot_decide_batch / sg_pslot_decide_batch as it
 *     is. New strings get ids in order of first appearance (request, then arg). Exits are parsed like entries.
 *     The call runs on `stream` and returns after it completed. All or nothing, each of these before anything is
 *     interned: item_count != the resource's item-rule count, an item range or byte range out of bounds, an item of two
 *     requests, a string of 2^24 bytes or more, `bytes` not 4-byte aligned (SG_E_INVAL); n or the value count above
 *     max_batch_values, args_cap / values_cap too small (SG_E_CAPACITY, *n_args / *n_values set); the dictionary or its
 *     arena full (SG_E_CAPACITY, dictionary unchanged; outputs undefined). SG_E_INVAL before sg_gateway_load_rules.
 * Not covered: regular expressions on the device, the node handle. GatewayApiDefinitionManager's path matching and the
 * expansion of HTTP requests into these records are the block below (sg_gateway_load_apis, sg_gateway_expand_batch). */
#define SG_GW_PARSE_CLIENT_IP  0
#define SG_GW_PARSE_HOST       1
#define SG_GW_PARSE_HEADER     2
#define SG_GW_PARSE_URL_PARAM  3
#define SG_GW_PARSE_COOKIE     4
#define SG_GW_MATCH_EXACT      0
#define SG_GW_MATCH_PREFIX     1
#define SG_GW_MATCH_REGEX      2
#define SG_GW_MATCH_CONTAINS   3
#define SG_GW_ITEM_NULL         1u  /* the RequestItemParser returned null                        */
#define SG_GW_ITEM_REGEX_MATCH  2u  /* REGEX rules: the value matches (or the pattern is invalid) */
#define SG_GW_NM_THRESHOLD  10000000 /* generateNonMatchPassParamItem's count                     */
typedef struct sg_gateway_rule {
    double   count;
    int64_t  interval_sec;             /* → durationInSec                                         */
    uint32_t resource;
    int32_t  resource_mode;            /* RESOURCE_MODE_ROUTE_ID 0 / CUSTOM_API_NAME 1            */
    int32_t  grade;
    int32_t  control_behavior;
    int32_t  burst;
    int32_t  max_queueing_timeout_ms;
    int32_t  capacity_log2;            /* the converted rule's sg_param_rule.capacity_log2        */
    int32_t  has_item;                 /* 0: paramItem == null; the fields below are then unread  */
    int32_t  parse_strategy;           /* SG_GW_PARSE_*                                           */
    int32_t  field_blank;              /* StringUtil.isBlank(fieldName)                           */
    int32_t  match_strategy;           /* SG_GW_MATCH_*                                           */
    int32_t  pattern_null;             /* pattern == null                                         */
    uint32_t pattern_off;
    uint32_t pattern_len;
} sg_gateway_rule;                     /* 72 bytes */
typedef struct sg_gateway_req {
    uint32_t resource;
    int32_t  resource_mode;
    uint32_t item_begin;
    uint32_t item_count;
} sg_gateway_req;                      /* 16 bytes */
typedef struct sg_gateway_item {
    uint32_t off;
    uint32_t len;
    uint32_t flags;                    /* SG_GW_ITEM_*                                            */
    uint32_t reserved;
} sg_gateway_item;                     /* 16 bytes */
int sg_gateway_load_rules(sg_handle* h, const sg_gateway_rule* rules, uint32_t n, const uint8_t* pattern_bytes,
                          uint64_t n_pattern_bytes, uint32_t n_resources);
int sg_gateway_converted(sg_handle* h, sg_pslot_rule* rules_out, uint32_t cap, uint32_t* n_rules,
                         sg_param_hot_item* hot_out, uint32_t hot_cap, uint32_t* n_hot, uint32_t* source_out);
int sg_gateway_param_rule_count(sg_handle* h, uint32_t resource, uint32_t* n_item_rules, int32_t* has_item_less);
int sg_gateway_parse_batch(sg_handle* h, const sg_gateway_req* req, uint64_t n, const sg_gateway_item* items,
                           uint64_t n_items, const uint8_t* bytes, uint64_t n_bytes, sg_pslot_arg* args_out,
                           uint64_t args_cap, uint64_t* values_out, uint64_t values_cap, sg_slot_ext* ext_inout,
                           sg_pslot_event* pev_inout, uint64_t* n_args, uint64_t* n_values, void* stream);

/* ---- Gateway API definitions (GatewayApiDefinitionManager, the Spring Cloud Gateway adapter's API matchers) and the
 * expansion of HTTP requests into entries: the front of the gateway path ----
 * SentinelGatewayFilter.filter (sentinel-spring-cloud-gateway-adapter/.../sc/SentinelGatewayFilter.java:72-100) makes
 * one entry for the request's route and one for every custom API whose ApiDefinition matches the request path
 * (pickMatchingApiDefinitions :106-112), each with the Object[] of parseParameterFor. These calls decide the path
 * predicates on the device and write the records sg_gateway_parse_batch and sg_slot_decide_batch take as they are.
 *
 * Definitions. sg_gateway_api is an ApiDefinition: `resource` is the caller's index of the API name, its predicates are
 * preds[pred_begin, + pred_count), SG_GW_API_NAME_BLANK / SG_GW_API_PREDS_NULL say what isValidApi looks at.
 * sg_gateway_api_pred is an ApiPredicateItem: the pattern is bytes [pattern_off, + pattern_len) of one blob.
 *   sg_gateway_load_apis  completes enqueued work; drops what GatewayApiDefinitionManager.isValidApi drops (blank
 *     name, null predicate set), silently; of valid definitions with one `resource` the LAST in caller order is the
 *     definition (the reference keeps them in a HashSet). A predicate that is not an ApiPathPredicateItem
 *     or whose pattern is null or blank (empty or ASCII whitespace only: 9-13, 28-32; a caller whose pattern is blank
 *     by other white space sets SG_GW_PRED_PATTERN_NULL) is skipped (WebExchangeApiMatcher.fromApiPathPredicate); a
 *     definition matches when any other predicate does. Each predicate is classified once:
 *       exact         a strategy other than PREFIX and REGEX: the path bytes equal the pattern bytes
 *       ant           PREFIX with `*` or `?`, no `{` `}`, at most one `**` segment: the Ant matcher below
 *       never         PREFIX without `*` and `?` (AntPathMatcher.isPattern is false: not even its own text matches),
 *                     and REGEX with SG_GW_PRED_REGEX_INVALID (the reference aborts the definition's matcher at a
 *                     Set-order-dependent point; here the predicate never matches and the others stay; §9)
 *       host verdict  REGEX; PREFIX holding `{` or `}`; PREFIX with two or more `**` segments. The caller evaluates
 *                     these (java.util.regex, Spring's AntPathMatcher) and hands the true ones over as verdict ids.
 *     Verdict ids: the host-verdict predicates in the order of preds[] (every one, referenced or not) are 0, 1, …;
 *     behind them come the kept gateway rules whose item has SG_GW_MATCH_REGEX, in the caller's rule order. Either
 *     load renumbers them; sg_gateway_verdict_ids lists them. default_context is the context id API entries get.
 *     A load replaces the definitions all or nothing: a resource >= n_resources, a predicate range outside preds or a
 *     pattern range outside the blob is SG_E_INVAL and leaves the old definitions in force.
 *   The Ant matcher (AntPathMatcher.doMatch(pattern, path, fullMatch = true) of Spring 5.3.18, default settings,
 *     patterns with at most one `**` segment): pattern and path both start with `/` or both do not, else no match. Both
 *     are split at `/`, empty tokens dropped, nothing trimmed, case-sensitive. Pattern segments before the `**` (all,
 *     without one) match the leading path segments one by one; both exhausted together: pattern ends with `/` == path
 *     ends with `/`; path exhausted first: a match iff the one remaining pattern segment is `*` and the path ends with
 *     `/`, or every remaining segment is `**`; pattern exhausted first: no match. Segments after the `**` match the
 *     trailing path segments from the back; at the last pattern segment, pattern ends with `/` != path ends with `/` is
 *     no match; when either side runs out, a match iff only `**` is left. Within a segment `?` is one UTF-8 sequence
 *     (its length from the lead byte, cut at the segment's end; any other byte counts as one), `*` any run, `a**b` is
 *     `a*b`, everything else literal bytes.
 *   sg_gateway_verdict_ids  kind_out[i] 0: index_out[i] is a preds[] index; 1: a gateway rule index. A cap too small:
 *     SG_E_CAPACITY with *n set. Null outputs with cap 0 ask for the count.
 *   sg_gateway_set_item_fields  field_id[i] = the caller's id of gateway rule i's fieldName (read for HEADER, URL_PARAM
 *     and COOKIE items); n must be the rule count of the last sg_gateway_load_rules (else SG_E_INVAL), which drops them.
 *   sg_gateway_expand_batch  n HTTP requests → entries; every pointer but h, n_req and n_items is a DEVICE pointer.
 *     A request's path is bytes [path_off, + path_len) of `bytes`, its fields (what the RequestItemParser can read:
 *     kind SG_GW_PARSE_*, name_id for kinds 2-4) are fields[field_begin, + field_count), and verdicts[verdict_begin,
 *     + verdict_count) holds the verdict ids that are true for it, ascending and unique. Entries come in request order:
 *     the route entry first (route != SG_GW_NO_ROUTE; resource_mode 0, the request's origin and context), then one per
 *     matching API by ascending caller index of its definition (resource_mode 1, origin 0, the default context; the
 *     reference's order is a HashSet's, §9). Per entry: req_out (item_count = the resource's item-rule count, items at
 *     items_out[item_begin ..]), src_out (the request index), ev_out (ts_ms, create_ts 0, count 1, SG_LOCAL_ENTRY) and
 *     ext_out.context (the arg fields are left for the parser). Item k is the request's first field with kind == the
 *     rule's parse strategy and, for kinds 2-4, name_id == the rule's field id; SG_GW_ITEM_NULL without one, for a
 *     strategy outside 0-4 and while no fields are set; SG_GW_ITEM_REGEX_MATCH when the rule's verdict id is listed.
 *     Every entry of a request is written; what the adapter does after a request's first blocked entry (the later
 *     transformers are not subscribed) stays with the caller. The call runs on `stream` and returns after it
 *     completed. All or nothing: a field, path or verdict range out of bounds, a verdict slice not ascending, a verdict
 *     id out of range, `bytes` not 4-byte aligned (SG_E_INVAL); n above max_batch, req_cap or items_cap too small
 *     (SG_E_CAPACITY, *n_req / *n_items set), a batch that expands to 2^32 entries or items, or more (SG_E_CAPACITY). SG_E_INVAL
 *     before sg_gateway_load_apis and sg_gateway_load_rules both succeeded. */
#define SG_GW_URL_MATCH_EXACT   0
#define SG_GW_URL_MATCH_PREFIX  1
#define SG_GW_URL_MATCH_REGEX   2
#define SG_GW_API_NAME_BLANK      1u  /* StringUtil.isBlank(apiName)                              */
#define SG_GW_API_PREDS_NULL      2u  /* getPredicateItems() == null                              */
#define SG_GW_PRED_PATTERN_NULL   1u  /* pattern == null                                          */
#define SG_GW_PRED_NOT_PATH       2u  /* not an ApiPathPredicateItem                              */
#define SG_GW_PRED_REGEX_INVALID  4u  /* Pattern.compile threw                                    */
#define SG_GW_NO_ROUTE  0xFFFFFFFFu   /* exchange has no GATEWAY_ROUTE_ATTR                       */
typedef struct sg_gateway_api {
    uint32_t resource;
    uint32_t pred_begin;
    uint32_t pred_count;
    uint32_t flags;                    /* SG_GW_API_*                                             */
} sg_gateway_api;                      /* 16 bytes */
typedef struct sg_gateway_api_pred {
    int32_t  match_strategy;           /* SG_GW_URL_MATCH_*; any other value is exact             */
    uint32_t flags;                    /* SG_GW_PRED_*                                            */
    uint32_t pattern_off;
    uint32_t pattern_len;
} sg_gateway_api_pred;                 /* 16 bytes */
typedef struct sg_gateway_http_req {
    int64_t  ts_ms;
    uint32_t route;                    /* resource index of the route id, or SG_GW_NO_ROUTE       */
    int32_t  origin;                   /* the route entry's sg_local_event.origin                 */
    uint32_t context;                  /* the route entry's sg_slot_ext.context                   */
    uint32_t path_off;
    uint32_t path_len;
    uint32_t field_begin;
    uint32_t field_count;
    uint32_t verdict_begin;
    uint32_t verdict_count;
    uint32_t reserved;
} sg_gateway_http_req;                 /* 48 bytes */
typedef struct sg_gateway_field {
    uint32_t kind;                     /* SG_GW_PARSE_*                                           */
    uint32_t name_id;                  /* kinds 2-4: the caller's id of the header / parameter / cookie name */
    uint32_t off;
    uint32_t len;
} sg_gateway_field;                    /* 16 bytes */
int sg_gateway_load_apis(sg_handle* h, const sg_gateway_api* apis, uint32_t n_apis, const sg_gateway_api_pred* preds,
                         uint32_t n_preds, const uint8_t* pattern_bytes, uint64_t n_pattern_bytes, uint32_t n_resources,
                         uint32_t default_context);
int sg_gateway_verdict_ids(sg_handle* h, uint8_t* kind_out, uint32_t* index_out, uint32_t cap, uint32_t* n);
int sg_gateway_set_item_fields(sg_handle* h, const uint32_t* field_id, uint32_t n);
int sg_gateway_expand_batch(sg_handle* h, const sg_gateway_http_req* req, uint64_t n, const sg_gateway_field* fields,
                            uint64_t n_fields, const uint32_t* verdicts, uint64_t n_verdicts, const uint8_t* bytes,
                            uint64_t n_bytes, sg_gateway_req* req_out, uint64_t req_cap, sg_gateway_item* items_out,
                            uint64_t items_cap, uint32_t* src_out, sg_local_event* ev_out, sg_slot_ext* ext_out,
                            uint64_t* n_req, uint64_t* n_items, void* stream);

/* ---------- Envoy rate-limit service ----------
 * SentinelEnvoyRlsServiceImpl.shouldRateLimit (sentinel-cluster/sentinel-cluster-server-envoy-rls/.../service/v3/
 * SentinelEnvoyRlsServiceImpl.java:34-85) for a time-ordered batch of n RateLimitRequests on a handle whose flow
 * rules were loaded as the RLS checker reads them (SimpleClusterFlowChecker.acquireClusterToken, flow/
 * SimpleClusterFlowChecker.java:33-65: GLOBAL threshold count · exceedCount, no namespace limiter, no prioritized
 * occupy). Request j is served at ts_ms with acquireCount = hits_addend (0 → 1) over its descriptors
 * desc_rule[desc_begin, desc_begin + desc_count): a descriptor's rule index (the caller resolves
 * EnvoySentinelRuleConverter.generateFlowId over domain + entries on its side), or -1 when it has no rule. Every
 * descriptor is one token request, all of a batch in one device batch, in order.
 *   overall[j]  SG_RLS_OK / SG_RLS_OVER_LIMIT (any descriptor not OK), or SG_RLS_ERROR when hits_addend < 0
 *               (responseObserver.onError, :36-40; its descriptors are not requested and get code 0)
 *   status[d]   code (SG_RLS_OK when the result is OK or the rule is missing, :55-58, else SG_RLS_OVER_LIMIT),
 *               and for a descriptor with a rule: limit_remaining = the TokenResult's remaining and
 *               requests_per_unit = (int) rule.getCount() (:67-73), has_rule = 1.
 * A descriptor whose rule is not GLOBAL or lies in a namespace with a limiter (the cluster path would apply them,
 * SimpleClusterFlowChecker does not) is SG_E_UNSUPPORTED, more descriptors than max_batch SG_E_CAPACITY: both
 * before any state change. */
#define SG_RLS_OK          1   /* envoy.service.ratelimit.v3.RateLimitResponse.Code.OK         */
#define SG_RLS_OVER_LIMIT  2   /* ... Code.OVER_LIMIT                                          */
#define SG_RLS_ERROR      (-1) /* hits_addend < 0: the call fails                               */
typedef struct {
    int64_t  ts_ms;        /* TimeUtil.currentTimeMillis() when the call is served */
    int32_t  hits_addend;  /* RateLimitRequest.hits_addend                         */
    uint32_t desc_begin;
    uint32_t desc_count;
    uint32_t pad;
} sg_rls_request;          /* 24 bytes */
typedef struct {
    int32_t code;
    int32_t limit_remaining;
    int32_t requests_per_unit;
    int32_t has_rule;
} sg_rls_status;           /* 16 bytes */
int sg_rls_should_rate_limit(sg_handle* h, const sg_rls_request* req, uint32_t n, const int32_t* desc_rule,
                             uint64_t n_desc, int32_t* overall, sg_rls_status* status);

/* ---- the token server's stat log: sentinel-server.log (cluster/server/log/ClusterServerStatLogUtil.java:32-52) ----
 * Every checker behind DefaultTokenService reports through ClusterServerStatLogUtil.log(key, count): an EagleEye
 * StatLogger with 1-second slots (time slot t - t % 1000) and one COUNT_SUM entry per key string, written as one line
 * per entry `time|1|key|count,0` (StatLogWriteTask.run; the key is the single string, e.g. `flow|block|123`). The
 * device keeps that rollup across batches in an exact table in device memory and hands out rows.
 * What is logged (the event says which key, flow_id is the rule's flowId):
 *   flow tokens (ClusterFlowChecker.java:91, 102-107; sg_flow_decide_batch, _host, sg_flow_submit, sg_flow_enqueue):
 *     SHOULD_WAIT → SG_SLOG_FLOW_WAITING += 1; BLOCKED → SG_SLOG_FLOW_BLOCK += acquireCount and
 *     SG_SLOG_FLOW_BLOCK_REQUEST += 1, and for a prioritized request SG_SLOG_FLOW_OCCUPIED_BLOCK += 1. OK,
 *     TOO_MANY_REQUEST, FAIL, NO_RULE_EXISTS and BAD_REQUEST log nothing: the default server logs no passes.
 *   RLS (SimpleClusterFlowChecker.java:49-50, 60-61; sg_rls_should_rate_limit): OK → SG_SLOG_FLOW_PASS += acquireCount
 *     and SG_SLOG_FLOW_PASS_REQUEST += 1; BLOCKED → SG_SLOG_FLOW_BLOCK, SG_SLOG_FLOW_BLOCK_REQUEST; no waiting or
 *     occupied rows; a descriptor without a rule and a request with hits_addend < 0 log nothing.
 *   concurrent tokens (ConcurrentClusterFlowChecker.java:58/67, 73, 96-99; sg_conc_decide_batch, _host): an acquire's
 *     OK → SG_SLOG_CONC_PASS += acquireCount, its BLOCKED → SG_SLOG_CONC_BLOCK += acquireCount (once: of the two
 *     identical Java sites one runs); RELEASE_OK → SG_SLOG_CONC_RELEASE += the token's acquireCount under the token's
 *     flowId. ALREADY_RELEASE, NO_RULE_EXISTS, BAD_REQUEST and sg_conc_expire (RegularExpireStrategy) log nothing.
 *   cluster param tokens (ClusterParamFlowChecker.java:58-80; sg_cparam_decide_batch, _host): OK → SG_SLOG_PARAM_PASS
 *     += 1; BLOCKED → SG_SLOG_PARAM_BLOCK += 1 with value = blockObject, the first value in request order whose check
 *     failed, as the caller's u64 value id (the caller turns it into %s, with sg_vdict_lookup for instance).
 *     TOO_MANY_REQUEST, NO_RULE_EXISTS and BAD_REQUEST log nothing.
 * Not logged: the embedded token server's decisions taken inside the local chain's cx walkers
 * (sg_local_set_cluster_state(SERVER) decides them in the walker, and which rule decided is not recoverable
 * afterwards); ClusterConcurrentCheckerLogListener's periodic lines (sg_conc_read_state gives the caller their
 * numbers).
 *   sg_server_log_enable ← the StatLogger's creation: a table of 2^capacity_log2 slots (4..24), one slot per (second,
 *     family, flowId, value) with that key's counters side by side (96 bytes a slot, three such arrays), and every
 *     flow, concurrent and cluster param token batch decided from then on adds its logged decisions behind its
 *     walkers. Allowed at any time (rows record only what was decided after it); a second call with the same capacity
 *     does nothing, with another SG_E_INVAL. The table belongs to the handle and outlives every
 *     rule reload: rows carry the flowId, not the rule index, so a reload that renumbers the rules changes nothing. A
 *     handle that never calls it launches exactly the kernels it launched before and stores nothing extra.
 *   sg_server_log ← the rolling task (StatLogWriteTask) at now_ms: it first drains the pipelines, then hands out every
 *     row whose second is complete (timestamp + 1000 <= now_ms - now_ms % 1000) into HOST memory, sorted by (timestamp,
 *     event, flow_id, value), and removes them from the table. cap too small: SG_E_CAPACITY, *n_rows = the rows needed,
 *     nothing changes (the lost totals included). SG_E_INVAL before sg_server_log_enable. A decision whose key found
 *     no free slot is not logged and never changes a decision: it is counted in *lost_events and its acquireCount in
 *     *lost_count, reported by the next successful call and cleared by it. A row exists if and only if its count is
 *     non-zero (every request that reaches a checker has acquireCount >= 1, DefaultTokenService.java:87-93). One row
 *     per key and second (the reference's maxEntryCount(5000) rolls the map early, so a key can have several lines in
 *     a second: summed per key and second they equal the row). */
#define SG_SLOG_FLOW_WAITING         0   /* flow|waiting|id            += 1            */
#define SG_SLOG_FLOW_BLOCK           1   /* flow|block|id              += acquireCount */
#define SG_SLOG_FLOW_BLOCK_REQUEST   2   /* flow|block_request|id      += 1            */
#define SG_SLOG_FLOW_OCCUPIED_BLOCK  3   /* flow|occupied_block|id     += 1            */
#define SG_SLOG_FLOW_PASS            4   /* flow|pass|id               += acquireCount (RLS only) */
#define SG_SLOG_FLOW_PASS_REQUEST    5   /* flow|pass_request|id       += 1            (RLS only) */
#define SG_SLOG_PARAM_PASS           6   /* param|pass|id              += 1            */
#define SG_SLOG_PARAM_BLOCK          7   /* param|block|id|value       += 1            */
#define SG_SLOG_CONC_PASS            8   /* concurrent|pass|id         += acquireCount */
#define SG_SLOG_CONC_BLOCK           9   /* concurrent|block|id        += acquireCount */
#define SG_SLOG_CONC_RELEASE        10   /* concurrent|release|id      += the token's acquireCount */
typedef struct sg_server_row {
    int64_t  timestamp;   /* the second: t - t % 1000                         */
    int64_t  count;
    int64_t  flow_id;     /* the rule's flowId, not its index                 */
    uint64_t value;       /* SG_SLOG_PARAM_BLOCK: the blocking value's id, else 0 */
    int32_t  event;       /* SG_SLOG_*                                        */
    int32_t  reserved;
} sg_server_row;
int sg_server_log_enable(sg_handle* h, int32_t capacity_log2);
int sg_server_log(sg_handle* h, int64_t now_ms, sg_server_row* rows, uint64_t cap, uint64_t* n_rows,
                  uint64_t* lost_events, uint64_t* lost_count);
/* The two logs over the node handle, with the contracts of sg_server_log_enable / sg_server_log and
 * sg_local_block_log_enable / sg_local_block_log word for word but for these points.
 *   sg_node_server_log_enable enables the front and every shard: sg_node_flow_decide_batch(_host), sg_node_flow_enqueue,
 *     sg_node_conc_* and sg_node_cparam_* then log on the shard that decides, and param tokens decided on the front
 *     (sg_node_front, rules under an enabled limiter) on the front. sg_node_local_block_log_enable enables every shard.
 *     If one handle fails (SG_E_NOMEM, SG_E_DEVICE) the handles before it stay enabled and log, the node's log counts as
 *     off (the fetch is SG_E_INVAL), and the same call again completes the rest.
 *   sg_node_server_log collects every handle's rows, sums rows with equal keys (a rule served by the front and by a
 *     shard stays one row), adds the lost totals and sorts. sg_node_local_block_log concatenates and sorts: a resource
 *     has one owner shard, so no key can come from two; the call checks that (SG_E_DEVICE, the rows kept for the next
 *     call, if it ever fails). cap too small: SG_E_CAPACITY with *n_rows = the sum of the parts' rows, which is
 *     sufficient (equal keys only merge), and nothing changes. If a handle fails in the middle of a fetch, the rows
 *     and lost totals already taken from the handles before it are kept in the node and handed out by the next
 *     successful call; the failing handle and those after it keep theirs in their tables. */
int sg_node_server_log_enable(sg_node* nd, int32_t capacity_log2);
int sg_node_server_log(sg_node* nd, int64_t now_ms, sg_server_row* rows, uint64_t cap, uint64_t* n_rows,
                       uint64_t* lost_events, uint64_t* lost_count);
int sg_node_local_block_log_enable(sg_node* nd, int32_t capacity_log2);
int sg_node_local_block_log(sg_node* nd, int64_t now_ms, sg_block_row* rows, uint64_t cap, uint64_t* n_rows,
                            uint64_t* lost_events, uint64_t* lost_count);

/* Testing aid: copy an internal buffer of the last batch to host memory.
 * what: 0 = records (request order, u64; on the binned flow path with compact front records, u32
 * {bin digit | key in bin | acquire code} in the buffer's first half), 1 = records sorted by flowId, 2 = window-period table
 * (u32 [8][65536]), 3 = first period per window length (i64[8]), 4 = periods per window length (u32[8]), 6 = the
 * saturated ranges the last cluster param walk handed to its skip pass (u32; a batch with multi-value requests
 * clears it between its rounds, SG_E_INVAL before the first cluster param batch). */
int sg_debug_copy(sg_handle* h, int what, void* dst, uint64_t bytes);

/* Library build identification (architecture the kernels were compiled for). */
const char* sg_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* SENTINEL_GPU_H */
