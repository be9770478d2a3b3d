"""Hand-traced KATs of the stat log model (tests/serverlog_ref.py) against the Java lines it is written from, and of
metrics.server_log_lines against literal sentinel-server.log lines. No GPU.

  ClusterFlowChecker.java:91          flow|waiting|id                      (SHOULD_WAIT)
  ClusterFlowChecker.java:102-107     flow|block|id += acquireCount, flow|block_request|id += 1, and for a prioritized
                                      request flow|occupied_block|id += 1  (BLOCKED)
  SimpleClusterFlowChecker.java:49-50 flow|pass|id += acquireCount, flow|pass_request|id += 1 (OK, RLS)
  SimpleClusterFlowChecker.java:60-61 flow|block|id, flow|block_request|id (BLOCKED, RLS)
  ConcurrentClusterFlowChecker.java:58/67, 73, 96-99   concurrent|block / pass / release
  ClusterParamFlowChecker.java:58-80  param|pass|id, param|block|id|blockObject (the first failing value)
"""
import numpy as np

from oracle.binding import ClusterTokenService
from sentinel_amd import abi, metrics
from tests.serverlog_ref import T0, ServerLog

W, B, BR, OB, P, PR = (abi.SLOG_FLOW_WAITING, abi.SLOG_FLOW_BLOCK, abi.SLOG_FLOW_BLOCK_REQUEST,
                       abi.SLOG_FLOW_OCCUPIED_BLOCK, abi.SLOG_FLOW_PASS, abi.SLOG_FLOW_PASS_REQUEST)


def _rows(log, now):
    return [(int(r["timestamp"]), int(r["event"]), int(r["flow_id"]), int(r["value"]), int(r["count"]))
            for r in log.take(now)]


def test_a_blocked_prioritized_request_makes_three_rows_and_a_plain_one_two():
    log = ServerLog()
    log.flow(T0 + 5, 123, 3, True, abi.BLOCKED)
    assert _rows(log, T0 + 1000) == [(T0, B, 123, 0, 3), (T0, BR, 123, 0, 1), (T0, OB, 123, 0, 1)]
    log.flow(T0 + 1005, 123, 3, False, abi.BLOCKED)
    assert _rows(log, T0 + 2000) == [(T0 + 1000, B, 123, 0, 3), (T0 + 1000, BR, 123, 0, 1)]


def test_should_wait_makes_one_row_and_the_other_statuses_none():
    log = ServerLog()
    log.flow(T0, 9, 4, True, abi.SHOULD_WAIT)
    assert _rows(log, T0 + 1000) == [(T0, W, 9, 0, 1)]  # log(key): one, not the acquireCount
    for st in (abi.OK, abi.TOO_MANY_REQUEST, abi.FAIL, abi.NO_RULE_EXISTS, abi.BAD_REQUEST):
        log.flow(T0 + 1000, 9, 4, True, st)
    assert _rows(log, T0 + 5000) == []


def test_rls_pass_makes_two_rows_and_knows_no_priority_or_waiting():
    log = ServerLog()
    log.flow(T0, 7, 5, False, abi.OK, rls=True)
    assert _rows(log, T0 + 1000) == [(T0, P, 7, 0, 5), (T0, PR, 7, 0, 1)]
    log.flow(T0 + 1000, 7, 5, True, abi.BLOCKED, rls=True)
    log.flow(T0 + 1000, 7, 5, True, abi.SHOULD_WAIT, rls=True)
    assert _rows(log, T0 + 2000) == [(T0 + 1000, B, 7, 0, 5), (T0 + 1000, BR, 7, 0, 1)]


def test_sums_per_key_and_second_and_only_complete_seconds_leave():
    log = ServerLog()
    for t, fid, acq in [(T0 + 1, 5, 2), (T0 + 999, 5, 3), (T0 + 1000, 5, 4), (T0 + 500, 6, 1)]:
        log.flow(t, fid, acq, False, abi.BLOCKED)
    assert _rows(log, T0 + 999) == []                       # the open second stays
    assert _rows(log, T0 + 1999) == [(T0, B, 5, 0, 5), (T0, B, 6, 0, 1), (T0, BR, 5, 0, 2), (T0, BR, 6, 0, 1)]
    assert _rows(log, T0 + 1999) == []
    assert _rows(log, T0 + 2000) == [(T0 + 1000, B, 5, 0, 4), (T0 + 1000, BR, 5, 0, 1)]


def test_the_batch_form_equals_the_per_request_form_on_an_oracle_trace():
    """flow_batch (numpy groups) against flow() request by request, on a trace whose oracle results hold OK, BLOCKED,
    SHOULD_WAIT, NO_RULE_EXISTS and BAD_REQUEST; rows carry the flowId, not the rule index."""
    rng = np.random.default_rng(5)
    rules = np.zeros(6, abi.RULE_DTYPE)
    rules["flow_id"] = [900, 5, 77, 1 << 40, 12, 3]
    rules["count"] = [0, 3, 8, 1, 20, 2]
    rules["threshold_type"], rules["sample_count"], rules["window_interval_ms"] = abi.THRESHOLD_GLOBAL, 10, 1000
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"], ns["max_allowed_qps"] = 1, 30000
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_rules(rules)
    n = 4000
    req = np.zeros(n, abi.REQ_DTYPE)
    req["ts_ms"] = T0 + 700 + np.sort(rng.integers(0, 2500, n))
    req["key"] = rng.integers(0, 6, n)
    req["key"][rng.random(n) < 0.02] = abi.KEY_NO_RULE
    req["key"][rng.random(n) < 0.02] = abi.KEY_BAD
    req["key"][rng.random(n) < 0.02] = 6                      # an index past the rules: NO_RULE_EXISTS
    req["acquire"] = rng.integers(1, 4, n)
    req["acquire"][rng.random(n) < 0.02] = 0                  # BAD_REQUEST
    req["key"] |= np.where(rng.random(n) < 0.3, np.uint32(abi.KEY_PRIO), np.uint32(0))
    res = ora.decide(req)
    for st in (abi.OK, abi.BLOCKED, abi.SHOULD_WAIT, abi.NO_RULE_EXISTS, abi.BAD_REQUEST):
        assert (res["status"] == st).any(), st
    for rls in (False, True):
        a, b = ServerLog(), ServerLog()
        a.flow_batch(rules, req, res, rls)
        for q, r in zip(req, res):
            k = int(q["key"]) & abi.KEY_INDEX
            if r["status"] in (abi.NO_RULE_EXISTS, abi.BAD_REQUEST):
                continue
            b.flow(int(q["ts_ms"]), int(rules["flow_id"][k]), int(q["acquire"]), bool(int(q["key"]) & abi.KEY_PRIO),
                   int(r["status"]), rls)
        assert a.counts == b.counts and len(a.counts) > 10
        assert any(k[2] == 1 << 40 for k in a.counts)


def test_a_release_logs_the_acquires_count_under_the_tokens_flow_id_after_a_reorder():
    """ConcurrentClusterFlowChecker.java:96-99 against the oracle: tokens of two rules, the rule array reversed, then
    the releases — each logs node.getAcquireCount() under the flowId its token was acquired for; a second release of a
    token and an unknown id log nothing."""
    from oracle.binding import ConcurrentTokenService
    CP, CB, CR = abi.SLOG_CONC_PASS, abi.SLOG_CONC_BLOCK, abi.SLOG_CONC_RELEASE
    rules = np.zeros(2, abi.RULE_DTYPE)
    rules["flow_id"], rules["count"], rules["threshold_type"] = [501, 777], [5, 4], abi.THRESHOLD_GLOBAL
    rules["sample_count"], rules["window_interval_ms"] = 10, 1000
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"], ns["max_allowed_qps"] = 1, 30000
    ora = ConcurrentTokenService()
    ora.set_namespaces(ns)
    ora.load_rules(rules)
    log = ServerLog()
    a = np.zeros(4, abi.CONC_REQ_DTYPE)
    a["ts_ms"], a["kind"], a["client"] = T0 + np.arange(4), abi.CONC_ACQUIRE, 1
    a["key"], a["acquire"] = [0, 1, 0, 1], [3, 4, 3, 1]        # 501: 3 ok, then 3 + 3 > 5 blocks; 777: 4 ok, 4 + 1 blocks
    res = ora.decide(a)
    assert [int(s) for s in res["status"]] == [abi.OK, abi.OK, abi.BLOCKED, abi.BLOCKED]
    log.conc_batch(rules, a, res)
    new = rules[::-1].copy()                                   # index 0 is flowId 777 now
    ora.load_rules(new)
    r = np.zeros(4, abi.CONC_REQ_DTYPE)
    r["ts_ms"], r["kind"] = T0 + 1000 + np.arange(4), abi.CONC_RELEASE
    r["token_id"] = [res["token_id"][0], res["token_id"][1], res["token_id"][0], 999_999]
    res2 = ora.decide(r)
    assert [int(s) for s in res2["status"]] == [abi.RELEASE_OK, abi.RELEASE_OK, abi.ALREADY_RELEASE, abi.ALREADY_RELEASE]
    log.conc_batch(new, r, res2)
    assert _rows(log, T0 + 2000) == [(T0, CP, 501, 0, 3), (T0, CP, 777, 0, 4), (T0, CB, 501, 0, 3), (T0, CB, 777, 0, 1),
                                     (T0 + 1000, CR, 501, 0, 3), (T0 + 1000, CR, 777, 0, 4)]
    assert not log.tokens


def blocking_value_case():
    """One rule, count 1 per second and value: a saturated by a single-value pass, then multi-value requests whose
    first failing value is first, middle, last, a repeated value ([b, a, a] and [a, a]), and passes between them.
    (rules, ns, req, values, the statuses and blockObjects ClusterParamFlowChecker.java:61-70 gives by hand)."""
    a, fresh = 1 << 50, iter(range(100, 200))
    lists = [[a], [a], [a, next(fresh), next(fresh)], [next(fresh), a, next(fresh)], [next(fresh), next(fresh), a],
             [next(fresh), a, a], [a, a], [next(fresh), next(fresh)], [next(fresh)]]
    status = [abi.OK, abi.BLOCKED, abi.BLOCKED, abi.BLOCKED, abi.BLOCKED, abi.BLOCKED, abi.BLOCKED, abi.OK, abi.OK]
    block = [0, a, a, a, a, a, a, 0, 0]
    rules = np.zeros(1, abi.CPARAM_RULE_DTYPE)
    rules["flow_id"], rules["count"], rules["threshold_type"] = 4242, 1, abi.THRESHOLD_GLOBAL
    rules["sample_count"], rules["window_interval_ms"] = 10, 1000
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    req = np.zeros(len(lists), abi.CPARAM_REQ_DTYPE)
    req["ts_ms"], req["acquire"] = T0 + 10 * np.arange(len(lists)), 1
    req["value_count"] = [len(x) for x in lists]
    req["value_begin"] = np.concatenate([[0], np.cumsum(req["value_count"])[:-1]])
    return rules, ns, req, np.array([v for x in lists for v in x], np.uint64), status, block


def test_a_multi_value_block_names_the_first_failing_value():
    from tests.serverlog_ref import ParamChecker
    rules, ns, req, values, status, block = blocking_value_case()
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_param_rules(rules)
    res, blocks = ParamChecker(ora, rules, ns).decide(req, values)
    assert [int(s) for s in res["status"]] == status and blocks == block
    log = ServerLog()
    log.param_batch(rules, req, res, blocks)
    assert _rows(log, T0 + 1000) == [(T0, abi.SLOG_PARAM_PASS, 4242, 0, 3), (T0, abi.SLOG_PARAM_BLOCK, 4242, 1 << 50, 6)]


def test_the_restated_param_check_follows_hot_items_and_avg_local():
    """AVG_LOCAL over 3 connected clients and per-value hot item counts: the restatement's verdict equals the oracle's
    on every request (ParamChecker.decide asserts it), and blocked multi-value requests name one of their values."""
    from tests.serverlog_ref import ParamChecker
    rng = np.random.default_rng(4)
    rules = np.zeros(3, abi.CPARAM_RULE_DTYPE)
    rules["flow_id"], rules["count"] = [11, 12, 13], [2, 1, 3]
    rules["threshold_type"] = [abi.THRESHOLD_AVG_LOCAL, abi.THRESHOLD_GLOBAL, abi.THRESHOLD_AVG_LOCAL]
    rules["sample_count"], rules["window_interval_ms"] = [10, 2, 5], [1000, 1000, 500]
    rules["hot_begin"], rules["hot_count"] = [0, 2, 4], 2
    hot = np.zeros(6, abi.PARAM_HOT_DTYPE)
    hot["value"], hot["threshold"] = [1, 2, 1, 3, 2, 3], [0, 5, 4, 0, 1, 7]
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 3
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_param_rules(rules, hot)
    n = 1500
    req = np.zeros(n, abi.CPARAM_REQ_DTYPE)
    req["ts_ms"] = T0 + np.sort(rng.integers(0, 2500, n))
    req["key"], req["acquire"] = rng.integers(0, 3, n), rng.integers(1, 3, n)
    req["value_count"] = rng.integers(1, 4, n)
    req["value_begin"] = np.concatenate([[0], np.cumsum(req["value_count"])[:-1]])
    values = rng.integers(1, 6, int(req["value_count"].sum())).astype(np.uint64)
    res, blocks = ParamChecker(ora, rules, ns, hot).decide(req, values)
    blocked = np.nonzero(res["status"] == abi.BLOCKED)[0]
    assert len(blocked) > 100 and (res["status"] == abi.OK).sum() > 100
    for i in blocked:
        assert blocks[i] in values[req["value_begin"][i]: req["value_begin"][i] + req["value_count"][i]]


def test_server_log_lines_against_literal_strings():
    rows = np.zeros(5, abi.SERVER_ROW_DTYPE)
    rows[0] = (T0, 7, 123, 0, abi.SLOG_FLOW_BLOCK, 0)
    rows[1] = (T0, 1, 123, 0, abi.SLOG_FLOW_OCCUPIED_BLOCK, 0)
    rows[2] = (T0 + 1000, 2, 9, 0, abi.SLOG_FLOW_WAITING, 0)
    rows[3] = (T0 + 1000, 3, 44, 17, abi.SLOG_PARAM_BLOCK, 0)
    rows[4] = (T0 + 86_400_000, 1 << 33, 5, 0, abi.SLOG_CONC_RELEASE, 0)
    assert metrics.server_log_lines(rows, value_str=lambda v: f"user-{v}") == [
        "2023-11-14 22:13:20|1|flow|block|123|7,0\n",
        "2023-11-14 22:13:20|1|flow|occupied_block|123|1,0\n",
        "2023-11-14 22:13:21|1|flow|waiting|9|2,0\n",
        "2023-11-14 22:13:21|1|param|block|44|user-17|3,0\n",
        "2023-11-15 22:13:20|1|concurrent|release|5|8589934592,0\n",
    ]
    names = {abi.SLOG_FLOW_BLOCK_REQUEST: "flow|block_request|8", abi.SLOG_FLOW_PASS: "flow|pass|8",
             abi.SLOG_FLOW_PASS_REQUEST: "flow|pass_request|8", abi.SLOG_PARAM_PASS: "param|pass|8",
             abi.SLOG_CONC_PASS: "concurrent|pass|8", abi.SLOG_CONC_BLOCK: "concurrent|block|8"}
    for ev, key in names.items():
        r = np.zeros(1, abi.SERVER_ROW_DTYPE)
        r[0] = (T0, 1, 8, 0, ev, 0)
        assert metrics.server_log_lines(r) == [f"2023-11-14 22:13:20|1|{key}|1,0\n"]
