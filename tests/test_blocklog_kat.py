"""LogSlot's model (tests/blocklog_ref.py) on the CPU: hand-traced ruleLimitApp of every exception class, the line
format of StatLogWriteTask, and — for the traces tests/test_blocklog_gpu.py reuses — that the model's pass / block
status equals the oracle's on every event and that each trace really yields the rows it is meant to cover (a GPU test
that compares rows would pass vacuously on a trace without blocks).

ParamFlowChecker.passCheck returns true when args.length <= paramIdx or the argument is null, so the reference throws no
ParamFlowException with ruleLimitApp "" or "null" through these paths; ParamFlowSlot.java:81-91 still spells both out,
and so do the model and the row kinds (SG_BLOCK_APP_NO_ARG / _NULL_ARG)."""
import datetime

import numpy as np

from oracle.binding import LocalChain, local_rule
from sentinel_amd import abi, metrics
from tests import blocklog_ref as ref
from tests.blocklog_ref import AUTHORITY, DEFAULT, DEGRADE, FLOW, OTHER, PARAM, SYSTEM, T0


def test_rule_limit_app_by_exception_class():
    K = abi
    assert ref.rule_limit_app(FLOW, flow_app=DEFAULT) == (K.BLOCK_APP_LIMIT_APP, 0)
    assert ref.rule_limit_app(FLOW, flow_app=OTHER) == (K.BLOCK_APP_LIMIT_APP, 0xFFFFFFFF)
    assert ref.rule_limit_app(FLOW, flow_app=3, origin=3) == (K.BLOCK_APP_LIMIT_APP, 3)
    assert ref.rule_limit_app(DEGRADE, origin=2) == (K.BLOCK_APP_LIMIT_APP, 0)           # always "default"
    assert ref.rule_limit_app(AUTHORITY, origin=2) == (K.BLOCK_APP_ORIGIN, 2)            # context.getOrigin()
    # the quirk: SystemBlockException(resourceName, limitType) → super(limitType) = BlockException(ruleLimitApp)
    for kind in (K.SYSTEM_QPS, K.SYSTEM_THREAD, K.SYSTEM_RT, K.SYSTEM_LOAD, K.SYSTEM_CPU):
        assert ref.rule_limit_app(SYSTEM, wait_ms=kind, origin=1) == (K.BLOCK_APP_SYSTEM, kind)
    assert ref.rule_limit_app(PARAM, param_idx=1, args=[5, 77]) == (K.BLOCK_APP_VALUE, 77)
    assert ref.rule_limit_app(PARAM, param_idx=0, args=[None]) == (K.BLOCK_APP_NULL_ARG, 0)
    assert ref.rule_limit_app(PARAM, param_idx=2, args=[5, 77]) == (K.BLOCK_APP_NO_ARG, 0)  # "" for a missing argument
    assert ref.rule_limit_app(PARAM, param_idx=0, args=[("coll", 9)]) == (K.BLOCK_APP_LABEL, 9)
    assert ref.rule_limit_app(PARAM, param_idx=0, args=[("coll", 0)]) == (K.BLOCK_APP_LABEL, 0)


def test_rollup_and_rolling_task():
    log = ref.BlockLog()
    log.stat(T0 + 10, 1, FLOW, 0, 0, 0, 2)
    log.stat(T0 + 999, 1, FLOW, 0, 0, 0, 3)        # the same key and second
    log.stat(T0 + 1000, 1, FLOW, 0, 0, 0, 1)       # the next second
    log.stat(T0 + 20, 0, DEGRADE, 0, 0, 2, 1)
    assert len(log.roll(T0 + 999)) == 0            # the second is not complete
    rows = log.roll(T0 + 1500)
    assert [(int(r["resource"]), int(r["status"]), int(r["count"])) for r in rows] == [(0, DEGRADE, 1), (1, FLOW, 5)]
    assert log.pending() == 1 and len(log.roll(T0 + 1999)) == 0
    assert [int(r["count"]) for r in log.roll(T0 + 2000)] == [1] and log.pending() == 0


def test_line_format():
    rows = np.array([(T0, 5, 0, 0, 0, FLOW, abi.BLOCK_APP_LIMIT_APP),
                     (T0, 2, 0xFFFFFFFF, 0, 2, FLOW, abi.BLOCK_APP_LIMIT_APP),
                     (T0, 1, 1, 0, 1, FLOW, abi.BLOCK_APP_LIMIT_APP),
                     (T0, 7, 0, 1, 1, DEGRADE, abi.BLOCK_APP_LIMIT_APP),
                     (T0, 1, 2, 1, 2, AUTHORITY, abi.BLOCK_APP_ORIGIN),
                     (T0 + 1000, 3, abi.SYSTEM_RT, 1, 0, SYSTEM, abi.BLOCK_APP_SYSTEM),
                     (T0 + 1000, 4, 42, 1, 0, PARAM, abi.BLOCK_APP_VALUE),
                     (T0 + 1000, 1, 0, 1, 0, PARAM, abi.BLOCK_APP_NULL_ARG),
                     (T0 + 1000, 1, 0, 1, 0, PARAM, abi.BLOCK_APP_NO_ARG),
                     (T0 + 1000, 1 << 33, 6, 1, 0, PARAM, abi.BLOCK_APP_LABEL)], abi.BLOCK_ROW_DTYPE)
    lines = metrics.block_log_lines(rows, ["res/a", "res/b"], ["", "appA", "appB"], value_str=lambda v: f"v{v}",
                                    label_str=lambda i: "[1, 2]" if i == 6 else "?", tz=datetime.timezone.utc)
    d0, d1 = "2023-11-14 22:13:20", "2023-11-14 22:13:21"
    assert lines == [f"{d0}|1|res/a,FlowException,default,|5,0\n",
                     f"{d0}|1|res/a,FlowException,other,appB|2,0\n",
                     f"{d0}|1|res/a,FlowException,appA,appA|1,0\n",
                     f"{d0}|1|res/b,DegradeException,default,appA|7,0\n",
                     f"{d0}|1|res/b,AuthorityException,appB,appB|1,0\n",
                     f"{d1}|1|res/b,SystemBlockException,rt,|3,0\n",
                     f"{d1}|1|res/b,ParamFlowException,v42,|4,0\n",
                     f"{d1}|1|res/b,ParamFlowException,null,|1,0\n",
                     f"{d1}|1|res/b,ParamFlowException,,|1,0\n",
                     f"{d1}|1|res/b,ParamFlowException,[1, 2],|{1 << 33},0\n"]


def test_mixed_flow_fails_in_rule_order():
    m = ref.MixedFlow([(0, 4.0, DEFAULT), (0, 1.0, OTHER), (0, 2.0, 1)])
    P = abi.LOCAL_PASS
    # origin 1: its own rule first (2 passes), origin 2: "other" first (1 pass), origin 0: "default" only
    out = [m.entry(T0 + i, 0, o, 1) for i, o in enumerate([1, 1, 1, 2, 2, 0, 0, 1, 2])]
    assert out == [(P, None), (P, None), (FLOW, 1), (P, None), (FLOW, OTHER), (P, None), (FLOW, DEFAULT),
                   (FLOW, 1), (FLOW, OTHER)]


def _oracle_statuses(rules, n_res, n_origins, batches):
    from oracle.binding import local_flow_rule
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(np.array([local_rule() for _ in range(n_res)]))
    fr = np.array([local_flow_rule(r, c, limit_app=a) for r, c, a in rules], abi.LOCAL_FLOW_RULE_DTYPE)
    assert ora.load_flow_rules(fr, n_origins) == len(fr)
    return [ora.decide(ev) for ev in batches]


def test_mixed_trace_model_equals_oracle_and_covers_every_rule():
    batches, decided, model = ref.mixed_case()
    want = _oracle_statuses(ref.MIXED_RULES, ref.MIXED_N_RES, ref.MIXED_N_ORIGINS, batches)
    for ev, (st, app), w in zip(batches, decided, want):
        assert np.array_equal(st, w["status"]) and not w["wait_ms"].any()
    assert model.uniform(0) is None and model.uniform(1) == DEFAULT and model.uniform(2) is None
    ev, (st, app) = batches[0], decided[0]
    first = (ev["ts_ms"] < T0 + 1000) & (ev["resource"] == 0) & (st == FLOW)
    assert {1, OTHER, DEFAULT} <= set(app[first].tolist())        # each of the three rules failed first in one second
    rows, log = ref.mixed_rows(T0 + 1000)
    assert len(rows) >= 8 and log.pending() > 0                    # a second complete, a second open
    assert (st[ev["resource"] == 1] == FLOW).sum() > 64            # the uniform cx resource is saturated


def test_random_trace_model_equals_oracle_and_blocks():
    K, rules, batches, decided = ref.random_case()
    want = _oracle_statuses(rules, K, 4, batches)
    n_block = 0
    apps = set()
    for ev, (st, app), w in zip(batches, decided, want):
        assert np.array_equal(st, w["status"])
        n_block += int((st == FLOW).sum())
        apps |= set(app[st == FLOW].tolist())
    assert n_block > 1000 and {DEFAULT, OTHER, 1, 2, 3, 4} <= apps


def test_wait_trace_has_a_priority_wait_and_flow_blocks():
    base, ev = ref.wait_case()
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(np.array(base))
    st = ora.decide(ev)["status"].tolist()
    assert abi.LOCAL_PASS_WAIT in st and st.count(FLOW) >= 3 and st[:2] == [abi.LOCAL_PASS] * 2


def test_embedded_server_trace_model_equals_oracle_and_both_rules_fail():
    from tests.test_oracle_flow_rules_kat import _server
    fr, ev, st, app = ref.embedded_case()
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(np.array([local_rule()]))
    assert ora.load_flow_rules(fr, 2) == 2
    ora.attach_cluster(_server(float(ref.EMB_SERVER_COUNT)), abi.CLUSTER_SERVER)
    want = ora.decide(ev)
    assert np.array_equal(want["status"], st) and not want["wait_ms"].any()
    blocked = {a for s, a in zip(st, app) if s == FLOW}
    assert blocked == {1, DEFAULT}          # the origin rule and the server's BLOCKED both failed first somewhere
