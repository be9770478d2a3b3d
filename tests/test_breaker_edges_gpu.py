"""Parity of the device's circuit breakers (local.hip: LNode::cb_complete, cb_trips, degrade_blocks, cb_stat_window; the
wave walker's epoch search in lwalk_wave; api.cpp sg_local_load_rules) with the oracle off the default path: the traces
and references of tests/test_breaker_edges_premise.py, whose premises are asserted again here on what ran.

After every batch, under each walker selection, every result (status and wait_ms) and every resource's second window,
borrow array, minute window, thread count and breakers' (state, next_retry, stat_start, bad, total) are compared
bit-exactly with the oracle's state after the same batch (the reads of test_local_gpu._compare). Some cases run once
more through the full-chain walker (context tracking on, sg_slot_decide_batch without ext records) and one through the
pipelined path (sg_local_enqueue). The loader's refusals and accepted bounds follow at the end."""
import numpy as np
import pytest

from oracle.binding import degrade_rule, local_flow_rule, local_rule
from sentinel_amd import abi

import test_breaker_edges_premise as P
from test_local_gpu import WALKERS

pytestmark = pytest.mark.gpu


def _engine(flags=0):
    from sentinel_amd.engine import FlowEngine
    return FlowEngine(device=0, max_batch=1 << 16, flags=flags)


def _same_results(got, want, ev, b):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        i = bad[0]
        raise AssertionError(f"batch {b}: {len(bad)} results differ; first at {i}: ev={ev[i]} oracle={want[i]} "
                             f"gpu={got[i]}")


def _same_state(eng, snap, b):
    for r, (s_o, b_o, m_o, threads, cbs) in enumerate(snap):
        s_g, b_g, m_g, head = eng.local_state(r)
        assert np.array_equal(s_o, s_g), f"batch {b}: second window of {r}:\n{s_o}\nvs\n{s_g}"
        assert np.array_equal(b_o, b_g), f"batch {b}: borrow array of {r}:\n{b_o}\nvs\n{b_g}"
        assert np.array_equal(m_o, m_g), f"batch {b}: minute window of {r} differs at " \
                                         f"{np.nonzero((m_o != m_g).any(1))[0]}"
        assert head[0] == threads, f"batch {b}: threads of {r}: {threads} vs {head[0]}"
        for i, want in enumerate(cbs):
            got = tuple(int(x) for x in head[1 + 6 * i: 6 + 6 * i])
            assert got == want, f"batch {b}: breaker {i} of {r}: {want} vs {got}"


def _check(name, eng, decide):
    ref = P.reference(name)
    for b, (ev, want, snap) in enumerate(ref.outs):
        _same_results(decide(ev), want, ev, b)
        _same_state(eng, snap, b)


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("name", P.NAMES)
def test_breaker_edges(name, flags):
    case = P.case(name)
    P.premise(name)
    eng = _engine(flags)
    eng.local_load_rules(case.rules, case.S, case.interval, 500)
    skipped = 0
    if name == "flow_saturated" and flags == 0:
        eng.enable_stats(True)

    def decide(ev):
        nonlocal skipped
        got = eng.local_decide_host(ev)
        if name == "flow_saturated" and flags == 0:
            skipped += eng.stats()["skipped_ranges"]
        return got
    _check(name, eng, decide)
    if name == "flow_saturated" and flags == 0:
        assert skipped > 0, "no dead period was skipped under an OPEN breaker"


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("name", P.FULL_CHAIN)
def test_breaker_edges_full_chain(name, flags):
    """The same references through the full-chain walker (k_lwalk_cx and its wave walker): the breakers stay in
    sg_local_rule, the flow rules come through sg_local_load_flow_rules with one context tracked, and the batches go
    through sg_slot_decide_batch without ext records (every entry in context 0, no arguments)."""
    case = P.case(name)
    P.premise(name)
    base = case.rules.copy()
    base["flow_grade"], base["flow_count"] = abi.FLOW_GRADE_NONE, 0.0
    frules = np.array([local_flow_rule(r, float(x["flow_count"]), grade=int(x["flow_grade"]))
                       for r, x in enumerate(case.rules) if x["flow_grade"] != abi.FLOW_GRADE_NONE],
                      abi.LOCAL_FLOW_RULE_DTYPE)
    eng = _engine(flags)
    eng.local_load_rules(base, case.S, case.interval, 500)
    assert eng.local_load_flow_rules(frules, 0, 1) == len(frules)
    _check(name, eng, lambda ev: eng.slot_decide_host(ev, None, None, None))


def test_breaker_edges_pipelined():
    """Long response times on the pipelined path: every batch is enqueued before the first wait, so HALF_OPEN crosses
    a batch boundary while the next batch's front half is already running. State reads would drain the pipeline:
    the results of every batch, the state after the last."""
    import torch
    name = P.PIPELINED
    case, ref = P.case(name), P.reference(name)
    P.premise(name)
    eng = _engine()
    eng.local_load_rules(case.rules, case.S, case.interval, 500)
    bufs = []
    for ev, _, _ in ref.outs:
        d_ev = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).copy()).to("cuda")
        d_out = torch.zeros(len(ev) * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        bufs.append((d_ev, d_out, eng.local_enqueue(d_ev.data_ptr(), len(ev), d_out.data_ptr())))
    for b, ((ev, want, _), (_, d_out, ticket)) in enumerate(zip(ref.outs, bufs)):
        eng.local_wait(ticket)
        _same_results(d_out.cpu().numpy().view(abi.LOCAL_RES_DTYPE), want, ev, b)
    _same_state(eng, ref.outs[-1][2], len(ref.outs) - 1)


# ---- the loader: what DegradeRuleManager.isValidRule (:183-202) drops is refused

RT, ER, EC = abi.DEGRADE_RT, abi.DEGRADE_EXCEPTION_RATIO, abi.DEGRADE_EXCEPTION_COUNT
REFUSED = {
    "time_window_0": degrade_rule(ER, 0.3, 0, 5, 1000),
    "time_window_negative": degrade_rule(RT, 20, -1, 5, 1000, 0.5),
    "min_request_amount_0": degrade_rule(EC, 3, 1, 0, 1000),
    "min_request_amount_negative": degrade_rule(ER, 0.3, 1, -5, 1000),
    "slow_ratio_above_1": degrade_rule(RT, 20, 1, 5, 1000, 1.0000000000000002),
    "slow_ratio_negative": degrade_rule(RT, 20, 1, 5, 1000, -0.1),
    "slow_ratio_nan": degrade_rule(RT, 20, 1, 5, 1000, float("nan")),
    "exception_ratio_above_1": degrade_rule(ER, 1.0000000000000002, 1, 5, 1000),
    "stat_interval_0": degrade_rule(ER, 0.3, 1, 5, 0),
    "count_negative": degrade_rule(EC, -1, 1, 5, 1000),
    "count_nan": degrade_rule(RT, float("nan"), 1, 5, 1000, 0.5),
}


def test_invalid_degrade_rules_are_refused_and_the_loaded_rules_stay():
    """One refused load per condition between the batches of a reference: SG_E_INVAL "invalid degrade rule", as the
    first or the second breaker of a resource, and the handle goes on deciding the trace as if nothing had been sent
    (results and state after every batch)."""
    from sentinel_amd.engine import EngineError
    name = "stat300_700"
    case, ref = P.case(name), P.reference(name)
    eng = _engine()
    eng.local_load_rules(case.rules, case.S, case.interval, 500)
    good = degrade_rule(ER, 0.3, 1, 5, 1000)
    items = list(REFUSED.items())
    per_batch = -(-len(items) // len(ref.outs))
    for b, (ev, want, snap) in enumerate(ref.outs):
        for k, (why, bad) in enumerate(items[b * per_batch:(b + 1) * per_batch]):
            rules = case.rules.copy()
            rules[k % len(rules)] = local_rule(5.0, abi.FLOW_GRADE_QPS, [bad, good] if k % 2 else [good, bad])
            with pytest.raises(EngineError) as ei:
                eng.local_load_rules(rules, case.S, case.interval, 500)
            assert ei.value.code == abi.SG_E_INVAL and "invalid degrade rule" in str(ei.value), why
        _same_results(eng.local_decide_host(ev), want, ev, b)
        _same_state(eng, snap, b)
    # an exception count above 1 and an RT count above 1 are no ratios: valid
    eng.local_load_rules(np.array([local_rule(0.0, abi.FLOW_GRADE_NONE, [degrade_rule(EC, 7, 1, 5, 1000),
                                                                         degrade_rule(RT, 7, 1, 5, 1000, 0.5)])]))


def test_boundary_degrade_rules_are_accepted():
    """Window 1, amount 1, slow ratio 0.0 and 1.0, exception ratio 1.0 and 0.0, count 0: isValidRule keeps them. The
    handle then decides a small trace as the oracle does."""
    from oracle.binding import LocalChain, LocalTraceGen
    rules = np.zeros(3, abi.LOCAL_RULE_DTYPE)
    rules[0] = local_rule(0.0, abi.FLOW_GRADE_NONE, [degrade_rule(RT, 20, 1, 1, 1, 0.0), degrade_rule(ER, 1.0, 1, 1, 1)])
    rules[1] = local_rule(0.0, abi.FLOW_GRADE_NONE, [degrade_rule(RT, 0, 1, 1, 1000, 1.0), degrade_rule(ER, 0.0, 1, 1, 7)])
    rules[2] = local_rule(0.0, abi.FLOW_GRADE_NONE, [degrade_rule(EC, 0, 1, 1, 1)])
    eng = _engine()
    eng.local_load_rules(rules)
    ora = LocalChain()
    ora.load_rules(rules)
    rng = np.random.default_rng(5)
    n = 3000
    ent = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
    ent["ts_ms"] = P.T0 + np.sort(rng.integers(0, 2500, n))
    ent["resource"] = rng.integers(0, 3, n)
    ent["count"] = 1
    ev, want = LocalTraceGen(ora).run(ent, rng.integers(0, 41, n).astype(np.int32),
                                      (rng.random(n) < 0.3).astype(np.uint8), P.T0 + 2500)
    assert (want["status"] == abi.LOCAL_BLOCK_DEGRADE).sum() > 100 and (want["status"] == abi.LOCAL_PASS).sum() > 100
    _same_results(eng.local_decide_host(ev), want, ev, 0)
    _same_state(eng, P.snapshot(ora, 3), 0)
