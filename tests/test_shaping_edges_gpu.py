"""Parity of the device's WarmUp, RateLimiter and WarmUpRateLimiter controllers (local.hip: warm_cool_down, warm_sync,
warm_qps, pace_step, cx_rule; the lone WarmUp rule's dead periods in cx_wave and k_lwalk_cx; api.cpp make_flow_rule)
with the oracle off the default path: the traces and references of tests/test_shaping_edges_premise.py, whose premises
are asserted again here on what ran. Every result of every batch, every rule's {storedTokens, lastFilledTime,
latestPassedTime} after every batch, and at the end every resource's second, borrow and minute windows and thread
count are compared bit-exactly (test_local_rules_gpu._compare)."""
import numpy as np
import pytest

from oracle.binding import local_rule
from sentinel_amd import abi

import test_shaping_edges_premise as P
from test_local_rules_gpu import WALKERS, _compare, _engine

pytestmark = pytest.mark.gpu


def _load(case, flags=0):
    n = len(case.frules)
    base = np.zeros(n, abi.LOCAL_RULE_DTYPE)
    base[:] = local_rule(0.0, abi.FLOW_GRADE_NONE)
    eng = _engine(flags)
    eng.local_load_rules(base, case.S, case.interval, 500, cold_factor=case.cold)
    assert eng.local_load_flow_rules(case.frules, 0) == n
    return eng


def _decide(case, ref, eng):
    """The reference's batches through the engine, state carried over; returns the controllers after each batch."""
    n = len(case.frules)
    ctls = []
    for b, (ev, want, ctl) in enumerate(ref.outs):
        got = eng.local_decide_host(ev)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            i = bad[0]
            raise AssertionError(f"batch {b}: {len(bad)} results differ; first at {i}: ev={ev[i]} "
                                 f"rule={case.frules[ev[i]['resource'] & abi.KEY_INDEX]} oracle={want[i]} gpu={got[i]}")
        got_ctl = np.array([eng.local_controller(i) for i in range(n)], np.int64)
        assert np.array_equal(got_ctl, ctl), (f"batch {b}: controllers of rules "
                                              f"{np.nonzero((got_ctl != ctl).any(1))[0]} differ:\n{ctl}\nvs\n{got_ctl}")
        ctls.append(got_ctl)
    return ctls


def _check(case, ref, flags=0):
    eng = _load(case, flags)
    ctls = _decide(case, ref, eng)
    _compare(eng, ref.ora, case.frules, len(case.frules), 0)
    return eng, ctls


# ---- 1. cold factor x count x warm-up period

@pytest.mark.parametrize("cold,flags", [(c, 0) for c in P.COLD_FACTORS] +
                         [(5, abi.FLAG_SERIAL_ONLY), (5, abi.FLAG_WAVE_ONLY)])
def test_cold_factor(cold, flags, monkeypatch):
    if flags == 0:
        monkeypatch.setenv("SG_DEBUG", "64")  # the wave walker's counters (local.hip cx_wave; results unchanged)
    case, ref = P.cold_case(cold), P.cold_reference(cold)
    P.premise_cold(case, ref)
    eng, _ = _check(case, ref, flags)
    if flags == 0:  # a lone WarmUp rule's dead periods ran on the wave walker, off the default cold factor
        d = eng.debug_copy(5, np.uint64, 32)
        assert d[20] > 0 and d[23] > 0, f"wave walker segments {d[20]}, dead chunks {d[23]}"


@pytest.mark.parametrize("cold", [0, 1])
def test_cold_factor_at_most_1_is_3(cold):
    """sg_local_config.cold_factor <= 1 given to both sides (SentinelConfig.coldFactor(): the default 3); the device's
    controllers also equal those of a handle loaded with 3 on the same trace."""
    case, ref = P.cold_case(cold), P.cold_reference(cold)
    P.premise_cold(case, ref)
    _, ctls = _check(case, ref)
    three = _decide(case, ref, _load(case._replace(cold=3)))
    assert all(np.array_equal(a, b) for a, b in zip(ctls, three))


# ---- 2. window shapes under warm-up

@pytest.mark.parametrize("S,interval,flags", [(s, i, 0) for s, i in P.SHAPES] +
                         [(2, 3000, abi.FLAG_SERIAL_ONLY), (2, 3000, abi.FLAG_WAVE_ONLY)])
def test_window_shapes_under_warm_up(S, interval, flags):
    case, ref = P.shape_case(S, interval), P.shape_reference(S, interval)
    P.premise_shape(case, ref)
    _check(case, ref, flags)


# ---- 3. time edges

@pytest.mark.parametrize("t0,flags", [(t, 0) for t in P.STARTS] + [(0, abi.FLAG_SERIAL_ONLY), (0, abi.FLAG_WAVE_ONLY)])
def test_time_edges(t0, flags):
    case, ref = P.edge_case(t0), P.edge_reference(t0)
    P.premise_edge(case, ref)
    _check(case, ref, flags)


# ---- 4. large acquires, extreme counts

@pytest.mark.parametrize("flags", WALKERS)
def test_large_acquires_and_extreme_counts(flags):
    case, ref = P.big_case(), P.big_reference()
    P.premise_big(case, ref)
    _check(case, ref, flags)


@pytest.mark.parametrize("flags", WALKERS)
def test_non_positive_acquires(flags):
    """Math.round's negative ties (java_round against a round-half-away llround) in the WarmUpRateLimiter's cost."""
    case, ref = P.nonpos_case(), P.nonpos_reference()
    P.premise_nonpos(case, ref)
    _check(case, ref, flags)
