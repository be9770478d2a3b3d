"""Parity of the cluster hot-parameter path with the oracle where test_cparam_gpu.py does not reach: sampleCount
11..64 (cp_walk_serial_mem, lanes 10..63 of the wave walker's register ring, 64-wide checkpoints and saves), a rule
reload that changes the ring stride, multi-value requests under a namespace limiter (with the group fallback, and the
deterministic case of a refused request that names a slot nothing saved), and saturated window periods long enough
for several k_cp_skipfill pieces. Every TokenResult and window sum bit-exact; the traces and their premises come
from test_cparam_edges_premise.py, which asserts the premises without a GPU as well."""
import numpy as np
import pytest

from sentinel_amd import abi

import test_cparam_edges_premise as P
from test_cparam_gpu import WALKERS, _check, _compare_sums, _pair

pytestmark = pytest.mark.gpu


def _pair_ns(ns, rules, hot=None, flags=0):
    """_pair with the namespaces given."""
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=1 << 20, flags=flags)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(rules, hot, 12)
    return eng, P.oracle(ns, rules, hot)


# --------------------------------------------------------------------------------------- A. sampleCount 11..64

@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("S,interval", P.SHAPES)
def test_single_value_requests_wide_rings(S, interval, flags):
    """FLAG_SERIAL_ONLY: every slot on cp_walk_serial_mem (ring re-read at every period change, ring[P % S] written
    directly); FLAG_WAVE_ONLY: every slot on the wave walker's register ring, lanes up to S - 1; k_cp_read and k_cp_top
    with the wide stride."""
    rules, batches = P.single_value_case(S, interval)
    eng, ora = _pair(rules, flags=flags)
    for req, vals in batches:
        out = _check(eng, ora, req, vals)
    P.premise_ok_and_blocked(out)
    now = int(req["ts_ms"][-1])
    _compare_sums(eng, ora, req, vals, now)
    top = P.top_values(ora, rules, P.pairs_of(req, vals), now)
    got = eng.cparam_top_values(now, len(rules), 512)
    assert [dict(g) for g in got] == top
    assert all(len(g) == len(t) for g, t in zip(got, top))


@pytest.mark.parametrize("flags", WALKERS)
def test_mixed_sample_counts_one_handle(flags):
    """Rules with S = 2, 10, 11 and 64 in one handle: the register walker and the memory walker side by side on a
    stride of 64."""
    rules, batches = P.mixed_case()
    eng, ora = _pair(rules, flags=flags)
    for req, vals in batches:
        out = _check(eng, ora, req, vals)
        P.premise_ok_and_blocked(out)
        P.premise_multi_blocked(req, out)
        assert eng.cparam_last_rounds() > 1
    _compare_sums(eng, ora, req, vals, int(req["ts_ms"][-1]))


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("S,interval", P.SHAPES)
def test_multi_value_heavy_wide_rings(S, interval, flags):
    """Fixed-point rounds over wide rings: round 0 saves them (cp_prologue before the memory walker), later rounds
    restore them; the first batch resumes hot slots from 64-wide checkpoints, the second (more than 64 window periods)
    re-walks whole segments from the save."""
    rules, batches = P.heavy_case(S, interval)
    spans = [P.periods_spanned(req, interval // S) for req, _ in batches]
    assert spans[0] <= 64 < spans[1]
    eng, ora = _pair(rules, flags=flags)
    for req, vals in batches:
        out = _check(eng, ora, req, vals)
        P.premise_multi_blocked(req, out)
        assert eng.cparam_last_rounds() > 1
        _compare_sums(eng, ora, req, vals, int(req["ts_ms"][-1]))


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("max_rounds", [0, 2])
@pytest.mark.parametrize("S,interval", P.BUDGET_SHAPES)
def test_round_budget_wide_rings(monkeypatch, S, interval, max_rounds, flags):
    """The group fallback over wide rings: from the untouched rings (no round allowed), and after two rounds from the
    saves (k_cpfb_restore with the wide stride)."""
    monkeypatch.setenv("SG_CP_MAX_ROUNDS", str(max_rounds))
    rules, batches = P.budget_case(S, interval)
    eng, ora = _pair(rules, flags=flags)
    serial = 0
    for req, vals in batches:
        P.premise_multi_blocked(req, _check(eng, ora, req, vals))
        r = eng.cparam_last_rounds()
        assert 1 <= r <= max_rounds + 1
        serial += r == max_rounds + 1
    assert serial > 0, "the trace should outlast the round budget"
    _compare_sums(eng, ora, req, vals, int(req["ts_ms"][-1]))


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("S,interval", P.SHAPES)
def test_window_edges_between_batches(S, interval, flags):
    """The oldest bucket exactly at the window's lower edge as a batch opens, then one period past it, and a ring
    that is stale throughout."""
    rules, batches = P.edges_case(S, interval)
    eng, ora = _pair(rules, flags=flags)
    for b, (req, vals) in enumerate(batches):
        if b:
            P.premise_edge_sum(ora, P.EDGE_STEPS[b], batches[b - 1], req)
            _compare_sums(eng, ora, *batches[b - 1], int(req["ts_ms"][0]))
        P.premise_ok_and_blocked(_check(eng, ora, req, vals))
        _compare_sums(eng, ora, req, vals, int(req["ts_ms"][-1]))


# --------------------------------------------------------------------------------------- B. reload, stride 10 <-> 64

@pytest.mark.parametrize("flags", WALKERS)
def test_rule_reload_changes_the_stride(flags):
    """k_cp_copy with ostride != nstride, both ways: the surviving (rule, value) sums right after each reload, every
    result and the sums after each batch."""
    sets, batches = P.stride_case()
    eng, ora = _pair(sets[0], flags=flags)
    for b, (req, vals) in enumerate(batches):
        if b:
            eng.cparam_load_rules(sets[b], None, 12)
            ora.load_param_rules(sets[b])
            now = int(req["ts_ms"][0])
            P.premise_survivors_hold_counts(ora, *batches[b - 1], 8, now)
            _compare_sums(eng, ora, *P.surviving(*batches[b - 1], 8), now)
        P.premise_ok_and_blocked(_check(eng, ora, req, vals))
        _compare_sums(eng, ora, req, vals, int(req["ts_ms"][-1]))


# --------------------------------------------------------------------------------------- C. limiter x multi-value

@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("max_rounds", [None, 0, 1, 2])
@pytest.mark.parametrize("S", [10, 16])
def test_limiter_with_multi_value_requests(monkeypatch, S, max_rounds, flags):
    """Refused requests inside the fixed point and the group fallback: the walkers, k_cp_combine, the group linking
    and the replay all leave them out."""
    if max_rounds is not None:
        monkeypatch.setenv("SG_CP_MAX_ROUNDS", str(max_rounds))
    ns, rules, batches = P.limiter_case(S)
    eng, ora = _pair_ns(ns, rules, flags=flags)
    rounds = []
    for req, vals in batches:
        P.premise_limiter(req, _check(eng, ora, req, vals), rules)
        rounds.append(eng.cparam_last_rounds())
        _compare_sums(eng, ora, req, vals, int(req["ts_ms"][-1]))
    assert min(rounds) > (1 if max_rounds != 0 else 0)  # a let-through multi-value request is BLOCKED in every batch
    if max_rounds is not None:
        assert max_rounds + 1 in rounds, "the trace should outlast the round budget"


@pytest.mark.parametrize("flags", [0, abi.FLAG_SERIAL_ONLY])
def test_refused_request_links_no_slot_into_a_fallback_group(monkeypatch, flags):
    """P.trap_case: the limiter refuses M = (c0, A), the only multi-value request naming A, so the lane walker, which
    saves a short slot's ring only for a counted multi-value record, saves nothing for A. c0 belongs to a chain that
    outlasts the two rounds allowed. Were M to link A to c0's group, k_cpfb_restore would copy an entry into A's ring
    that an earlier batch wrote for another slot (here one with a window sum of 10 or more: every single on A would be
    BLOCKED), and k_cpfb_replay would decide A's requests on it."""
    monkeypatch.setenv("SG_CP_MAX_ROUNDS", "2")
    ns, rules, hot, (b0, b1, trap) = P.trap_case()
    eng, ora = _pair_ns(ns, rules, hot, flags=flags)
    _check(eng, ora, *b0)
    P.premise_trap_setup(ora, b1, _check(eng, ora, *b1))
    assert eng.cparam_last_rounds() == 1
    now = int(trap[0]["ts_ms"][0])
    before = ora.param_sum(0, P.TRAP_A, now)
    assert eng.cparam_sum(0, P.TRAP_A, now) == before
    P.premise_trap(before, *trap, _check(eng, ora, *trap))
    assert eng.cparam_last_rounds() == 3
    now = int(trap[0]["ts_ms"][-1])
    assert eng.cparam_sum(0, P.TRAP_A, now) == ora.param_sum(0, P.TRAP_A, now) == 9
    _compare_sums(eng, ora, *trap, now)


# --------------------------------------------------------------------------------------- D. saturated periods

@pytest.mark.parametrize("flags", [0, abi.FLAG_WAVE_ONLY])
@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("multi", [0.0, 0.05, 0.5])
def test_saturated_periods_of_a_hot_value(multi, limited, flags):
    """Saturated tails of two and more k_cp_skipfill pieces: a multi-value record at the head of a later piece reads
    its predecessor from the piece before; rounds > 0 rewrite BLOCKED results and first-record checks inside the
    ranges; refused lanes stay untouched."""
    ns, rules, (req, vals) = P.saturated_case(multi, limited)
    eng, ora = _pair_ns(ns, rules, flags=flags)
    P.premise_saturated(req, vals, _check(eng, ora, req, vals), multi, limited)
    if multi:
        assert eng.cparam_last_rounds() > 1
    now = int(req["ts_ms"][-1])
    for v in np.unique(vals):
        assert eng.cparam_sum(0, int(v), now) == ora.param_sum(0, int(v), now) > 0


@pytest.mark.parametrize("flags", [0, abi.FLAG_WAVE_ONLY])
def test_saturation_seen_only_by_a_later_round(flags):
    """P.rewrite_case: round 1 stores OK for a thousand singles, and passed checks for the (H, H) requests among them,
    that round 2 finds inside a saturated range of three pieces: k_cp_skipfill's round > 0 branch has to write BLOCKED and
    0 over them. (What a repeated value at the head of a piece carries is not observable through any result: in a
    saturated range its request's first record in the slot checks 0, so the request is BLOCKED either way.)"""
    rules, (req, vals) = P.rewrite_case()
    eng, ora = _pair(rules, flags=flags)
    P.premise_rewrite(req, vals, _check(eng, ora, req, vals))
    assert eng.cparam_last_rounds() > 2
    now = int(req["ts_ms"][-1])
    for v in (P.REWRITE_H, P.REWRITE_Y, P.REWRITE_Z):
        assert eng.cparam_sum(0, v, now) == ora.param_sum(0, v, now) == 1000
