"""Compact records of the binned cluster flow path (BatchArgs::rec4, env SG_REC4): k_prep<true> writes 4 bytes per
request — {bin digit | key in bin | acquire code} at the request's own index — the bin scatter (sort.hip
k_bin_scatter4) widens only the regular bins' records to 8 bytes for k_bin_sort, and the sorted records every walker
reads are 4-byte words {request index | acquire code}, each segment's flowId and end coming from the segment lists.
Every case replays seeded traces through the oracle (ClusterFlowChecker.acquireClusterToken,
srv/flow/ClusterFlowChecker.java:55-112), through the library in compact mode and through it with SG_REC4=0 (8-byte
records throughout): all results and every flowId's window and occupy state must be identical, and so must the sorted
records sg_debug_copy(h, 1, ...) returns (in compact mode an 8-byte view rebuilt from the lists)."""
import numpy as np
import pytest

from sentinel_amd import abi
from test_flow_gpu import (WALKERS, _compare_results, _compare_state, _host_records, _pair, _rules, _trace,
                           assert_stable_partition)

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_011


def _trio(monkeypatch, rules, bin_mode="2", **kw):
    """(compact engine, 8-byte engine, oracle) over the same rules; the switches are read when an engine is created."""
    monkeypatch.setenv("SG_BIN", bin_mode)
    monkeypatch.setenv("SG_REC4", "1")
    eng, ora = _pair(rules, **kw)
    monkeypatch.setenv("SG_REC4", "0")
    eng8, _ = _pair(rules, **kw)
    return eng, eng8, ora


def _step(eng, eng8, ora, req, n_keys):
    out = eng.decide_host(req)
    _compare_results(ora.decide(req), out, req)
    assert np.array_equal(out, eng8.decide_host(req)), "compact and 8-byte records decide differently"
    # the sorted records: the same stable partition by flowId (the order of the hot flowIds' segments depends on the
    # order in which the previous batch's blocks listed them, so only the partition is comparable)
    kshift = np.uint64(64 - max(1, int(n_keys).bit_length()))
    got, got8 = (e.debug_copy(1, np.uint64, len(req)) for e in (eng, eng8))
    assert_stable_partition(got, got8[np.argsort(got8 >> kshift, kind="stable")], int(kshift))
    return out


def _front_codes(req):
    """The acquire code k_prep packs: min(acquire, 127) << 1 | prio (127: the walker re-reads the request)."""
    return ((np.minimum(req["acquire"].astype(np.int64), 127) << 1) | (req["key"] >> 31).astype(np.int64)).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 63, 4097, 60_000])
@pytest.mark.parametrize("n_keys", [1, 7, 300, 5000])
@pytest.mark.parametrize("flags", WALKERS)
def test_forced_bins(monkeypatch, n_keys, n, flags):
    rng = np.random.default_rng(n_keys * 11 + n)
    rules = _rules(n_keys, rng)
    eng, eng8, ora = _trio(monkeypatch, rules, max_batch=1 << 16, flags=flags)
    t = T0
    for _ in range(4):  # the hot set of batch i is batch i-1's longest segments
        req = _trace(rng, n, n_keys, t, int(rng.integers(200, 2500)), zipf=1.2, prio=0.05)
        t = int(req["ts_ms"][-1]) + int(rng.integers(0, 300))
        _step(eng, eng8, ora, req, len(rules))
    _compare_state(eng, ora, rules)
    _compare_state(eng8, ora, rules)


def test_acquire_code_boundary(monkeypatch):
    """Acquire values around the 7-bit field's escape (127), with and without the prioritized bit; the front records
    of both layouts carry the code k_prep is documented to pack."""
    rng = np.random.default_rng(301)
    n_keys, n, max_batch = 40, 20_000, 1 << 16
    rules = _rules(n_keys, rng, counts=rng.integers(100, 4000, n_keys))
    eng, eng8, ora = _trio(monkeypatch, rules, max_batch=max_batch)
    t = T0
    for _ in range(2):
        req = _trace(rng, n, n_keys, t, 1500, prio=0.0)
        edge = rng.random(n) < 0.3
        req["acquire"][edge] = rng.choice(np.array([1, 126, 127, 128, 1000, 2**31 - 1], np.int32), int(edge.sum()))
        req["key"] |= np.where(rng.random(n) < 0.5, np.uint32(abi.KEY_PRIO), np.uint32(0))
        for a in (1, 126, 127, 128, 1000, 2**31 - 1):
            for p in (0, 1):
                assert np.any((req["acquire"] == a) & ((req["key"] >> 31) == p))
        t = int(req["ts_ms"][-1]) + 5
        _step(eng, eng8, ora, req, len(rules))
        c4 = eng.debug_copy(0, np.uint32, n)
        assert np.array_equal(c4 & np.uint32(0xFF), _front_codes(req))
        rec, kshift = _host_records(req, n_keys, max_batch)
        c8 = eng8.debug_copy(0, np.uint64, n)
        assert np.array_equal(c8 >> np.uint64(kshift), rec >> np.uint64(kshift))
        assert np.array_equal(c8 & np.uint64(0xFF), _front_codes(req).astype(np.uint64))
    _compare_state(eng, ora, rules)
    _compare_state(eng8, ora, rules)


def test_segment_lengths_at_class_and_staging_edges(monkeypatch):
    """One flowId each with exactly 4, 5, 16, 17, 32, 33, 64, 65, 256 and 257 records in a batch (the length classes,
    the short walker's staging width and the wave walker's threshold) among 3 000 background flowIds."""
    lens = [4, 5, 16, 17, 32, 33, 64, 65, 256, 257]
    rng = np.random.default_rng(302)
    n_keys, n = 3000 + len(lens), 30_000
    rules = _rules(n_keys, rng)
    eng, eng8, ora = _trio(monkeypatch, rules, max_batch=1 << 16)
    t = T0
    for _ in range(3):  # from the second batch on the 257-record flowId is a hot one
        req = _trace(rng, n, 3000, t, 1200, zipf=0.8, prio=0.05)
        prio = req["key"] & np.uint32(abi.KEY_PRIO)
        key = (req["key"] & np.uint32(abi.KEY_INDEX)) + np.uint32(len(lens))  # background: flowIds 10 .. 3009
        pos = rng.permutation(n)[:sum(lens)]
        key[pos] = np.repeat(np.arange(len(lens), dtype=np.uint32), lens)
        req["key"] = key | prio
        assert [int((key == k).sum()) for k in range(len(lens))] == lens
        t = int(req["ts_ms"][-1]) + 3
        _step(eng, eng8, ora, req, len(rules))
    _compare_state(eng, ora, rules)
    _compare_state(eng8, ora, rules)


def test_large_bin_path(monkeypatch):
    """2^14 flowIds on the default binned path (32 flowIds per regular bin): 30 000 requests on the flowIds of one bin,
    more than k_bin_sort keeps in registers, first with an empty hot table, then with those flowIds hot."""
    rng = np.random.default_rng(303)
    n_keys = 1 << 14
    rules = _rules(n_keys, rng)
    eng, eng8, ora = _trio(monkeypatch, rules, bin_mode="1", max_batch=1 << 16)
    t = T0
    for _ in range(2):
        req = _trace(rng, 40_000, n_keys, t, 1000, zipf=0.5, prio=0.02)
        prio = req["key"] & np.uint32(abi.KEY_PRIO)
        key = req["key"] & np.uint32(abi.KEY_INDEX)
        pos = rng.permutation(len(req))[:30_000]
        key[pos] = 7 * 32 + rng.integers(0, 32, 30_000).astype(np.uint32)
        req["key"] = key | prio
        t = int(req["ts_ms"][-1]) + 11
        _step(eng, eng8, ora, req, len(rules))
    _compare_state(eng, ora, rules, keys=range(0, n_keys, 7))
    _compare_state(eng, ora, rules, keys=range(7 * 32, 8 * 32))
    _compare_state(eng8, ora, rules, keys=range(7 * 32, 8 * 32))


def test_wide_index_falls_back_to_8_byte_records(monkeypatch):
    """max_batch = 2^24 + 4096 needs a 25-bit request index: the binned path runs with 8-byte front records."""
    monkeypatch.setenv("SG_BIN", "2")
    monkeypatch.setenv("SG_REC4", "1")
    rng = np.random.default_rng(304)
    n_keys, n, max_batch = 300, 50_000, (1 << 24) + 4096
    rules = _rules(n_keys, rng)
    eng, ora = _pair(rules, max_batch=max_batch)
    t = T0
    for _ in range(2):
        req = _trace(rng, n, n_keys, t, 1500, zipf=1.2, prio=0.05)
        t = int(req["ts_ms"][-1]) + 9
        _compare_results(ora.decide(req), eng.decide_host(req), req)
        rec, kshift = _host_records(req, n_keys, max_batch)
        front = eng.debug_copy(0, np.uint64, n)
        assert np.array_equal(front >> np.uint64(kshift), rec >> np.uint64(kshift))
        assert np.array_equal(front & np.uint64((1 << 33) - 1), rec & np.uint64((1 << 33) - 1))
    _compare_state(eng, ora, rules)


def test_refused_batch_and_rule_reload(monkeypatch):
    from sentinel_amd.engine import EngineError
    rng = np.random.default_rng(305)
    rules = _rules(2000, rng)
    eng, eng8, ora = _trio(monkeypatch, rules, max_batch=1 << 17)
    t = T0
    req = _trace(rng, 60_000, 2000, t, 800, zipf=1.3)
    _step(eng, eng8, ora, req, len(rules))
    bad = _trace(rng, 1000, 2000, t, 100)
    bad["ts_ms"] = bad["ts_ms"][::-1].copy()  # time-reversed: refused, decides nothing, resets the hot set
    for e in (eng, eng8):
        with pytest.raises(EngineError):
            e.decide_host(bad)
    _compare_state(eng, ora, rules, keys=range(0, 2000, 3))
    t = int(req["ts_ms"][-1]) + 10
    req = _trace(rng, 60_000, 2000, t, 800, zipf=1.3)
    _step(eng, eng8, ora, req, len(rules))
    new = rules[::-1].copy()  # flowIds renumbered: rule index k is another flowId now
    new["count"] = rng.integers(1, 40, len(new))
    for e in (eng, eng8, ora):
        e.load_rules(new)
    for _ in range(2):
        t = int(req["ts_ms"][-1]) + 10
        req = _trace(rng, 60_000, 2000, t, 800, zipf=1.3)
        _step(eng, eng8, ora, req, len(rules))
    _compare_state(eng, ora, new)
    _compare_state(eng8, ora, new)


def test_pipelined_entry(monkeypatch):
    """sg_flow_enqueue: 6 batches of 40 000 requests, 4 in flight, both workspaces, the front half of a batch beside
    the previous batch's walkers."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(306)
    n_keys, n, n_batches = 3000, 40_000, 6
    rules = _rules(n_keys, rng)
    eng, eng8, ora = _trio(monkeypatch, rules, max_batch=n)
    t = T0
    reqs = []
    for _ in range(n_batches):
        reqs.append(_trace(rng, n, n_keys, t, 900, zipf=1.2, prio=0.05))
        t = int(reqs[-1]["ts_ms"][-1]) + 7
    want = [ora.decide(r) for r in reqs]
    for e in (eng, eng8):
        ins = [torch.from_numpy(r.view(np.uint8).copy()).to(dev) for r in reqs]
        outs = [torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in reqs]
        torch.cuda.synchronize()
        tickets = []
        for b in range(n_batches):
            if b >= 4:
                e.wait(tickets[b - 4])
            tickets.append(e.enqueue_device(ins[b].data_ptr(), n, outs[b].data_ptr()))
        for tk in tickets[-4:]:
            e.wait(tk)
        for b in range(n_batches):
            _compare_results(want[b], outs[b].cpu().numpy().view(abi.RES_DTYPE), reqs[b])
        _compare_state(e, ora, rules)
