"""SystemSlot on the device (sg_local_load_system_rules) against the Python model of tests/system_ref.py: plain
resources (the chain is StatisticSlot + SystemSlot, so the model is the whole reference) with one case per limit type
and a mixed one, the serial path forced against the chosen one, a batch whose bound fails although nothing blocks, and
the load / tracking contract. Every comparison is bit-exact. The traces are built once on the CPU; the conditions they
must meet are asserted there (test_traces_meet_their_conditions, no GPU)."""
import functools
import heapq

import numpy as np
import pytest

from oracle.binding import local_flow_rule, local_rule
from sentinel_amd import abi
from tests.system_ref import LIMIT_NAMES, PlainChain, PlainNode, SystemConf

T0 = 1_700_000_000_000
N_RES, INBOUND, N_ORIGINS = 8, [1, 1, 0, 0, 1, 1, 1, 0], 2
SYS = abi.LOCAL_BLOCK_SYSTEM
# entry windows of the three batches: three intervals and more, and a gap longer than the interval before the last
WINDOWS = [(0, 1300), (1300, 2700), (4300, 5600)]


def R(load=-1.0, cpu=-1.0, qps=-1.0, avg_rt=-1, max_thread=-1):
    return (load, cpu, qps, avg_rt, max_thread)


GENEROUS = [R(qps=1e9, max_thread=10 ** 9, avg_rt=10 ** 9)]
# per case: the rules and status of each batch (loaded before it), the limit type it is about, resources with a
# count-0 flow rule, whether events carry origins
CASES = {
    "qps": dict(rules=[[R(qps=150.0)]] * 3, status=(-1.0, -1.0), main=0),
    "thread": dict(rules=[[R(max_thread=20)]] * 3, status=(-1.0, -1.0), main=1),
    "rt": dict(rules=[[R(avg_rt=90)]] * 3, status=(-1.0, -1.0), main=2),
    "load": dict(rules=[[R(load=1.0)]] * 3, status=(2.0, -1.0), main=3),
    "cpu": dict(rules=[[R(cpu=0.5)]] * 3, status=(0.2, 0.7), main=4),
    # a clear first batch, then everything at once; the min of duplicates and an ignored cpu > 1
    "mixed": dict(rules=[GENEROUS, [R(qps=400.0, max_thread=40, avg_rt=400), R(qps=230.0, avg_rt=97, load=1.0, cpu=7.0)],
                         [R(qps=400.0, max_thread=24, avg_rt=400), R(qps=230.0, avg_rt=97, load=1.0, cpu=7.0)]],
                  status=(0.5, 0.99), main=None),
    # checking off (the last rule sets nothing) keeps ENTRY_NODE counting; checking on then blocks at once
    "reload": dict(rules=[[R(qps=40.0), R()], [R(qps=40.0)], [R(qps=40.0), R()]], status=(-1.0, -1.0), main=0),
    # half of the inbound arrivals are FLOW-blocked: the QPS bound (arrivals) fails, the check (passes) never does
    "bound": dict(rules=[[R(qps=300.0)]] * 3, status=(-1.0, -1.0), main=None, flow_zero=(4, 5, 6)),
    "noorigin": dict(rules=[[R(qps=150.0)]] * 3, status=(-1.0, -1.0), main=0, origins=False),
}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(name):
    """The trace of a case and everything the model says about it (computed once, shared, never changed)."""
    spec = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    ch = PlainChain(N_RES, INBOUND, flow_zero=spec.get("flow_zero", ()))
    ch.load, ch.cpu = spec["status"]
    c = Case()
    c.spec, c.batches, c.kinds = spec, [], np.zeros(5, np.int64)
    pending = []  # (exit time, seq, create, res, count, origin, error)
    seq = 0
    for b, (lo, hi) in enumerate(WINDOWS):
        ch.conf = SystemConf(spec["rules"][b])
        ev, want = [], []

        def exits_until(t):
            while pending and pending[0][0] <= t:
                te, _, create, res, count, origin, error = heapq.heappop(pending)
                ch.exit_event(te, create, res, count, origin, error)
                ev.append((te, create, res, count, abi.LOCAL_EXIT_ERROR if error else abi.LOCAL_EXIT, origin))
                want.append((0, 0))

        for t in np.sort(rng.integers(T0 + lo, T0 + hi, 800)):
            t = int(t)
            exits_until(t)
            res = int(rng.integers(0, N_RES))
            origin = int(rng.integers(0, N_ORIGINS + 1)) if res < 4 and spec.get("origins", True) else 0
            count = int(rng.choice([1, 1, 1, 2, 3]))
            st = ch.entry_event(t, res, count, origin)
            ev.append((t, 0, res, count, abi.LOCAL_ENTRY, origin))
            want.append(st)
            if st[0] == SYS:
                c.kinds[st[1]] += 1
            if st[0] == 0:
                seq += 1
                heapq.heappush(pending, (t + int(rng.integers(1, 300)), seq, t, res, count, origin, bool(rng.random() < 0.1)))
        if b == len(WINDOWS) - 1:
            exits_until(1 << 62)
        e = np.zeros(len(ev), abi.LOCAL_EVENT_DTYPE)
        for i, (ts, create, res, count, kind, origin) in enumerate(ev):
            e[i] = (ts, create, res, count, kind, origin)
        w = np.array(want, dtype=abi.LOCAL_RES_DTYPE)
        c.batches.append((e, w, ch.entry.w.dump(), ch.entry.threads))
    c.nodes = {k: (n.sec.dump(), n.mnt.dump(), n.threads) for k, n in ch.nodes.items()}
    return c


def test_traces_meet_their_conditions():
    total = np.zeros(5, np.int64)
    for name, spec in CASES.items():
        c = build(name)
        total += c.kinds
        ev = np.concatenate([b[0] for b in c.batches])
        res = np.concatenate([b[1] for b in c.batches])
        assert 3000 <= len(ev) <= 5000, (name, len(ev))  # about 4,000 events
        entries = ev["kind"] == abi.LOCAL_ENTRY
        assert (res["status"][entries] == 0).mean() >= 0.30, name
        assert np.all(np.diff(ev["ts_ms"]) >= 0)
        assert ev["ts_ms"][-1] - ev["ts_ms"][0] >= 3000
        if spec["main"] is not None:
            assert c.kinds[spec["main"]] >= 5, (name, c.kinds)
    mixed = build("mixed")
    assert mixed.kinds.sum() >= 50 and (mixed.kinds > 0).sum() >= 3, mixed.kinds
    assert not (mixed.batches[0][1]["status"] == SYS).any()
    assert all((total >= 5)), dict(zip(LIMIT_NAMES, total))
    assert build("bound").kinds.sum() == 0
    rel = build("reload")
    assert not (rel.batches[0][1]["status"] == SYS).any() and not (rel.batches[2][1]["status"] == SYS).any()
    first = np.nonzero(rel.batches[1][0]["resource"] < 2)[0]  # resources 0, 1 are inbound
    first = first[rel.batches[1][0]["kind"][first] == abi.LOCAL_ENTRY][0]
    assert rel.batches[1][1]["status"][first] == SYS  # at once, from the window counted with checking off


# ------------------------------------------------------------------------------------------------- the device

def _engine():
    from sentinel_amd.engine import FlowEngine
    return FlowEngine(device=0, max_batch=1 << 16)


def _code(call, *args):
    from sentinel_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        call(*args)
    return e.value.code


def _rules(rows):
    out = np.zeros(len(rows), abi.SYSTEM_RULE_DTYPE)
    for i, (load, cpu, qps, avg_rt, max_thread) in enumerate(rows):
        out[i] = (load, cpu, qps, avg_rt, max_thread)
    return out


def _setup(name, system=True):
    spec = CASES[name]
    eng = _engine()
    fz = spec.get("flow_zero", ())
    eng.local_load_rules(np.array([local_rule() for _ in range(N_RES)]), 2, 1000, 500)
    if spec.get("origins", True):  # (declares the origin ids; the flow rules: count 0 on the resources of flow_zero)
        frules = np.array([local_flow_rule(k, 0.0) for k in fz], dtype=abi.LOCAL_FLOW_RULE_DTYPE).reshape(-1)
        assert eng.local_load_flow_rules(frules, N_ORIGINS, 0) == len(fz)
    eng.local_set_entry_types(INBOUND)
    if system:
        eng.local_set_system_status(*spec["status"])
    return eng


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.asarray(got) != np.asarray(want))
        raise AssertionError(f"{what}: {len(bad)} values differ; first at {bad[0]}: model={np.asarray(want)[tuple(bad[0])]} "
                             f"gpu={np.asarray(got)[tuple(bad[0])]}")


def _run(name, eng, forced=False):
    """Every batch of the case: results, ENTRY_NODE and the path after each; every node at the end."""
    c = build(name)
    paths = []
    for b, (ev, want, entry_sec, entry_thr) in enumerate(c.batches):
        rows = c.spec["rules"][b]
        assert eng.local_load_system_rules(_rules(rows)) == int(SystemConf(rows).check)
        got = eng.local_decide_host(ev)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{name} batch {b}: {len(bad)} results differ; first at {bad[0]}: ev={ev[bad[0]]} "
                                 f"model={want[bad[0]]} gpu={got[bad[0]]}")
        sec, thr = eng.local_entry_node()
        _same(sec, entry_sec, f"{name} batch {b}: ENTRY_NODE window")
        assert thr == entry_thr, (name, b, thr, entry_thr)
        path = eng.local_system_last_path()
        paths.append(path)
        if forced or (want["status"] == SYS).any():
            assert path == 2, (name, b, path)
    empty = PlainNode(2, 1000)
    for res in range(N_RES):
        for origin in [None] + list(range(1, N_ORIGINS + 1)):
            if origin is not None and not c.spec.get("origins", True):
                continue
            sec, bor, mnt, head = eng.local_state(res) if origin is None else eng.local_origin_state(res, origin)
            w_sec, w_mnt, w_thr = c.nodes.get((res, origin), (empty.sec.dump(), empty.mnt.dump(), 0))
            _same(sec, w_sec, f"{name}: second window of {(res, origin)}")
            _same(mnt, w_mnt, f"{name}: minute window of {(res, origin)}")
            assert head[0] == w_thr, (name, res, origin)
            assert np.all(bor[:, 1] == 0)
    return paths


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qps", "thread", "rt", "load", "cpu", "mixed", "reload"])
def test_plain_resources_against_the_model(name):
    paths = _run(name, _setup(name))
    if name in ("mixed", "reload"):
        assert paths[0] == 1  # far under every threshold / checking off: proven clear, the parallel walkers
    if name == "reload":
        assert paths[2] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "qps", "reload", "bound"])
def test_serial_path_forced(name, monkeypatch):
    """SG_SYS_SERIAL=1 (read at handle creation): every batch on the serial path, same results and state — the model
    is what the chosen path was compared with."""
    monkeypatch.setenv("SG_SYS_SERIAL", "1")
    eng = _setup(name)
    monkeypatch.delenv("SG_SYS_SERIAL")
    assert _run(name, eng, forced=True) == [2, 2, 2]


@pytest.mark.gpu
def test_bound_fails_but_nothing_blocks():
    """Arrivals over the QPS threshold, passes under it: the scan cannot prove the batches clear, the serial path
    decides them, and no entry is system-blocked."""
    eng = _setup("bound")
    paths = _run("bound", eng)
    assert 2 in paths, paths
    assert eng.local_system_first_unproven() != 0xFFFFFFFF


@pytest.mark.gpu
def test_far_under_and_over():
    c = build("qps")
    ev = c.batches[0][0]
    eng = _setup("qps")
    assert eng.local_system_last_path() == 0
    assert eng.local_load_system_rules(_rules(GENEROUS)) == 1
    clear = eng.local_decide_host(ev)
    assert eng.local_system_last_path() == 1 and eng.local_system_first_unproven() == 0xFFFFFFFF
    assert not (clear["status"] == SYS).any()
    later = ev.copy()
    later["ts_ms"] += 10_000
    later["create_ts"] += 10_000
    assert eng.local_load_system_rules(_rules([R(qps=5.0)])) == 1
    over = eng.local_decide_host(later)
    assert eng.local_system_last_path() == 2 and (over["status"] == SYS).any()
    first = eng.local_system_first_unproven()
    assert first <= np.nonzero(over["status"] == SYS)[0][0]


@pytest.mark.gpu
def test_contract():
    c = build("qps")
    ev, want = c.batches[0][0], c.batches[0][1]
    # a first load after a batch; reading an untracked ENTRY_NODE
    eng = _setup("qps", system=False)
    assert _code(eng.local_entry_node) == abi.SG_E_INVAL
    plain = eng.local_decide_host(ev)
    assert not (plain["status"] == SYS).any() and eng.local_system_last_path() == 0
    assert _code(eng.local_load_system_rules, _rules([R(qps=150.0)])) == abi.SG_E_UNSUPPORTED
    # sg_local_load_rules drops rules and tracking: the handle then equals one that never heard of system rules
    eng = _setup("qps")
    assert eng.local_load_system_rules(_rules([R(qps=150.0)])) == 1
    _same(eng.local_decide_host(ev), want, "tracked batch")
    again = _setup("qps", system=False)
    for e in (eng,):
        base = np.array([local_rule() for _ in range(N_RES)])
        e.local_load_rules(base, 2, 1000, 500)
        e.local_load_flow_rules(np.zeros(0, abi.LOCAL_FLOW_RULE_DTYPE), N_ORIGINS, 0)
        e.local_set_entry_types(INBOUND)
    assert _code(eng.local_entry_node) == abi.SG_E_INVAL
    a, b = eng.local_decide_host(ev), again.local_decide_host(ev)
    _same(a, b, "after the drop")
    _same(a, plain, "after the drop, against the untracked handle")
    assert eng.local_system_last_path() == 0
    for res in range(N_RES):
        for x, y in zip(eng.local_state(res), again.local_state(res)):
            _same(x, y, f"state of {res} after the drop")
    # tracking can start again on the fresh resources... but not after their first batch
    assert _code(eng.local_load_system_rules, _rules([])) == abi.SG_E_UNSUPPORTED
    # a sharded handle
    sh = _setup("qps")
    assert sh.local_load_system_rules(_rules([R(qps=150.0)])) == 1
    sh.set_shard(0, 2)
    assert _code(sh.local_decide_host, ev) == abi.SG_E_UNSUPPORTED


@pytest.mark.gpu
def test_enqueue_with_tracking_on():
    import torch
    c = build("noorigin")
    eng = _setup("noorigin")
    assert eng.local_load_system_rules(_rules(CASES["noorigin"]["rules"][0])) == 1
    bufs = []
    for ev, want, _, _ in c.batches:
        d_ev = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).copy()).to("cuda")
        d_out = torch.zeros(len(ev) * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        bufs.append((d_ev, d_out, eng.local_enqueue(d_ev.data_ptr(), len(ev), d_out.data_ptr()), want))
    for b, (_, d_out, ticket, want) in enumerate(bufs):
        eng.local_wait(ticket)
        _same(d_out.cpu().numpy().view(abi.LOCAL_RES_DTYPE), want, f"enqueued batch {b}")
    sec, thr = eng.local_entry_node()
    _same(sec, c.batches[-1][2], "ENTRY_NODE after the enqueued batches")
    assert thr == c.batches[-1][3]
