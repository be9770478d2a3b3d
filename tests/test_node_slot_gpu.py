"""The whole slot chain over the node handle (sg_node_slot_decide_batch, sg_node_pslot_load_rules and the node's
readers): G shards of one GPU standing for G GPUs of a node, each event's sg_slot_ext routed with it (k_lroute_*), the
arguments read in place by the shards or compacted per slice (k_lcmp_*, forced for every shard by
SG_NODE_COMPACT_ARGS=1). Every result and the whole chain state must equal one sequential replay by the oracle
(LocalChain + ParamFlowSlot, LocalTraceGen.run_ext); a refused call leaves no trace. All comparisons are exact."""
import functools

import numpy as np
import pytest

from oracle.binding import LocalChain, LocalTraceGen, ParamFlowSlot, degrade_rule, local_flow_rule, local_rule
from sentinel_amd import abi
from sentinel_amd.cluster import local_owners
from tests.test_authority_kat import AuthChecker, random_authority_rules, to_abi
from tests.test_oracle_pslot_kat import QPS, THREAD, rule as prule
from tests.test_slot_chain_gpu import Pool, _compare, _entries, _flow_rules, _param_rules, _run

pytestmark = pytest.mark.gpu

ROUTE_TILE = 4096      # events per tile of the multisplit and of the compaction (node.hip kRouteTile, kCmpTile)
MAX_BATCH = 1 << 14
N_RES, N_ORIGINS, N_CTX = 36, 3, 3
SEED = 1               # chosen on the CPU: the oracle's results of _case(SEED) hold every status _case asserts
T0 = 1_700_000_000_000
KEY = 0x7FFFFFFF


def _code(call, *args):
    from sentinel_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        call(*args)
    return e.value.code


def _rules(seed, n_res=N_RES):
    """Breakers as test_slot_chain_gpu._setup gives them, the mixed flow rules and param rules of one seed."""
    rng = np.random.default_rng(seed)
    base = np.zeros(n_res, abi.LOCAL_RULE_DTYPE)
    for r in range(n_res):
        brk = [degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.3, 1, 5, 1000)] if r % 4 == 0 else []
        base[r] = local_rule(0.0, abi.FLOW_GRADE_NONE, brk)
    flat = [x for r in range(n_res) for x in _flow_rules(rng, r, n_res, N_ORIGINS, N_CTX)]
    rng.shuffle(flat)
    frules = np.array(flat, abi.LOCAL_FLOW_RULE_DTYPE)
    params = _param_rules(rng, n_res)
    return base, frules, params


def _oracle(base, frules, params, n_ctx=N_CTX):
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(base)
    kept = ora.load_flow_rules(frules, N_ORIGINS, n_ctx)
    ps = ParamFlowSlot(params, n_resources=len(base))
    ora.attach_params(ps)
    return ora, ps, kept


def _load(eng, base, frules, params, kept=None, n_ctx=N_CTX):
    eng.local_load_rules(base, 2, 1000, 500)
    k = eng.local_load_flow_rules(frules, N_ORIGINS, n_ctx)
    assert kept is None or k == kept
    if params is not None:
        eng.pslot_load_rules(params, n_resources=len(base))
    return eng


def _node(G, compact, monkeypatch):
    from sentinel_amd.engine import NodeEngine
    if compact:
        monkeypatch.setenv("SG_NODE_COMPACT_ARGS", "1")
    else:
        monkeypatch.delenv("SG_NODE_COMPACT_ARGS", raising=False)
    nd = NodeEngine([0] * G, max_batch=MAX_BATCH)   # the variable is read once, here
    monkeypatch.delenv("SG_NODE_COMPACT_ARGS", raising=False)
    return nd


def _one():
    from sentinel_amd.engine import FlowEngine
    return FlowEngine(device=0, max_batch=MAX_BATCH)


def _draw(rng, pool, n, t, span, n_res=N_RES, n_ctx=N_CTX, **kw):
    ent = _entries(rng, n, n_res, t, span, N_ORIGINS, **kw)
    ext = pool.draw(rng, n)
    ext["context"] = rng.integers(0, max(n_ctx, 1), n)
    args, values = pool.arrays()
    rt = rng.integers(0, 41, n).astype(np.int32)
    er = (rng.random(n) < 0.05).astype(np.uint8)
    return ent, ext, rt, er, args, values


# ---- 1. parity with the oracle

BATCHES = ((9_000, 3000), (9_000, 3000), (4_133, 2000))


@functools.lru_cache(maxsize=None)
def _case(seed, with_auth):
    """The node's rules, its three-batch reference trace and the oracle in its final state (computed once, shared
    by the parameters, never modified)."""
    base, frules, params = _rules(seed)
    auth = random_authority_rules(np.random.default_rng(seed + 7), N_RES) if with_auth else []
    if with_auth:
        chk = AuthChecker(base, frules, params, auth, N_RES, N_ORIGINS, N_CTX)
        ora, ps, kept, gen = chk.ora, chk.ps, chk.kept, chk.gen
    else:
        chk = None
        ora, ps, kept = _oracle(base, frules, params)
        gen = LocalTraceGen(ora)
    rng = np.random.default_rng(seed + 1000)
    pool = Pool()
    t = T0 + int(rng.integers(0, 1000))
    batches = []
    for n, span in BATCHES:
        ent, ext, rt, er, args, values = _draw(rng, pool, n, t, span, zipf=0.9)
        if with_auth:
            ev, xo, want, _ = chk.batch(ent, ext, rt, er, t + span, args, values)
        else:
            ev, xo, want = gen.run_ext(ent, ext, rt, er, t + span, args, values)
        for a in (ev, xo, want, args, values):
            a.setflags(write=False)
        batches.append((ev, xo, args, values, want))
        t += span
    # the shapes the routing and the compaction must meet: the two large batches span more than two tiles, each batch
    # ends in a partial tile and fits the node. (The last batch's 4,133 entries, their exits and those carried over
    # do not reach two tiles with this trace — a blocked entry has no exit: it spans more than one.)
    for i, (ev, *_) in enumerate(batches):
        assert ROUTE_TILE < len(ev) <= MAX_BATCH and len(ev) % ROUTE_TILE != 0, len(ev)
        assert i == 2 or len(ev) > 2 * ROUTE_TILE, len(ev)
    st = np.concatenate([b[4] for b in batches])
    ent_at = np.concatenate([b[0]["kind"] for b in batches]) == abi.LOCAL_ENTRY
    have = set(st["status"][ent_at].tolist())
    need = {abi.LOCAL_PASS, abi.LOCAL_PASS_WAIT, abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_DEGRADE, abi.LOCAL_BLOCK_PARAM}
    if with_auth:
        need |= {abi.LOCAL_BLOCK_AUTHORITY}
    assert need <= have, f"seed {seed}: the oracle's statuses {have} lack {need - have}"
    blockers = np.unique(st["wait_ms"][ent_at & (st["status"] == abi.LOCAL_BLOCK_PARAM)])
    assert len(blockers) >= 2, "BLOCK_PARAM by fewer than two param rules"
    return base, frules, params, auth, kept, ora, ps, chk, pool, batches


def _decide_device(nd, ev, xo, args, values):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
    ev_t, xo_t, a_t, v_t = dev(ev), dev(xo), dev(args), dev(values)
    out_t = torch.empty(len(ev) * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    nd.slot_decide_device(ev_t.data_ptr(), xo_t.data_ptr(), len(ev), a_t.data_ptr(), len(args), v_t.data_ptr(),
                          len(values), out_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out_t.cpu().numpy().view(abi.LOCAL_RES_DTYPE)


@pytest.mark.parametrize("G,mode", [(1, "place"), (2, "place"), (3, "place"), (5, "place"), (3, "compact"),
                                    (3, "device"), (3, "authority"), (3, "authority_compact")])
def test_node_equals_oracle(G, mode, monkeypatch):
    with_auth = mode.startswith("authority")
    base, frules, params, auth, kept, ora, ps, chk, pool, batches = _case(SEED, with_auth)
    nd = _load(_node(G, mode.endswith("compact"), monkeypatch), base, frules, params, kept)
    one = _load(_one(), base, frules, params, kept)
    if with_auth:
        rules, ids = to_abi(auth)
        for e in (nd, one):
            assert e.local_load_authority_rules(rules, ids, N_ORIGINS) == len(auth)
    owners = np.array([nd.local_owner_of(r) for r in range(N_RES)])
    has_rules = np.isin(np.arange(N_RES), params["resource"])
    for b, (ev, xo, args, values, want) in enumerate(batches):
        got = _decide_device(nd, ev, xo, args, values) if mode == "device" else nd.slot_decide_host(ev, xo, args, values)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            i = bad[0]
            raise AssertionError(f"batch {b}: {len(bad)} results differ; first at {i}: ev={ev[i]} ext={xo[i]} "
                                 f"oracle={want[i]} node={got[i]}")
        assert np.array_equal(one.slot_decide_host(ev, xo, args, values), want), f"batch {b}: one handle differs"
        res = ev["resource"] & KEY
        with_args = has_rules[res] & (xo["args_null"] == 0)
        assert len(np.unique(owners[res[with_args]])) >= min(G, 2), "param-rule events reached fewer than two shards"
        assert len(np.unique(owners[res])) == G
    if with_auth:  # (the oracle's controller indices are shifted by the rules the checker added)
        _compare(nd, ora, ps, frules[:0], params, N_RES, N_ORIGINS, N_CTX, pool)
        for i in range(len(frules)):
            w = ora.controller(i + chk.n_added)
            if w is not None:
                assert np.array_equal(w, nd.local_controller(i)), f"controller of rule {i}"
    else:
        _compare(nd, ora, ps, frules, params, N_RES, N_ORIGINS, N_CTX, pool)


# ---- 2. shared and overlapping ranges

@pytest.mark.parametrize("compact", [False, True], ids=["place", "compact"])
def test_shared_and_overlapping_ranges(compact, monkeypatch):
    """Events of resources with different owners naming one arg range, two overlapping ranges (args[0..2) and
    args[1..3)), a COLLECTION sharing its values with a VALUE argument; every exit carries its entry's range."""
    n_res, G = 8, 2
    base = np.zeros(n_res, abi.LOCAL_RULE_DTYPE)
    for r in range(n_res):
        base[r] = local_rule(0.0, abi.FLOW_GRADE_NONE, [])
    frules = np.array([local_flow_rule(r, 100.0) for r in range(n_res)], abi.LOCAL_FLOW_RULE_DTYPE)
    params = np.array([x for r in range(n_res) for x in (prule(res=r, idx=1, count=2.0, grade=THREAD),
                                                         prule(res=r, idx=0, count=3.0, grade=QPS))],
                      abi.PSLOT_RULE_DTYPE)
    ora, ps, kept = _oracle(base, frules, params, n_ctx=0)
    nd = _load(_node(G, compact, monkeypatch), base, frules, params, kept, n_ctx=0)
    a = 0
    b = next(r for r in range(n_res) if nd.local_owner_of(r) != nd.local_owner_of(a))
    values = np.array([5, 6, 7, 9], np.uint64)
    args = np.array([(0, 1, abi.ARG_VALUE, 0),          # values[0]
                     (0, 2, abi.ARG_COLLECTION, 0),     # values[0..2): shares values[0] with the VALUE before it
                     (2, 1, abi.ARG_VALUE, 0),
                     (3, 1, abi.ARG_VALUE, 0)], abi.PSLOT_ARG_DTYPE)
    shapes = [(a, 0, 2), (b, 0, 2), (a, 1, 2), (b, 1, 2), (a, 2, 2), (b, 0, 3), (a, 0, 1), (b, 3, 1)]
    n = 160
    ent = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
    ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
    ent["ts_ms"] = T0 + np.arange(n) * 7
    ent["count"] = 1
    for i in range(n):
        r, ab, ac = shapes[i % len(shapes)]
        ent["resource"][i], ext["arg_begin"][i], ext["arg_count"][i] = r, ab, ac
    rt = (20 + 40 * (np.arange(n) % 5)).astype(np.int32)   # exits interleave with later entries
    ev, xo, want = LocalTraceGen(ora).run_ext(ent, ext, rt, np.zeros(n, np.uint8), T0 + n * 7 - 60, args, values)
    assert (want["status"] == abi.LOCAL_BLOCK_PARAM).any() and (ev["kind"] != abi.LOCAL_ENTRY).any()
    got = nd.slot_decide_host(ev, xo, args, values)
    assert np.array_equal(got, want), f"{(got != want).sum()} results differ"
    counts = [ps.thread_count(r, idx, int(v)) for r in (a, b) for idx in range(3) for v in values]
    assert any(counts), "no entry in flight at the end"
    assert counts == [nd.pslot_thread_count(r, idx, int(v)) for r in (a, b) for idx in range(3) for v in values]
    for ri in range(len(params)):
        for v in values:
            f, lt, tk = ps.token_state(ri, int(v))
            gf, glt, gtk = nd.param_state(ri, int(v))
            assert (gf, glt if f & 1 else 0, gtk if f & 2 else 0) == (f, lt if f & 1 else 0, tk if f & 2 else 0), \
                f"token state of param rule {ri} value {v}"


# ---- 3. routing shapes

@pytest.mark.parametrize("compact", [False, True], ids=["place", "compact"])
def test_routing_shapes(compact, monkeypatch):
    base, frules, params = _rules(SEED)
    ora, ps, kept = _oracle(base, frules, params)
    gen = LocalTraceGen(ora)
    nd = _load(_node(3, compact, monkeypatch), base, frules, params, kept)
    one = _load(_one(), base, frules, params, kept)
    rng = np.random.default_rng(31)
    pool = Pool()

    def step(ent, ext, rt, er, t_end, args, values):
        ev, xo, want = gen.run_ext(ent, ext, rt, er, t_end, args, values)
        assert np.array_equal(nd.slot_decide_host(ev, xo, args, values), want)
        assert np.array_equal(one.slot_decide_host(ev, xo, args, values), want)
        return ev, xo, want

    t = T0
    step(*_draw(rng, pool, 1500, t, 1000)[:4], t + 1000, *pool.arrays())
    t += 1000
    # a second later every exit is due; one entry drains them, then a single event is a batch of its own
    ent, ext, rt, er, args, values = _draw(rng, pool, 1, t + 1999, 1)
    # (its own exit, at most 40 ms of response time after a wait of at most 500 ms, is due in the same call)
    ev, xo, want = gen.run_ext(ent, ext, rt, er, t + 2600, args, values)
    assert gen.pending() == 0
    keep = int(np.nonzero(ev["kind"] == abi.LOCAL_ENTRY)[0][-1])
    for lo, hi in ((0, keep), (keep, keep + 1), (keep + 1, len(ev))):
        assert np.array_equal(nd.slot_decide_host(ev[lo:hi], xo[lo:hi], args, values), want[lo:hi])
        assert np.array_equal(one.slot_decide_host(ev[lo:hi], xo[lo:hi], args, values), want[lo:hi])
    t += 2600
    # every event on one resource with param rules: the other slices are empty
    hot = int(params["resource"][0])
    ent, ext, rt, er, args, values = _draw(rng, pool, 600, t, 400)
    ent["resource"] = hot
    ev, _, _ = step(ent, ext, rt, er, t + 400, args, values)
    assert (ev["resource"] & KEY == hot).all()
    t += 400
    # no event at all: the binding's host form answers it itself, the device form reaches the library (no buffer read)
    assert len(nd.slot_decide_host(ev[:0], xo[:0], args, values)) == 0
    nd.slot_decide_device(0, 0, 0, 0, 0, 0, 0, 0)
    # every args_null == 1
    ent, ext, rt, er, args, values = _draw(rng, pool, 800, t, 500)
    ext["args_null"] = 1
    step(ent, ext, rt, er, t + 500, args, values)
    t += 500
    # ext = None: every event in context 0 with null args, which is local_decide_host (the exits still pending carry
    # their entries' contexts: one more entry far enough ahead drains them first, its own exit too)
    ent, ext, rt, er, args, values = _draw(rng, pool, 1, t + 599, 1)
    step(ent, ext, rt, er, t + 1200, args, values)
    assert gen.pending() == 0
    t += 1200
    ent, ext, rt, er, args, values = _draw(rng, pool, 800, t, 500)
    ext["args_null"], ext["context"], ext["arg_begin"], ext["arg_count"] = 1, 0, 0, 0
    ev, xo, want = gen.run_ext(ent, ext, rt, er, t + 500, args, values)
    half = len(ev) // 2
    assert np.array_equal(nd.slot_decide_host(ev[:half], None, None, None), want[:half])
    assert np.array_equal(nd.local_decide_host(ev[half:]), want[half:])
    assert np.array_equal(one.slot_decide_host(ev, None, None, None), want)
    t += 500
    # an event of a resource >= K whose ext names an arg range past the arrays: answered as one handle answers it
    ent, ext, rt, er, args, values = _draw(rng, pool, 300, t, 200)
    ev, xo, want = gen.run_ext(ent, ext, rt, er, t + 200, args, values)
    at = len(ev) // 2
    stray = ev[at:at + 1].copy()
    stray["resource"], stray["kind"] = N_RES + 3, abi.LOCAL_ENTRY
    sx = np.zeros(1, abi.SLOT_EXT_DTYPE)
    sx["arg_begin"], sx["arg_count"] = len(args) + 5, 4
    ev2, xo2 = np.concatenate([ev[:at], stray, ev[at:]]), np.concatenate([xo[:at], sx, xo[at:]])
    got_one = one.slot_decide_host(ev2, xo2, args, values)
    got = nd.slot_decide_host(ev2, xo2, args, values)
    assert np.array_equal(got, got_one)
    assert np.array_equal(np.delete(got, at), want)
    _compare(nd, ora, ps, frules, params, N_RES, N_ORIGINS, N_CTX, pool)


# ---- 4. refusals leave no trace

def _snapshot(nd):
    return [np.concatenate([np.asarray(a).reshape(-1) for a in nd.local_state(r)]) for r in range(N_RES)]


@pytest.mark.parametrize("compact", [False, True], ids=["place", "compact"])
def test_refusals_leave_no_trace(compact, monkeypatch):
    base, frules, params = _rules(SEED)
    ora, ps, kept = _oracle(base, frules, params)
    gen = LocalTraceGen(ora)
    nd = _load(_node(3, compact, monkeypatch), base, frules, params, kept)
    rng = np.random.default_rng(41)
    pool = Pool()
    ent, ext, rt, er, args, values = _draw(rng, pool, 3000, T0, 1500)
    ev, xo, want = gen.run_ext(ent, ext, rt, er, T0 + 1500, args, values)
    assert np.array_equal(nd.slot_decide_host(ev, xo, args, values), want)
    before = _snapshot(nd)
    # the next batch, two tiles of the multisplit; the oracle sees the valid one only
    ent, ext, rt, er, args, values = _draw(rng, pool, 3500, T0 + 1500, 1500)
    ev, xo, want = gen.run_ext(ent, ext, rt, er, T0 + 3000, args, values)
    assert ROUTE_TILE < len(ev) <= 2 * ROUTE_TILE
    last = len(ev) - 1
    assert (ev["resource"][last] & KEY) < N_RES
    n_args, n_values = len(args), len(values)
    past = np.concatenate([args, np.array([(n_values, 1, abi.ARG_VALUE, 0),
                                           (0xFFFFFFFF, 2, abi.ARG_COLLECTION, 0)], abi.PSLOT_ARG_DTYPE)])

    def bad_ext(**kw):
        x = xo.copy()
        x["args_null"][last] = 0
        for k, v in kw.items():
            x[k][last] = v
        return x

    cases = [("context", ev, bad_ext(context=N_CTX), args, abi.SG_E_INVAL),
             ("arg range", ev, bad_ext(arg_begin=n_args - 1, arg_count=2), args, abi.SG_E_INVAL),
             ("value", ev, bad_ext(arg_begin=n_args, arg_count=1), past, abi.SG_E_INVAL),
             ("collection", ev, bad_ext(arg_begin=n_args + 1, arg_count=1), past, abi.SG_E_INVAL)]
    late = ev.copy()
    late["ts_ms"][last] = late["ts_ms"][last - 1] - 1
    cases.append(("time", late, xo, args, abi.SG_E_TIME))
    for name, e, x, a, code in cases:
        assert _code(nd.slot_decide_host, e, x, a, values) == code, name
        for r, (w, g) in enumerate(zip(before, _snapshot(nd))):
            assert np.array_equal(w, g), f"{name}: the refused batch changed resource {r}"
    assert np.array_equal(nd.slot_decide_host(ev, xo, args, values), want)
    ent, ext, rt, er, args, values = _draw(rng, pool, 2000, T0 + 3000, 1000)
    ev, xo, want = gen.run_ext(ent, ext, rt, er, T0 + 4000, args, values)
    assert np.array_equal(nd.slot_decide_host(ev, xo, args, values), want)
    _compare(nd, ora, ps, frules, params, N_RES, N_ORIGINS, N_CTX, pool)


# ---- 5. the load contract

def _moving_pair(relate, G):
    """A RELATE pair (resource, ref) that gives some resource another owner at G shards."""
    old = local_owners(N_RES, relate, G)
    for a in range(N_RES):
        for b in range(N_RES):
            if a != b and not np.array_equal(local_owners(N_RES, list(relate) + [(a, b)], G), old):
                return a, b
    raise AssertionError("no RELATE pair moves an owner")


def _front_param_idx(nd, rule):
    """sg_pslot_param_idx of the node's front handle (sg_node_front): (return code, paramIdx). The front decides no
    batch, so its paramIdx of a rule is the loaded one; SG_E_INVAL: the front holds no such param rule."""
    import ctypes as C
    front = nd._L.sg_node_front(nd.h)
    assert front
    v = C.c_int32(-99)
    return nd._L.sg_pslot_param_idx(C.c_void_p(front), rule, C.byref(v)), v.value


def test_load_contract(monkeypatch):
    from sentinel_amd.engine import NodeEngine
    G = 3
    base, frules, params = _rules(SEED)
    fresh = NodeEngine([0] * G, max_batch=MAX_BATCH)
    assert _code(fresh.pslot_load_rules, params, None, N_RES) == abi.SG_E_INVAL        # before local_load_rules
    ora, ps, kept = _oracle(base, frules, params)
    nd = _load(_node(G, False, monkeypatch), base, frules, None, kept)
    assert _code(nd.pslot_load_rules, params, None, N_RES + 1) == abi.SG_E_INVAL        # not the node's resource count
    assert _code(nd.pslot_load_rules, params, None, N_RES - 1) == abi.SG_E_INVAL
    bad = params.copy()
    bad["grade"][len(bad) // 2] = 7
    last = len(params) - 1
    front_holds = [(abi.SG_OK, int(params["param_idx"][i])) for i in (0, last)]
    # a load the front refuses on a node without param rules leaves the front without any
    assert _code(nd.pslot_load_rules, bad, None, N_RES) == abi.SG_E_INVAL
    assert _front_param_idx(nd, 0)[0] == abi.SG_E_INVAL and _code(nd.pslot_param_idx, 0) == abi.SG_E_INVAL
    nd.pslot_load_rules(params, n_resources=N_RES)
    assert [_front_param_idx(nd, i) for i in (0, last)] == front_holds
    assert _front_param_idx(nd, last + 1)[0] == abi.SG_E_INVAL
    t, pool, gen = _run(ora, ps, nd, frules, params, N_RES, N_ORIGINS, N_CTX, [(3000, 1500)], 51, compare=False)
    # an invalid rule set is refused by the front: the front and the shards keep their rules, the shards their state
    assert _code(nd.pslot_load_rules, bad, None, N_RES) == abi.SG_E_INVAL
    assert [_front_param_idx(nd, i) for i in (0, last)] == front_holds
    t, pool, gen = _run(ora, ps, nd, frules, params, N_RES, N_ORIGINS, N_CTX, [(3000, 1500)], 52, pool=pool, gen=gen,
                        t=t, compare=False)
    # a flow-rule reload that moves a resource after a slot batch: refused whole, the rules in force stay, and the
    # front (put back on them by a fresh load of every rule set) still holds the param rules
    relate = [(int(r["resource"]), int(r["ref_resource"])) for r in frules if r["strategy"] == abi.STRATEGY_RELATE]
    want_own = [int(x) for x in local_owners(N_RES, relate, G)]
    assert [nd.local_owner_of(r) for r in range(N_RES)] == want_own
    a, b = _moving_pair(relate, G)
    moved = np.concatenate([frules, np.array([local_flow_rule(a, 7.0, strategy=abi.STRATEGY_RELATE, ref=b)],
                                             abi.LOCAL_FLOW_RULE_DTYPE)])
    assert _code(nd.local_load_flow_rules, moved, N_ORIGINS, N_CTX) == abi.SG_E_UNSUPPORTED
    assert [nd.local_owner_of(r) for r in range(N_RES)] == want_own
    assert [_front_param_idx(nd, i) for i in (0, last)] == front_holds
    assert nd.local_load_flow_rules(frules, N_ORIGINS, N_CTX) == ora.load_flow_rules(frules, N_ORIGINS, N_CTX)
    _run(ora, ps, nd, frules, params, N_RES, N_ORIGINS, N_CTX, [(3000, 1500)], 53, pool=pool, gen=gen, t=t)
    # local_load_rules clears the node's param rules: entries a param rule blocked now pass, as in an oracle without
    _load(nd, base, frules, None, kept)
    assert _code(nd.pslot_param_idx, 0) == abi.SG_E_INVAL and _front_param_idx(nd, 0)[0] == abi.SG_E_INVAL
    none =np.zeros(0, abi.PSLOT_RULE_DTYPE)
    ora_p, ps_p, _ = _oracle(base, frules, params)
    ora_n, ps_n, _ = _oracle(base, frules, none)
    rng = np.random.default_rng(54)
    pool = Pool()
    ent, ext, rt, er, args, values = _draw(rng, pool, 3000, T0, 1500)
    _, _, with_p = LocalTraceGen(ora_p).run_ext(ent, ext, rt, er, T0 + 1500, args, values)
    ev, xo, want = LocalTraceGen(ora_n).run_ext(ent, ext, rt, er, T0 + 1500, args, values)
    assert (with_p["status"] == abi.LOCAL_BLOCK_PARAM).any() and not (want["status"] == abi.LOCAL_BLOCK_PARAM).any()
    assert np.array_equal(nd.slot_decide_host(ev, xo, args, values), want)
