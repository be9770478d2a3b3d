"""Device param-flow codec and value dictionary (sg_codec_decode_param / sg_codec_encode_param / sg_vdict_*,
pcodec.hip) against the pure-Python reference of param_frames.py — kinds, xids, request records, value ids and the
dictionary's contents, all for equality — and the whole server step, frames → decode → sg_cparam_decide_batch →
encode, against reference decode → ClusterTokenService.decide_param → reference encode, byte for byte."""
import struct

import numpy as np
import pytest

from codec_frames import flow_frame, pack
from oracle import binding
from oracle.binding import ClusterTokenService
from param_frames import RefDecoder, encode_ref, param_frame, random_frames, random_value
from sentinel_amd import abi
from sentinel_amd.param_wire import canonical_key, canonical_payload, value_hash

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
I, L, B, D, F, S, Z, STR = range(8)


@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """These tests hand torch device buffers to the library: torch's HIP runtime has to initialise before the
    library's (the order smoke() uses); initialised second it finds no device."""
    import torch
    torch.cuda.init()
    yield


def _ns():
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    ns["max_allowed_qps"] = 30000
    return ns


def _cprules(n, rng):
    r = np.zeros(n, abi.CPARAM_RULE_DTYPE)
    r["flow_id"] = rng.choice(np.arange(1, 50 * n, dtype=np.int64), n, replace=False) * 7919 + 3
    r["count"] = rng.integers(1, 40, n)
    r["threshold_type"] = abi.THRESHOLD_GLOBAL
    r["sample_count"] = 10
    r["window_interval_ms"] = 1000
    return r


def _engine(flow_ids=None, cap_log2=16, arena=1 << 22, max_values=1 << 18, max_batch=1 << 18):
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=max_batch)
    eng.set_namespaces(_ns())
    if flow_ids is not None:
        r = np.zeros(len(flow_ids), abi.CPARAM_RULE_DTYPE)
        r["flow_id"] = flow_ids
        r["count"] = 5
        r["threshold_type"] = abi.THRESHOLD_GLOBAL
        r["sample_count"], r["window_interval_ms"] = 10, 1000
        eng.cparam_load_rules(r, None, 4)
    eng.vdict_init(cap_log2, arena, max_values)
    return eng


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class _Decoded:
    pass


def _decode_gpu(eng, frames, ts, values_cap=None):
    """Device decode of a list of frames → records on the host (and the device tensors, for the server step)."""
    import torch
    payload, offsets = pack(frames)
    n = len(frames)
    p_t = _dev(payload if len(payload) else np.zeros(4, np.uint8))
    o_t, t_t = _dev(offsets), _dev(np.asarray(ts, np.int64) if n else np.zeros(1, np.int64))
    cap = values_cap if values_cap is not None else max(1, int(len(payload)))   # a parameter takes >= 2 bytes
    d = _Decoded()
    d.req_t = torch.zeros(max(n, 1) * abi.CPARAM_REQ_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d.val_t = torch.zeros(max(cap, 1) * 8, dtype=torch.uint8, device="cuda")
    d.xid_t = torch.zeros(max(n, 1) * 4, dtype=torch.uint8, device="cuda")
    d.kind_t = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    d.n_values = eng.codec_decode_param(p_t.data_ptr(), o_t.data_ptr(), t_t.data_ptr(), n, d.req_t.data_ptr(),
                                        d.val_t.data_ptr(), cap, d.xid_t.data_ptr(), d.kind_t.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d.req = d.req_t.cpu().numpy().view(abi.CPARAM_REQ_DTYPE)[:n]
    d.values = d.val_t.cpu().numpy().view(np.uint64)[:d.n_values]
    d.xid = d.xid_t.cpu().numpy().view(np.int32)[:n]
    d.kind = d.kind_t.cpu().numpy()[:n]
    return d


def _assert_decoded(d, want):
    req, values, xid, kind = want
    assert d.n_values == len(values)
    assert np.array_equal(d.kind, kind)
    assert np.array_equal(d.xid, xid)
    if not np.array_equal(d.req, req):
        i = np.nonzero(d.req != req)[0][0]
        raise AssertionError(f"request {i}: {d.req[i]} vs {req[i]}")
    assert np.array_equal(d.values, values)


def _assert_dictionary(eng, ref):
    size, arena = eng.vdict_size()
    assert size == len(ref.ids)
    assert arena == sum(len(p) for _, p in ref.ids if len(p) > 8)
    assert eng.vdict_lookup(np.arange(1, size + 1, dtype=np.uint64)) == list(ref.ids)


@pytest.mark.parametrize("n", [0, 1, 257, 5000, 70_000])
def test_random_frames_match_reference(n):
    rng = np.random.default_rng(100 + n)
    flow_ids = rng.choice(np.arange(1, 10_000, dtype=np.int64), 300, replace=False) * 7919 + 3
    eng, ref = _engine(flow_ids), RefDecoder(flow_ids)
    for b in range(2 if n <= 5000 else 1):   # the second batch meets a filled dictionary
        frames = random_frames(n, flow_ids, rng)
        ts = T0 + 1000 * b + np.sort(rng.integers(0, 1000, n)).astype(np.int64)
        _assert_decoded(_decode_gpu(eng, frames, ts), ref.decode(frames, ts))
        _assert_dictionary(eng, ref)
    if n >= 5000:
        assert len({k for k in ref.ids if k[0] == STR and len(k[1]) >= 300}) > 3   # steps past the LDS stage


def test_dedupe_and_first_appearance_order():
    n = 20_000
    eng, ref = _engine([11], cap_log2=16, max_values=1 << 17), RefDecoder([11])
    three = [(STR, b"a long string value"), (I, struct.pack(">i", 7)), (D, struct.pack(">d", 2.5))]
    ts = np.full(n, T0, np.int64)
    frames = [param_frame(i, 11, 1, three[i % 3:] + three[:i % 3]) for i in range(n)]
    d = _decode_gpu(eng, frames, ts)
    assert eng.vdict_size()[0] == 3
    assert eng.vdict_lookup([1, 2, 3]) == three          # frame 0 holds them in this order
    assert list(d.values[:6]) == [1, 2, 3, 2, 3, 1]
    _assert_decoded(d, ref.decode(frames, ts))
    # pairwise distinct new values, one per frame (long and short payloads): dense ids in frame order
    distinct = [(STR, b"value-%09d" % i) if i % 2 else (L, struct.pack(">q", i * 1_000_003)) for i in range(n)]
    frames = [param_frame(i, 11, 1, [distinct[i]]) for i in range(n)]
    d = _decode_gpu(eng, frames, ts)
    assert np.array_equal(d.values, np.arange(4, n + 4, dtype=np.uint64))
    _assert_decoded(d, ref.decode(frames, ts))
    # a second batch reuses the ids and continues the numbering
    frames = [param_frame(i, 11, 1, [distinct[n - 1 - i], (S, struct.pack(">h", i % 30_000))]) for i in range(n)]
    d = _decode_gpu(eng, frames, ts)
    assert np.array_equal(d.values[0::2], np.arange(n + 3, 3, -1, dtype=np.uint64))
    assert np.array_equal(d.values[1::2], np.arange(n + 4, 2 * n + 4, dtype=np.uint64))
    _assert_decoded(d, ref.decode(frames, ts))
    _assert_dictionary(eng, ref)


def test_value_identity():
    eng = _engine([11])
    fives = [canonical_key(5, "int"), canonical_key(5, "long"), canonical_key(5, "short"), canonical_key(5, "byte"),
             canonical_key("5"), canonical_key(5.0, "float"), canonical_key(5.0, "double")]
    assert list(eng.vdict_intern(fives)) == [1, 2, 3, 4, 5, 6, 7]
    assert list(eng.vdict_intern(fives[::-1])) == [7, 6, 5, 4, 3, 2, 1]
    # on the wire: BOOLEAN 02 is 01, every NaN of a width is one value, the zeros differ, "" is a value
    dn = [bytes.fromhex(x) for x in ("7FF8000000000000", "FFF8000000000001", "7FF0000000000001")]
    fn = [bytes.fromhex(x) for x in ("7FC00000", "FFC00001", "7F800001")]
    ps = [(Z, b"\x02"), (Z, b"\x01"), (Z, b"\x00")] + [(D, x) for x in dn] + [(F, x) for x in fn] + \
         [(D, struct.pack(">d", 0.0)), (D, struct.pack(">d", -0.0)), (F, struct.pack(">f", 0.0)),
          (F, struct.pack(">f", -0.0)), (STR, b""), (STR, b""), (Z, b"\xff")]
    d = _decode_gpu(eng, [param_frame(1, 11, 1, ps[:8]), param_frame(2, 11, 1, ps[8:])], [T0, T0])
    assert list(d.values) == [8, 8, 9, 10, 10, 10, 11, 11, 11, 12, 13, 14, 15, 16, 16, 8]
    assert list(d.kind) == [abi.FRAME_PARAM] * 2 and list(d.req["value_count"]) == [8, 8]
    assert eng.vdict_lookup([8, 10, 11, 16]) == [(Z, b"\x01"), (D, dn[0]), (F, fn[0]), (STR, b"")]
    # the host intern call and the decoder share one dictionary and one canonical form
    assert list(eng.vdict_intern([(F, fn[2]), (Z, b"\x07"), (STR, b""), (STR, b"new")])) == [11, 8, 16, 17]


def test_capacity_is_all_or_nothing():
    eng = _engine([11], cap_log2=6, arena=1 << 16, max_values=4096)
    ints = [(I, struct.pack(">i", i)) for i in range(70)]
    with pytest.raises(Exception) as e:
        _decode_gpu(eng, [param_frame(i, 11, 1, [ints[i]]) for i in range(65)], np.full(65, T0))
    assert e.value.code == abi.SG_E_CAPACITY and eng.vdict_size() == (0, 0)
    d = _decode_gpu(eng, [param_frame(i, 11, 1, [ints[i], ints[i // 2]]) for i in range(64)], np.full(64, T0))
    assert eng.vdict_size() == (64, 0)
    assert list(d.values[0::2]) == [1, 2] + list(range(3, 65)) and list(d.values[1::2]) == [i // 2 + 1 for i in range(64)]
    d = _decode_gpu(eng, [param_frame(9, 11, 1, [ints[63], ints[0]])], [T0])   # known values still decode
    assert list(d.values) == [64, 1]
    with pytest.raises(Exception) as e:
        _decode_gpu(eng, [param_frame(9, 11, 1, [ints[5], ints[64]])], [T0])
    assert e.value.code == abi.SG_E_CAPACITY and eng.vdict_size() == (64, 0)
    with pytest.raises(Exception) as e:
        eng.vdict_intern([ints[66]])
    assert e.value.code == abi.SG_E_CAPACITY and eng.vdict_size() == (64, 0)
    assert eng.vdict_lookup([64, 1]) == [ints[63], ints[0]]


def test_arena_capacity_is_all_or_nothing():
    eng = _engine([11], cap_log2=10, arena=100, max_values=4096)
    strs = [(STR, b"string-%04d" % i) for i in range(12)]   # 11 bytes each
    with pytest.raises(Exception) as e:
        _decode_gpu(eng, [param_frame(i, 11, 1, [strs[i]]) for i in range(10)], np.full(10, T0))
    assert e.value.code == abi.SG_E_CAPACITY and eng.vdict_size() == (0, 0)
    d = _decode_gpu(eng, [param_frame(i, 11, 1, [strs[i], (STR, b"short")]) for i in range(9)], np.full(9, T0))
    assert eng.vdict_size() == (10, 99)   # payloads of at most 8 bytes take no arena
    assert list(d.values) == [1, 2] + [v for i in range(3, 11) for v in (i, 2)]
    assert list(_decode_gpu(eng, [param_frame(1, 11, 1, [strs[8], strs[0]])], [T0]).values) == [10, 1]
    with pytest.raises(Exception) as e:
        _decode_gpu(eng, [param_frame(1, 11, 1, [strs[3], strs[9]])], [T0])
    assert e.value.code == abi.SG_E_CAPACITY and eng.vdict_size() == (10, 99)
    assert list(eng.vdict_intern([(STR, b"tiny"), strs[8]])) == [11, 10]
    assert eng.vdict_lookup([10, 11]) == [strs[8], (STR, b"tiny")]


def test_values_cap_one_short():
    eng = _engine([11])
    frames = [param_frame(i, 11, 1, [(I, struct.pack(">i", i)), (I, struct.pack(">i", i + 1))]) for i in range(300)]
    with pytest.raises(Exception) as e:
        _decode_gpu(eng, frames, np.full(300, T0), values_cap=599)
    assert e.value.code == abi.SG_E_CAPACITY and e.value.n_values == 600
    assert eng.vdict_size() == (0, 0)
    assert _decode_gpu(eng, frames, np.full(300, T0), values_cap=600).n_values == 600
    assert eng.vdict_size() == (301, 0)


def test_argument_errors():
    import torch
    from sentinel_amd.engine import EngineError, FlowEngine
    eng = FlowEngine(device=0, max_batch=1024)
    frame = [param_frame(1, 11, 1, [(I, b"\0\0\0\1")])]
    with pytest.raises(EngineError) as e:      # no dictionary yet
        _decode_gpu(eng, frame, [T0])
    assert e.value.code == abi.SG_E_INVAL
    eng.vdict_init(8, 1 << 12, 1024)
    with pytest.raises(EngineError) as e:      # a dictionary does not grow or restart
        eng.vdict_init(9, 1 << 12, 1024)
    assert e.value.code == abi.SG_E_UNSUPPORTED
    d = _decode_gpu(eng, frame, [T0])          # no param rules loaded: every flowId is unknown
    assert list(d.req["key"]) == [abi.KEY_NO_RULE] and list(d.values) == [1]
    for ids in ([0], [2], [1, 5]):
        with pytest.raises(EngineError) as e:
            eng.vdict_lookup(ids)
        assert e.value.code == abi.SG_E_INVAL
    for keys in ([(I, b"\0\0\1")], [(8, b"")], [(D, b"\0" * 4)]):
        with pytest.raises(EngineError) as e:
            eng.vdict_intern(keys)
        assert e.value.code == abi.SG_E_INVAL
    with pytest.raises(EngineError) as e:      # more values than max_batch_values
        eng.vdict_intern([(S, struct.pack(">h", i)) for i in range(1025)])
    assert e.value.code == abi.SG_E_CAPACITY and eng.vdict_size() == (1, 0)
    payload, offsets = pack(frame * 2)
    p_t = _dev(np.concatenate([np.zeros(1, np.uint8), payload]))
    o_t, t_t = _dev(offsets), _dev(np.array([T0, T0], np.int64))
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    with pytest.raises(EngineError) as e:      # a payload that is not 4-byte aligned
        eng.codec_decode_param(p_t.data_ptr() + 1, o_t.data_ptr(), t_t.data_ptr(), 2, buf.data_ptr(), buf.data_ptr(),
                               8, buf.data_ptr(), buf.data_ptr())
    assert e.value.code == abi.SG_E_INVAL and eng.vdict_size() == (1, 0)


def _colliding_keys(count, slots, homes):
    """`count` distinct LONG keys whose home slots (value_hash & (slots - 1)) fall on `homes` slots only."""
    keys, x = [], 0
    while len(keys) < count:
        k = (L, struct.pack(">q", x))
        if value_hash(*k) & (slots - 1) < homes:
            keys.append(k)
        x += 1
    return keys


def test_long_probe_chains_resolve():
    eng = _engine([11], cap_log2=10, max_values=4096)
    keys = _colliding_keys(1024, 2048, 16)   # 64 keys per home slot on average: chains of hundreds of slots
    assert len({value_hash(*k) & 2047 for k in keys}) <= 16
    order = np.random.default_rng(5).permutation(1024)
    assert list(eng.vdict_intern([keys[i] for i in order[:500]])) == list(range(1, 501))
    frames = [param_frame(i, 11, 1, [keys[order[500 + i]]]) for i in range(524)]
    d = _decode_gpu(eng, frames, np.full(524, T0))
    assert list(d.values) == list(range(501, 1025))
    assert eng.vdict_size() == (1024, 0)                      # filled to capacity
    inv = np.empty(1024, np.int64)
    inv[order] = np.arange(1, 1025)
    assert list(eng.vdict_intern(keys)) == list(inv)          # every lookup still resolves
    d = _decode_gpu(eng, [param_frame(i, 11, 1, [keys[i], keys[1023 - i]]) for i in range(1024)], np.full(1024, T0))
    assert np.array_equal(d.values[0::2], inv.astype(np.uint64)) and np.array_equal(d.values[1::2], inv[::-1].astype(np.uint64))
    assert eng.vdict_lookup(inv[:50]) == keys[:50]


def test_encode_matches_reference():
    import torch
    rng = np.random.default_rng(9)
    n = 100_001
    xid = rng.integers(-2**31, 2**31, n).astype(np.int32)
    kind = rng.choice(np.array([4, 4, 4, 4, 0, 1, 2, 3, 5], np.uint8), n)
    res = np.zeros(n, abi.RES_DTYPE)
    res["status"] = rng.choice(np.array([abi.OK, abi.BLOCKED, abi.TOO_MANY_REQUEST, abi.NO_RULE_EXISTS,
                                         abi.BAD_REQUEST], np.int32), n)
    res["remaining"] = rng.integers(-2**31, 2**31, n)
    res["wait_ms"] = rng.integers(1, 2000, n)
    eng = _engine()
    out_t = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    x_t, k_t, r_t = _dev(xid), _dev(kind), _dev(res)  # kept alive until the kernel has run
    eng.codec_encode_param(x_t.data_ptr(), k_t.data_ptr(), r_t.data_ptr(), n, out_t.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out_t.cpu().numpy()
    assert np.array_equal(got, encode_ref(xid, kind, res))
    g = got.reshape(n, 16)
    assert not g[:, 12:].any()                       # waitInMs 0 although res.wait_ms is not
    assert not g[kind != abi.FRAME_PARAM].any() and (g[kind == abi.FRAME_PARAM, 6] == 2).all()


def test_server_step_end_to_end():
    """frames → device decode → sg_cparam_decide_batch → device encode, over three consecutive 1 s batches."""
    import torch
    from sentinel_amd.engine import FlowEngine
    rng = np.random.default_rng(77)
    R = 200
    rules = _cprules(R, rng)
    pool = [random_value(rng) for _ in range(1500)]
    pool = list(dict.fromkeys((t, canonical_payload(t, p)) for t, p in pool))
    # hot items: the shim types each ParamFlowItem by its classType and names it through the dictionary
    hot_keys = [canonical_key(3, "int"), canonical_key("4", "long"), canonical_key("hot"), canonical_key(2.5, "double"),
                canonical_key("true", "boolean")] + pool[:35]
    eng = FlowEngine(device=0, max_batch=1 << 17)
    eng.set_namespaces(_ns())
    eng.vdict_init(14, 1 << 20, 1 << 17)
    ref = RefDecoder(rules["flow_id"])
    hot_ids = eng.vdict_intern(hot_keys)
    assert np.array_equal(hot_ids, ref.intern(hot_keys))
    hot = np.zeros(60, abi.PARAM_HOT_DTYPE)
    hot["threshold"] = rng.integers(0, 80, 60)
    uniq = np.unique(hot_ids)
    for k in range(20):   # every tenth rule has three hot items (distinct values within a rule)
        hot["value"][3 * k: 3 * k + 3] = rng.choice(uniq, 3, replace=False)
        rules["hot_begin"][10 * k], rules["hot_count"][10 * k] = 3 * k, 3
    eng.cparam_load_rules(rules, hot, 12)
    ora = ClusterTokenService()
    ora.set_namespaces(_ns())
    ora.load_param_rules(rules, hot)
    zipf = 1.0 / np.arange(1, R + 1)
    zipf /= zipf.sum()
    vz = 1.0 / np.arange(1, len(pool) + 1) ** 1.1
    vz /= vz.sum()
    for b in range(3):
        n = int(rng.integers(20_000, 60_000))
        fids = rules["flow_id"][rng.choice(R, n, p=zipf)]
        vidx = rng.choice(len(pool), (n, 3), p=vz)
        u = rng.random((n, 3))
        frames = []
        for i in range(n):
            fid, count = int(fids[i]), 1
            k = 1 if u[i, 0] >= 0.1 else 2 + (u[i, 0] < 0.05)                     # 10 % multi-value
            if u[i, 1] < 0.01:
                fid = int(u[i, 2] * 2**40) + 1                                    # unknown flowId
            elif u[i, 1] < 0.02:
                fid = -int(u[i, 2] * 5)                                           # flowId <= 0
            elif u[i, 1] < 0.03:
                count = -int(u[i, 2] * 3)                                         # count <= 0
            elif u[i, 1] < 0.04:
                count = 2
            ps = [pool[vidx[i, j]] for j in range(k)]
            if u[i, 1] > 0.995:
                ps = [(200, b"")]                                                 # no valid parameter
            frames.append(param_frame(i, fid, count, ps))
        bad = random_frames(40, rules["flow_id"], rng, bad_frac=1.0)              # every rejected shape, too
        for j, f in enumerate(bad):
            frames[(j * 499 + 7) % n] = f
        ts = T0 + b * 1000 + np.sort(rng.integers(0, 1000, n)).astype(np.int64)
        d = _decode_gpu(eng, frames, ts)
        res_t = torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        out_t = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        eng.cparam_decide_device(d.req_t.data_ptr(), n, d.val_t.data_ptr(), d.n_values, res_t.data_ptr(), s)
        eng.codec_encode_param(d.xid_t.data_ptr(), d.kind_t.data_ptr(), res_t.data_ptr(), n, out_t.data_ptr(), s)
        torch.cuda.synchronize()
        want_req, want_values, want_xid, want_kind = ref.decode(frames, ts)
        _assert_decoded(d, (want_req, want_values, want_xid, want_kind))
        want_res = ora.decide_param(want_req, want_values)
        want = encode_ref(want_xid, want_kind, want_res)
        got = out_t.cpu().numpy()
        if not np.array_equal(got, want):
            badi = np.nonzero((got != want).reshape(n, 16).any(axis=1))[0]
            raise AssertionError(f"batch {b}: {len(badi)} response frames differ; first {badi[0]}: "
                                 f"{got.reshape(n, 16)[badi[0]]} vs {want.reshape(n, 16)[badi[0]]}")
        assert (want_res["status"] == abi.OK).any() and (want_res["status"] == abi.BLOCKED).any()
    _assert_dictionary(eng, ref)
    now = int(ts[-1])
    pairs = set()
    for i in rng.permutation(n):
        q = want_req[i]
        if q["key"] < R and q["value_count"] > 0 and q["acquire"] > 0:
            pairs.add((int(q["key"]), int(want_values[q["value_begin"]])))
        if len(pairs) == 50:
            break
    assert len(pairs) == 50
    for k, v in sorted(pairs):
        assert eng.cparam_sum(k, v, now) == ora.param_sum(k, v, now), (k, v)


def test_flow_path_unchanged_on_a_mixed_stream():
    import torch
    rng = np.random.default_rng(4)
    n = 6000
    flow_rules = np.zeros(50, abi.RULE_DTYPE)
    flow_rules["flow_id"] = np.arange(1, 51) * 13
    flow_rules["count"] = 10
    flow_rules["threshold_type"] = abi.THRESHOLD_GLOBAL
    flow_rules["sample_count"], flow_rules["window_interval_ms"] = 10, 1000
    pfids = np.arange(1, 31, dtype=np.int64) * 17
    eng = _engine(pfids)
    eng.load_rules(flow_rules)
    pframes = random_frames(n, pfids, rng, long_strings=False)
    frames = [flow_frame(i, int(flow_rules["flow_id"][i % 50]), 1 + i % 3, i % 7 == 0) if i % 2 else pframes[i]
              for i in range(n)]
    ts = T0 + np.sort(rng.integers(0, 1000, n)).astype(np.int64)
    payload, offsets = pack(frames)
    p_t, o_t, t_t = _dev(payload), _dev(offsets), _dev(ts)
    req_t = torch.empty(n * abi.REQ_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    xid_t = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    kind_t = torch.empty(n, dtype=torch.uint8, device="cuda")
    eng.codec_decode(p_t.data_ptr(), o_t.data_ptr(), t_t.data_ptr(), n, req_t.data_ptr(), xid_t.data_ptr(),
                     kind_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_req, want_xid, want_kind = binding.codec_decode_flow(payload, offsets, ts, flow_rules["flow_id"])
    assert np.array_equal(kind_t.cpu().numpy(), want_kind)
    assert np.array_equal(xid_t.cpu().numpy().view(np.int32), want_xid)
    assert np.array_equal(req_t.cpu().numpy().view(abi.REQ_DTYPE), want_req)
    d = _decode_gpu(eng, frames, ts)
    _assert_decoded(d, RefDecoder(pfids).decode(frames, ts))
    assert (d.kind[1::2] == abi.FRAME_OTHER).all() and (want_kind[1::2] == abi.FRAME_FLOW).all()
    assert (d.kind[0::2] == abi.FRAME_PARAM).sum() > 2000
