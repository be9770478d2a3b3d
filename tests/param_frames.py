"""Param-flow frames for the codec tests: the builder follows the reference's writers, the decoder is a pure-Python
reading of its server decoders with an insertion-ordered dict as the value dictionary.

Request payload (what the length-field frame decoder hands to NettyRequestDecoder):
  DefaultRequestEntityWriter.writeTo   [i32 xid][u8 type = 2]
  ParamFlowRequestDataWriter.writeTo   [i64 flowId][i32 count][i32 amount] then per parameter [u8 type][payload]
                                       (cli/codec/data/ParamFlowRequestDataWriter.java:48-125)
Server side: DefaultRequestEntityDecoder.decode, ParamFlowRequestDataDecoder.decode / decodeParam
(srv/codec/data/ParamFlowRequestDataDecoder.java:35-90), the response through FlowResponseDataWriter with
waitInMs 0 (ParamFlowRequestProcessor.toResponse). Big-endian throughout.
"""
import struct

import numpy as np

from sentinel_amd import abi
from sentinel_amd.param_wire import canonical_payload

T = abi
SIZES = abi.PARAM_TYPE_SIZE


def param_bytes(type_tag, payload):
    """One parameter on the wire: payload = the value's bytes (a STRING's without the length)."""
    if type_tag == T.PARAM_TYPE_STRING:
        return struct.pack(">Bi", type_tag, len(payload)) + bytes(payload)
    return struct.pack(">B", type_tag) + bytes(payload)


def param_frame(xid, flow_id, count, params, amount=None, trailing=b""):
    """params: [(type tag, payload bytes), ...]; amount defaults to their number."""
    body = struct.pack(">iBqii", xid, T.MSG_TYPE_PARAM_FLOW, flow_id, count, len(params) if amount is None else amount)
    return body + b"".join(param_bytes(t, p) for t, p in params) + trailing


class _Throw(Exception):
    """The Java decoder would throw here: IndexOutOfBoundsException or NegativeArraySizeException."""


def _walk(f, amount):
    """decodeParam `amount` times over frame f from byte 21 → [(type tag, payload)] of the valid parameters."""
    pos, out = 21, []

    def take(k):
        nonlocal pos
        if k < 0 or pos + k > len(f):
            raise _Throw()
        b = f[pos:pos + k]
        pos += k
        return b

    for _ in range(amount):
        t = take(1)[0]
        if t == T.PARAM_TYPE_STRING:
            out.append((t, take(struct.unpack(">i", take(4))[0])))
        elif t < 7:
            out.append((t, take(SIZES[t])))
    return out


def decode_frame(f):
    """→ (kind, xid, flowId, count, [(type tag, payload)])."""
    if len(f) < 5:
        return T.FRAME_SHORT, 0, 0, 0, []
    xid, typ = struct.unpack(">ib", f[:5])
    if typ != T.MSG_TYPE_PARAM_FLOW:
        return T.FRAME_OTHER, xid, 0, 0, []
    if len(f) - 5 < 16:
        return T.FRAME_NO_DATA, xid, 0, 0, []
    fid, count, amount = struct.unpack(">qii", f[5:21])
    if amount <= 0:
        return T.FRAME_NO_DATA, xid, 0, 0, []
    try:
        params = _walk(f, amount) if amount <= len(f) - 21 else None
    except _Throw:
        params = None
    if params is None:   # amount > the bytes left: the loop runs off the end, every parameter takes a byte
        return T.FRAME_MALFORMED, xid, 0, 0, []
    return T.FRAME_PARAM, xid, fid, count, params


class RefDecoder:
    """Reference decoder with its value dictionary: ids 1, 2, 3, … in order of first appearance."""

    def __init__(self, flow_ids=()):
        self.ids = {}    # (type tag, canonical payload) → id, insertion-ordered
        self.rule = {int(f): i for i, f in enumerate(flow_ids)}

    def intern(self, keys):
        out = []
        for t, p in keys:
            out.append(self.ids.setdefault((t, canonical_payload(t, p)), len(self.ids) + 1))
        return np.array(out, np.uint64).reshape(-1)

    def decode(self, frames, ts):
        n = len(frames)
        req = np.zeros(n, abi.CPARAM_REQ_DTYPE)
        xid = np.zeros(n, np.int32)
        kind = np.zeros(n, np.uint8)
        values = []
        for i, f in enumerate(frames):
            k, x, fid, count, params = decode_frame(f)
            kind[i], xid[i] = k, x
            req[i]["ts_ms"] = ts[i]
            req[i]["value_begin"] = len(values)
            if k != T.FRAME_PARAM:
                req[i]["key"] = abi.KEY_BAD
                continue
            req[i]["key"] = abi.KEY_BAD if fid <= 0 else self.rule.get(fid, abi.KEY_NO_RULE)
            req[i]["acquire"] = count
            req[i]["value_count"] = len(params)
            values.extend(int(v) for v in self.intern(params))
        return req, np.array(values, np.uint64).reshape(-1), xid, kind


def encode_ref(xid, kind, res):
    """16-byte response frames: [u16 14][i32 xid][u8 2][u8 status][i32 remaining][i32 0], zeros for other kinds."""
    n = len(xid)
    out = np.zeros((n, 16), np.uint8)
    m = np.asarray(kind) == T.FRAME_PARAM
    out[m, 1] = 14
    out[m, 2:6] = np.asarray(xid, np.int32).astype(">i4").view(np.uint8).reshape(n, 4)[m]
    out[m, 6] = T.MSG_TYPE_PARAM_FLOW
    out[m, 7] = (res["status"].astype(np.int64) & 0xFF).astype(np.uint8)[m]
    out[m, 8:12] = res["remaining"].astype(">i4").view(np.uint8).reshape(n, 4)[m]
    return out.reshape(-1)


def random_value(rng, pool=None):
    """One (type tag, payload): all eight types, strings of 0-60 bytes; with a pool, mostly values from it."""
    if pool is not None and rng.random() < 0.85:
        return pool[int(rng.integers(len(pool)))]
    t = int(rng.integers(0, 8))
    if t == T.PARAM_TYPE_STRING:
        return t, bytes(rng.integers(0, 256, int(rng.integers(0, 61)), dtype=np.uint8))
    if t in (T.PARAM_TYPE_DOUBLE, T.PARAM_TYPE_FLOAT) and rng.random() < 0.3:   # NaNs, zeros, infinities
        hi = int(rng.choice([0x7FF8, 0x7FF0, 0xFFF0, 0x7FFF, 0xFFF8, 0x0000, 0x8000, 0x7FF4]))
        if t == T.PARAM_TYPE_DOUBLE:
            return t, struct.pack(">HHI", hi, 0, int(rng.integers(0, 2)))
        hi = {0x7FF8: 0x7FC0, 0x7FF0: 0x7F80, 0xFFF0: 0xFF80, 0x7FFF: 0x7FFF, 0xFFF8: 0xFFC0, 0x7FF4: 0x7FA0}.get(hi, hi)
        return t, struct.pack(">HH", hi, int(rng.integers(0, 2)))
    if rng.random() < 0.5:   # small numbers: the same digits under several types
        return t, (int(rng.integers(0, 7))).to_bytes(SIZES[t], "big")
    return t, bytes(rng.integers(0, 256, SIZES[t], dtype=np.uint8))


BAD_SHAPES = 14


def bad_frame(shape, xid, fid, rng):
    """One frame of each shape the server decoder rejects, tolerates or leaves to another decoder."""
    val = lambda: random_value(rng)
    head = struct.pack(">iB", xid, T.MSG_TYPE_PARAM_FLOW)
    if shape == 0:    # under 5 bytes
        return bytes(rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8))
    if shape == 1:    # zero data
        return head
    if shape == 2:    # under 16 data bytes
        return head + bytes(rng.integers(0, 256, int(rng.integers(1, 16)), dtype=np.uint8))
    if shape == 3:    # amount 0 or negative
        return param_frame(xid, fid, 1, [val()], amount=int(rng.integers(-3, 1)))
    if shape == 4:    # amount greater than the bytes left
        ps = [val() for _ in range(int(rng.integers(0, 3)))]
        return param_frame(xid, fid, 1, ps, amount=int(rng.choice([len(ps) + 1, 1000, 2**31 - 1])))
    if shape == 5:    # unknown type bytes among valid parameters
        ps = [val(), (int(rng.integers(8, 256)), b""), val(), (int(rng.integers(8, 256)), b"")]
        return param_frame(xid, fid, 1, ps)
    if shape == 6:    # only unknown type bytes: an empty parameter list
        k = int(rng.integers(1, 5))
        return param_frame(xid, fid, 1, [(int(rng.integers(8, 256)), b"") for _ in range(k)])
    if shape == 7:    # a parameter truncated at each field: after the type byte, inside the payload or the length
        whole = param_bytes(*val())   # at least 2 bytes: cut before the type byte, after it, or inside what follows
        return param_frame(xid, fid, 1, [val()], amount=2) + whole[:int(rng.integers(0, len(whole)))]
    if shape == 8:    # negative string length
        return param_frame(xid, fid, 1, [val()], amount=2) + struct.pack(">Bi", 7, -int(rng.integers(1, 100))) + b"abcd"
    if shape == 9:    # string length past the end
        return param_frame(xid, fid, 1, [], amount=1) + struct.pack(">Bi", 7, 9) + b"12345678"
    if shape == 10:   # trailing bytes
        return param_frame(xid, fid, 1, [val()], trailing=bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8)))
    if shape == 11:   # a flow frame
        return struct.pack(">iBqi?", xid, T.MSG_TYPE_FLOW, fid, 1, False)
    if shape == 12:   # a ping or another message type
        return struct.pack(">iB", xid, int(rng.choice([0, 3, 4, 200]))) + bytes(int(rng.integers(0, 24)))
    return param_frame(xid, int(rng.integers(-5, 1)), 1, [val()])   # flowId <= 0


def random_frames(n, flow_ids, rng, bad_frac=0.1, pool_size=500, long_strings=True):
    """n frames: valid param requests (values mostly from a pool, so they repeat; 10 % with 2-4 values; unknown
    flowIds and count <= 0 mixed in), bad_frac of the shapes of bad_frame, and a few strings of 300-900 bytes."""
    known = np.asarray(flow_ids, np.int64)
    pool = [random_value(rng) for _ in range(pool_size)]
    frames = []
    for i in range(n):
        xid = int(rng.integers(-2**31, 2**31))
        fid = int(known[rng.integers(len(known))]) if rng.random() < 0.95 else int(rng.integers(1, 2**62))
        if rng.random() < bad_frac:
            frames.append(bad_frame(i % BAD_SHAPES, xid, fid, rng))
            continue
        k = 1 if rng.random() < 0.9 else int(rng.integers(2, 5))
        ps = [random_value(rng, pool) for _ in range(k)]
        if long_strings and rng.random() < 0.004:
            ps.append((T.PARAM_TYPE_STRING, bytes(rng.integers(0, 256, int(rng.integers(300, 901)), dtype=np.uint8))))
        count = 1 if rng.random() < 0.95 else int(rng.integers(-2, 4))
        frames.append(param_frame(xid, fid, count, ps))
    return frames
