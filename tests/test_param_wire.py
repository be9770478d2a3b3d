"""CPU checks of the param-flow wire layer: known-answer frames of the builder, the canonical dictionary keys, the
reference decoder's verdict on every malformed shape, and the ABI surface of the new entry points."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from param_frames import RefDecoder, decode_frame, encode_ref, param_frame
from sentinel_amd import abi, param_wire
from sentinel_amd.param_wire import canonical_key, key_value, value_hash

I, L, B, D, F, S, Z, STR = range(8)


def test_known_answer_frame():
    f = param_frame(7, 11, 1, [canonical_key(1, "int"), canonical_key("ab")])
    assert f == bytes.fromhex("00000007" "02" "000000000000000B" "00000001" "00000002" "00" "00000001" "07" "00000002"
                              "6162")
    assert len(f) == 33
    assert decode_frame(f) == (abi.FRAME_PARAM, 7, 11, 1, [(I, b"\x00\x00\x00\x01"), (STR, b"ab")])


@pytest.mark.parametrize("value,cls,hexparam", [
    (-2, "long", "01" "FFFFFFFFFFFFFFFE"),
    (-3, "byte", "02" "FD"),
    (1.5, "double", "03" "3FF8000000000000"),
    (-2.5, "float", "04" "C0200000"),
    (258, "short", "05" "0102"),
    (True, "boolean", "06" "01"),
    (False, "java.lang.Boolean", "06" "00"),
    (-1, "java.lang.Integer", "00" "FFFFFFFF"),
    ("", None, "07" "00000000"),
])
def test_known_answer_per_type(value, cls, hexparam):
    key = canonical_key(value, cls)
    f = param_frame(1, 2, 3, [key])
    assert f == bytes.fromhex("00000001" "02" "0000000000000002" "00000003" "00000001" + hexparam)
    kind, _, _, _, params = decode_frame(f)
    assert kind == abi.FRAME_PARAM and params == [key]
    back = key_value(*key)
    assert back == value and type(back) is type(value)


def test_canonical_keys():
    nan = bytes.fromhex("7FF8000000000000")
    for bits in ("7FF8000000000000", "FFF8000000000001", "7FF0000000000001"):
        assert param_wire.canonical_payload(D, bytes.fromhex(bits)) == nan
    assert param_wire.canonical_payload(D, bytes.fromhex("7FF0000000000000")) == bytes.fromhex("7FF0000000000000")  # +inf
    for bits in ("7FC00000", "FFC00001", "7F800001"):
        assert param_wire.canonical_payload(F, bytes.fromhex(bits)) == bytes.fromhex("7FC00000")
    assert param_wire.canonical_payload(F, bytes.fromhex("FF800000")) == bytes.fromhex("FF800000")  # -inf
    assert canonical_key(float("nan"), "double") == (D, nan)
    assert canonical_key(float("nan"), "float") == (F, bytes.fromhex("7FC00000"))
    assert math.isnan(key_value(D, nan))
    assert param_wire.canonical_payload(Z, b"\x02") == b"\x01" == param_wire.canonical_payload(Z, b"\xff")
    assert param_wire.canonical_payload(Z, b"\x00") == b"\x00"
    assert canonical_key(0.0, "double") != canonical_key(-0.0, "double")
    assert canonical_key(0.0, "float") != canonical_key(-0.0, "float")
    assert canonical_key("TRUE", "boolean") == (Z, b"\x01") and canonical_key("yes", "boolean") == (Z, b"\x00")
    fives = [canonical_key(5, "int"), canonical_key(5, "long"), canonical_key(5, "short"), canonical_key(5, "byte"),
             canonical_key("5"), canonical_key(5.0, "float"), canonical_key("5.0", "double")]
    assert len(set(fives)) == 7
    assert canonical_key("7", "no.such.Class") == (STR, b"7")   # an unknown classType is a String
    with pytest.raises(ValueError):
        param_wire.canonical_payload(I, b"\x00")


def test_reference_dictionary_order_and_identity():
    ref = RefDecoder([11])
    frames = [param_frame(1, 11, 1, [(Z, b"\x02"), (I, b"\0\0\0\5")]),
              param_frame(2, 11, 1, [(Z, b"\x01"), (D, bytes.fromhex("FFF8000000000123")), (L, b"\0" * 7 + b"\5")]),
              param_frame(3, 12, 2, [(D, bytes.fromhex("7FF8000000000000")), (STR, b"")])]
    req, values, xid, kind = ref.decode(frames, [5, 6, 7])
    assert list(values) == [1, 2, 1, 3, 4, 3, 5]
    assert list(req["value_begin"]) == [0, 2, 5] and list(req["value_count"]) == [2, 3, 2]
    assert list(req["key"]) == [0, 0, abi.KEY_NO_RULE] and list(req["acquire"]) == [1, 1, 2]
    assert list(ref.ids) == [(Z, b"\x01"), (I, b"\0\0\0\5"), (D, bytes.fromhex("7FF8000000000000")),
                             (L, b"\0" * 7 + b"\5"), (STR, b"")]


HEAD = struct.pack(">iB", 9, 2)
BODY = struct.pack(">qii", 11, 1, 1)


@pytest.mark.parametrize("frame,kind", [
    (b"", abi.FRAME_SHORT),
    (b"\0\0\0\1", abi.FRAME_SHORT),
    (HEAD, abi.FRAME_NO_DATA),                                                # zero data bytes
    (HEAD + bytes(15), abi.FRAME_NO_DATA),                                    # under 16 data bytes
    (HEAD + struct.pack(">qii", 11, 1, 0) + b"\0\0\0\0\1", abi.FRAME_NO_DATA),   # amount 0
    (HEAD + struct.pack(">qii", 11, 1, -1) + b"\0\0\0\0\1", abi.FRAME_NO_DATA),  # amount negative
    (HEAD + BODY, abi.FRAME_MALFORMED),                                       # amount 1, nothing left
    (HEAD + struct.pack(">qii", 11, 1, 2**31 - 1) + b"\2\1", abi.FRAME_MALFORMED),   # amount > bytes left
    (HEAD + struct.pack(">qii", 11, 1, 2) + b"\2\1", abi.FRAME_MALFORMED),    # runs off the end at a type byte
    (HEAD + BODY + b"\0\0\0\0", abi.FRAME_MALFORMED),                         # INTEGER cut
    (HEAD + BODY + b"\1" + bytes(7), abi.FRAME_MALFORMED),                    # LONG cut
    (HEAD + BODY + b"\2", abi.FRAME_MALFORMED),                               # BYTE cut
    (HEAD + BODY + b"\3" + bytes(7), abi.FRAME_MALFORMED),                    # DOUBLE cut
    (HEAD + BODY + b"\4" + bytes(3), abi.FRAME_MALFORMED),                    # FLOAT cut
    (HEAD + BODY + b"\5\0", abi.FRAME_MALFORMED),                             # SHORT cut
    (HEAD + BODY + b"\6", abi.FRAME_MALFORMED),                               # BOOLEAN cut
    (HEAD + BODY + b"\7\0\0\0", abi.FRAME_MALFORMED),                         # STRING length cut
    (HEAD + BODY + b"\7\0\0\0\3ab", abi.FRAME_MALFORMED),                     # STRING bytes cut
    (HEAD + BODY + b"\7\xff\xff\xff\xffab", abi.FRAME_MALFORMED),             # negative STRING length
    (HEAD + BODY + b"\7\0\0\0\2ab", abi.FRAME_PARAM),
    (HEAD + BODY + b"\7\0\0\0\2abXYZ", abi.FRAME_PARAM),                      # trailing bytes
    (HEAD + BODY + b"\x08", abi.FRAME_PARAM),                                 # an unknown type byte: no parameter
    (struct.pack(">iB", 9, 1) + bytes(13), abi.FRAME_OTHER),                  # a flow frame
    (struct.pack(">iB", 9, 0), abi.FRAME_OTHER),                              # ping
    (struct.pack(">iB", 9, 3) + bytes(30), abi.FRAME_OTHER),                  # concurrent acquire
])
def test_reference_decoder_kinds(frame, kind):
    got = decode_frame(frame)
    assert got[0] == kind
    if frame[-1:] == b"\x08":
        assert got[4] == []   # DefaultTokenService answers BAD_REQUEST for an empty parameter list
    req, values, _, kinds = RefDecoder([11]).decode([frame], [0])
    if kind != abi.FRAME_PARAM:
        assert req["key"][0] == abi.KEY_BAD and req["acquire"][0] == 0 and req["value_count"][0] == 0
        assert len(values) == 0


def test_reference_encoder():
    res = np.zeros(3, abi.RES_DTYPE)
    res["status"] = [abi.BLOCKED, abi.BAD_REQUEST, abi.OK]
    res["remaining"] = [258, -1, 7]
    res["wait_ms"] = [99, 99, 99]
    out = encode_ref(np.array([7, -2, 5], np.int32), np.array([4, 4, 5], np.uint8), res).reshape(3, 16)
    assert bytes(out[0]) == bytes.fromhex("000E" "00000007" "02" "01" "00000102" "00000000")
    assert bytes(out[1]) == bytes.fromhex("000E" "FFFFFFFE" "02" "FC" "FFFFFFFF" "00000000")
    assert not out[2].any()


def test_value_hash_is_a_function_of_the_key():
    assert value_hash(I, b"\0\0\0\5") != value_hash(F, b"\0\0\0\5")
    assert value_hash(STR, b"") != value_hash(STR, b"\0")
    assert value_hash(STR, b"abcdefgh") != value_hash(STR, b"abcdefgh\0")
    assert 0 <= value_hash(STR, b"x" * 100) < 1 << 64


def test_abi_surface():
    assert (abi.FRAME_FLOW, abi.FRAME_SHORT, abi.FRAME_NO_DATA, abi.FRAME_OTHER) == (0, 1, 2, 3)   # not renumbered
    assert (abi.FRAME_PARAM, abi.FRAME_MALFORMED) == (4, 5)
    assert C.sizeof(abi.sg_vdict_config) == 24 and abi.sg_vdict_config.arena_bytes.offset == 8
    assert abi.CPARAM_REQ_DTYPE.itemsize == 24
    from sentinel_amd.engine import EXPORTS, load_library
    L = load_library()
    for name in ["sg_vdict_init", "sg_vdict_intern", "sg_vdict_lookup", "sg_vdict_size", "sg_codec_decode_param",
                 "sg_codec_encode_param"]:
        assert name in EXPORTS
        assert getattr(L, name).argtypes is not None
    text = open(__file__.replace("tests/test_param_wire.py", "include/sentinel_gpu.h")).read()
    for d, v in [("SG_FRAME_PARAM", 4), ("SG_FRAME_MALFORMED", 5), ("SG_PARAM_TYPE_STRING", 7)]:
        assert f"#define {d}" in text and int(text.split(f"#define {d}")[1].split()[0]) == v
