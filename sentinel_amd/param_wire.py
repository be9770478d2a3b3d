"""Param-flow values as the device value dictionary keys them (include/sentinel_gpu.h, sg_vdict_*).

A value's key is (type tag, canonical payload bytes): the payload ParamFlowRequestDataWriter.encodeValue puts on the
wire (big-endian; a STRING's bytes without the length), except BOOLEAN 00 / 01 and one NaN per float width
(Double.equals / Float.equals compare doubleToLongBits / floatToIntBits). canonical_key builds it from a Python value
and the classType of a ParamFlowItem, the way ParamFlowRuleUtil.parseItemValue types a hot item; key_value is the
inverse, for printing sg_cparam_top_values. value_hash mirrors the device hash (pcodec.hip value_hash).
"""
import math
import struct

import numpy as np

from . import abi

_M = (1 << 64) - 1

# ParamFlowItem.classType → type tag: int.class.toString() is "int", Integer.class.getName() "java.lang.Integer"
# (ParamFlowRuleUtil.parseItemValue :220-239). A blank or unknown classType is a String; char has no wire type.
CLASS_TYPES = {
    "int": abi.PARAM_TYPE_INTEGER, "java.lang.Integer": abi.PARAM_TYPE_INTEGER,
    "long": abi.PARAM_TYPE_LONG, "java.lang.Long": abi.PARAM_TYPE_LONG,
    "byte": abi.PARAM_TYPE_BYTE, "java.lang.Byte": abi.PARAM_TYPE_BYTE,
    "double": abi.PARAM_TYPE_DOUBLE, "java.lang.Double": abi.PARAM_TYPE_DOUBLE,
    "float": abi.PARAM_TYPE_FLOAT, "java.lang.Float": abi.PARAM_TYPE_FLOAT,
    "short": abi.PARAM_TYPE_SHORT, "java.lang.Short": abi.PARAM_TYPE_SHORT,
    "boolean": abi.PARAM_TYPE_BOOLEAN, "java.lang.Boolean": abi.PARAM_TYPE_BOOLEAN,
}
_INT_FMT = {abi.PARAM_TYPE_INTEGER: ">i", abi.PARAM_TYPE_LONG: ">q", abi.PARAM_TYPE_BYTE: ">b",
            abi.PARAM_TYPE_SHORT: ">h"}


def type_of_class(class_type) -> int:
    if class_type is None or not str(class_type).strip():
        return abi.PARAM_TYPE_STRING
    if class_type == "char":
        raise ValueError("a char parameter has no cluster wire type (ParamFlowRequestDataWriter drops it)")
    return CLASS_TYPES.get(class_type, abi.PARAM_TYPE_STRING)


def canonical_payload(type_tag: int, payload: bytes) -> bytes:
    """The dictionary's payload for wire payload bytes of a type."""
    payload = bytes(payload)
    size = abi.PARAM_TYPE_SIZE[type_tag]
    if size is not None and len(payload) != size:
        raise ValueError(f"type {type_tag} takes {size} payload bytes, got {len(payload)}")
    if type_tag == abi.PARAM_TYPE_BOOLEAN:
        return b"\x01" if payload != b"\x00" else b"\x00"
    if type_tag == abi.PARAM_TYPE_DOUBLE:
        bits = struct.unpack(">Q", payload)[0]
        if bits & 0x7FFFFFFFFFFFFFFF > 0x7FF0000000000000:
            return struct.pack(">Q", 0x7FF8000000000000)
    if type_tag == abi.PARAM_TYPE_FLOAT:
        bits = struct.unpack(">I", payload)[0]
        if bits & 0x7FFFFFFF > 0x7F800000:
            return struct.pack(">I", 0x7FC00000)
    return payload


def wire_payload(value, type_tag: int) -> bytes:
    """The payload bytes encodeValue writes for a Python value of the given type (no canonicalisation)."""
    if type_tag in _INT_FMT:
        return struct.pack(_INT_FMT[type_tag], int(value))
    if type_tag == abi.PARAM_TYPE_DOUBLE:
        return struct.pack(">d", float(value))
    if type_tag == abi.PARAM_TYPE_FLOAT:
        f = float(value)
        if math.isnan(f):
            return struct.pack(">I", 0x7FC00000)
        if math.isinf(f) or abs(f) > 3.4028235677973366e38:   # (float) of a double past Float.MAX_VALUE is infinite
            return struct.pack(">f", math.copysign(math.inf, f))
        return struct.pack(">f", f)
    if type_tag == abi.PARAM_TYPE_BOOLEAN:
        return b"\x01" if value else b"\x00"
    if type_tag == abi.PARAM_TYPE_STRING:
        return value if isinstance(value, (bytes, bytearray)) else str(value).encode("utf-8")
    raise ValueError(f"unknown parameter type {type_tag}")


def canonical_key(value, class_type=None):
    """(type tag, canonical payload) of a hot item's value. A str value of a numeric classType is parsed as
    parseItemValue does (Integer.parseInt, Boolean.parseBoolean: "true" in any case, …)."""
    t = type_of_class(class_type)
    if isinstance(value, str) and t != abi.PARAM_TYPE_STRING:
        if t == abi.PARAM_TYPE_BOOLEAN:
            value = value.lower() == "true"
        elif t in (abi.PARAM_TYPE_DOUBLE, abi.PARAM_TYPE_FLOAT):
            value = float(value)
        else:
            value = int(value)
    return t, canonical_payload(t, wire_payload(value, t))


def key_value(type_tag: int, payload: bytes):
    """The Python value of a dictionary key (the inverse of canonical_key); a STRING comes back as bytes when it is
    not valid UTF-8."""
    payload = bytes(payload)
    if type_tag in _INT_FMT:
        return struct.unpack(_INT_FMT[type_tag], payload)[0]
    if type_tag == abi.PARAM_TYPE_DOUBLE:
        return struct.unpack(">d", payload)[0]
    if type_tag == abi.PARAM_TYPE_FLOAT:
        return struct.unpack(">f", payload)[0]
    if type_tag == abi.PARAM_TYPE_BOOLEAN:
        return payload != b"\x00"
    if type_tag == abi.PARAM_TYPE_STRING:
        try:
            return payload.decode("utf-8")
        except UnicodeDecodeError:
            return payload
    raise ValueError(f"unknown parameter type {type_tag}")


def pack_keys(keys):
    """[(type tag, payload), ...] → (types u8[n], offsets u32[n + 1], bytes u8) as sg_vdict_intern takes them."""
    keys = list(keys)
    types = np.array([k[0] for k in keys], np.uint8).reshape(-1)
    offsets = np.zeros(len(keys) + 1, np.uint32)
    if keys:
        offsets[1:] = np.cumsum([len(k[1]) for k in keys])
    data = np.frombuffer(b"".join(bytes(k[1]) for k in keys) or b"\x00", np.uint8).copy()
    if len(types) == 0:
        types = np.zeros(1, np.uint8)[:0]
    return types, offsets, data


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def value_hash(type_tag: int, payload: bytes) -> int:
    """The device hash of a canonical key: 8-byte little-endian chunks (the last zero-padded, at least one). The main
    table's home slot of a value is value_hash & (2 * capacity - 1)."""
    payload = bytes(payload)
    h = _mix64(type_tag | (len(payload) << 8))
    for b in range(0, max(len(payload), 1), 8):
        h = _mix64(h ^ int.from_bytes(payload[b:b + 8], "little"))
    return h
