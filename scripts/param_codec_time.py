#!/usr/bin/env python3
"""Times the param-flow wire codec on the trace of `bench_configs.py --workload cparam` sent as frames (DESIGN.md,
"Param-flow wire codec and the value dictionary"). No oracle: tests/test_param_codec_gpu.py checks the results.

The trace: 1000 ClusterParamFlowRules (GLOBAL, count U{1..40}, S = 10 / 1000 ms), rules Zipf(1.0), each rule's values
Zipf(1.1) over 50k distinct values, --events requests per 1000 ms batch, 10 % of them with 2-3 values. Every value
goes on the wire as a STRING of 8-16 bytes (its u64 and a tail), so each one is looked up through the arena. The same
frames are served every second with later timestamps.

  (a) cold decode    sg_codec_decode_param on an empty dictionary: every value of the batch is new
  (b) steady decode  the same call once every value is known
  (c) encode         sg_codec_encode_param
  (d) decide         sg_cparam_decide_batch on the decoded records (the step the codec feeds)

HIP events on the stream around each call, after a warm-up on a small engine that loads every kernel; (b), (c), (d)
are medians over --reps consecutive seconds of one run. sg_codec_decode_param returns after the stream has completed
(it reads the value total and the miss count back), so its events include those two round trips. Prints one JSON
line; target: (b) + (c) <= (d)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_configs import gpu_keys, zipf_cdf  # noqa: E402
from sentinel_amd import abi  # noqa: E402
from sentinel_amd.engine import FlowEngine  # noqa: E402

T0 = 1_700_000_000_000
R, V = 1000, 50_000


def put_be(payload, pos, val, nbytes):
    for k in range(nbytes):
        payload[pos + k] = ((val >> (8 * (nbytes - 1 - k))) & 0xFF).to(torch.uint8)


def build_frames(n, dev, seed=7):
    """→ payload u8, offsets u32[n + 1], ts i64[n], number of values, their payload bytes."""
    rcdf, rperm = zipf_cdf(R, 1.0, 7)
    vcdf, vperm = zipf_cdf(V, 1.1, 8)
    rcdf_t, rperm_t = torch.from_numpy(rcdf).to(dev), torch.from_numpy(rperm.astype(np.int64)).to(dev)
    vcdf_t, vperm_t = torch.from_numpy(vcdf).to(dev), torch.from_numpy(vperm.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    ts = torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values + T0
    key = gpu_keys(rcdf_t, rperm_t, n, gen)
    cnt = torch.where(torch.rand(n, generator=gen, device=dev) < 0.1,
                      torch.randint(2, 4, (n,), generator=gen, device=dev), torch.ones(n, dtype=torch.int64, device=dev))
    begin = torch.cumsum(cnt, 0) - cnt
    nv = int(cnt.sum())
    frame_of = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
    vals = gpu_keys(vcdf_t, vperm_t, nv, gen) * 0x9E3779B1 + key[frame_of] * 0x85EBCA77 + 11
    lens = 8 + vals % 9
    vbytes = 5 + lens                                   # type byte, i32 length, the string
    vstart = torch.cumsum(vbytes, 0) - vbytes
    fbytes = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, frame_of, vbytes)
    flen = 21 + fbytes
    off = torch.cumsum(flen, 0) - flen
    total = int(flen.sum())
    assert total < 2**31
    payload = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
    put_be(payload, off, torch.arange(n, device=dev), 4)                    # xid
    payload[off + 4] = abi.MSG_TYPE_PARAM_FLOW
    put_be(payload, off + 5, key + 1, 8)                                    # flowId (rule k has flowId k + 1)
    put_be(payload, off + 13, torch.ones_like(key), 4)                      # count
    put_be(payload, off + 17, cnt, 4)                                       # amount
    pos = off[frame_of] + 21 + (vstart - vstart[begin][frame_of])
    payload[pos] = abi.PARAM_TYPE_STRING
    put_be(payload, pos + 1, lens, 4)
    for k in range(16):
        m = lens > k
        b = (vals >> (8 * k)) & 0xFF if k < 8 else (vals * 31 + k) & 0xFF
        payload[(pos + 5 + k)[m]] = b[m].to(torch.uint8)
    offsets = torch.cat([off, torch.tensor([total], device=dev)]).to(torch.int32)   # < 2^31: the u32 bit pattern
    return payload, offsets, ts, nv, int(lens.sum())


def rules_of():
    rng = np.random.default_rng(7)
    rules = np.zeros(R, abi.CPARAM_RULE_DTYPE)
    rules["flow_id"] = np.arange(R) + 1
    rules["count"] = rng.integers(1, 41, R)
    rules["threshold_type"] = abi.THRESHOLD_GLOBAL
    rules["sample_count"], rules["window_interval_ms"] = 10, 1000
    return rules


class Server:
    def __init__(self, n, nv, arena_bytes, dev):
        self.eng = FlowEngine(device=0, max_batch=max(n, nv))
        ns = np.zeros(1, abi.NS_DTYPE)
        ns["connected_count"] = 1
        self.eng.set_namespaces(ns)
        self.eng.cparam_load_rules(rules_of(), None, 17)
        cap = 10
        while (1 << cap) < nv:
            cap += 1
        self.eng.vdict_init(cap, arena_bytes, nv)       # sized for a batch of pairwise distinct values
        self.n, self.nv = n, nv
        self.req = torch.empty(n * 24, dtype=torch.uint8, device=dev)
        self.vals = torch.empty(nv * 8, dtype=torch.uint8, device=dev)
        self.xid = torch.empty(n * 4, dtype=torch.uint8, device=dev)
        self.kind = torch.empty(n, dtype=torch.uint8, device=dev)
        self.res = torch.empty(n * 12, dtype=torch.uint8, device=dev)
        self.out = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream

    def decode(self, payload, offsets, ts):
        got = self.eng.codec_decode_param(payload.data_ptr(), offsets.data_ptr(), ts.data_ptr(), self.n,
                                          self.req.data_ptr(), self.vals.data_ptr(), self.nv, self.xid.data_ptr(),
                                          self.kind.data_ptr(), self.st)
        assert got == self.nv

    def decide(self):
        self.eng.cparam_decide_device(self.req.data_ptr(), self.n, self.vals.data_ptr(), self.nv, self.res.data_ptr(),
                                      self.st)

    def encode(self):
        self.eng.codec_encode_param(self.xid.data_ptr(), self.kind.data_ptr(), self.res.data_ptr(), self.n,
                                    self.out.data_ptr(), self.st)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=16_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.init()

    # warm-up: every kernel of the three calls once, on a small engine of its own
    p, o, t, nv, sb = build_frames(50_000, dev, seed=3)
    w = Server(50_000, nv, sb, dev)
    for s in range(2):
        w.decode(p, o, t + 1000 * s)
        w.decide()
        w.encode()
    torch.cuda.synchronize()
    del w

    n = args.events
    payload, offsets, ts, nv, sbytes = build_frames(n, dev)
    srv = Server(n, nv, sbytes, dev)
    cold = event_ms(lambda: srv.decode(payload, offsets, ts))
    distinct, arena = srv.eng.vdict_size()
    srv.decide()
    srv.encode()
    dec, dcd, enc = [], [], []
    for s in range(1, args.reps + 1):
        ts_s = ts + 1000 * s
        dec.append(event_ms(lambda: srv.decode(payload, offsets, ts_s)))
        dcd.append(event_ms(srv.decide))
        enc.append(event_ms(srv.encode))
    assert srv.eng.vdict_size() == (distinct, arena)
    kinds = srv.kind.cpu().numpy()
    assert (kinds == abi.FRAME_PARAM).all()
    # algorithmic bytes. decode: the frames, offsets and timestamps read once, the records, xids, kinds and ids
    # written, and per value one table slot, its entry and its arena bytes; encode: xid, kind, result in, frame out
    b_dec = int(payload.numel()) - 8 + 12 * n + (24 + 4 + 1) * n + 8 * nv + (8 + 24) * nv + sbytes
    b_enc = (4 + 1 + 12 + 16) * n
    d, e, c = float(np.median(dec)), float(np.median(enc)), float(np.median(dcd))
    print(json.dumps({
        "frames": n, "values": nv, "payload_bytes": int(payload.numel()) - 8, "distinct_values": distinct,
        "arena_bytes": arena, "cold_decode_ms": round(cold, 4), "steady_decode": spread(dec), "encode": spread(enc),
        "decide": spread(dcd), "decode_alg_bytes": b_dec, "encode_alg_bytes": b_enc,
        "decode_gbs": round(b_dec / d / 1e6, 1), "encode_gbs": round(b_enc / e / 1e6, 1),
        "codec_over_decide": round((d + e) / c, 4), "target_met": bool(d + e <= c)}))


if __name__ == "__main__":
    main()
