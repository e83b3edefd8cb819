#!/usr/bin/env python3
"""Per-rank kernels of the pipelined MXFP4 op (comm_ops.cpp centralized_pipelined_mxfp4) on
one GPU without the exchange, timed one by one with the kernels' own HIP events
(bagua_time_next_kernels): 1 GiB of fp32 and 2^28 bf16 elements, p = 2, 4 and 8, with 4
uniform, 4 tapered and 8 tapered pieces, interleaved in every repetition with the unpieced
encode, middle step and decode; medians.  Per schedule it reports what the exchange cannot
hide -- the prefix (encode of piece 0) and the suffix (middle step + decode of the last
piece) -- and the sum of all pieces of each kernel against the unpieced launch.

    python tools/mxfp4_pipeline_probe.py [--reps 20] [--log2n 28] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bagua-core_amd"))

DTYPES = (("f32", 0, torch.float32), ("bf16", 2, torch.bfloat16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=28, help="bucket elements, log2")
    ap.add_argument("--out", help="also write the JSON record to this file")
    a = ap.parse_args()
    from bagua_core import _native as N
    K = N.K
    dev = torch.device("cuda", 0)
    n = 1 << a.log2n
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    schedules = (("4_uniform", 4), ("4_tapered", 4 | N.PIECES_TAPERED), ("8_tapered", 8 | N.PIECES_TAPERED))
    out = {"device": torch.cuda.get_device_name(0), "elements": n, "reps": a.reps, "statistic": "median, us",
           "schedules": [s for s, _ in schedules]}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        e1.record(st)
        N.time_next_kernels([(e0, e1)])
        N.check(call(), "kernel")
        torch.cuda.synchronize()
        N.check(K.bagua_time_next_kernels(None, None, 0), "disarm")
        return e0.elapsed_time(e1) * 1e3

    def median(v):
        v = sorted(v)
        return v[len(v) // 2]

    for name, dt, tdt in DTYPES:
        g = torch.Generator(device=dev).manual_seed(3)
        x = (torch.randn(n, device=dev, generator=g) * 1e-3).to(tdt)
        y = torch.empty_like(x)
        xp, yp = x.data_ptr(), y.data_ptr()
        for p in (2, 4, 8):
            cs = n // p
            r = p - 1
            S = K.bagua_mxfp4_compressed_bytes(cs, p)
            send = torch.empty(S, dtype=torch.uint8, device=dev)
            N.check(K.bagua_mxfp4_compress(dt, xp, n, cs, p, send.data_ptr(), S, -1, sp), "encode")
            # the received buffer: a copy of this rank's segments stands in for the peers'
            recv = send.clone()
            cp, rp = send.data_ptr(), recv.data_ptr()

            def ranges(sched):
                b, e = ctypes.c_int(), ctypes.c_int()
                rs = []
                for q in range(sched & N.PIECES_COUNT_MASK):
                    N.check(K.bagua_mxfp4_piece_range(cs, sched, q, ctypes.byref(b), ctypes.byref(e)), "range")
                    if e.value > b.value:
                        rs.append((b.value, e.value))
                return rs

            rs = {s: ranges(sched) for s, sched in schedules}
            whole = {"encode": [], "middle": [], "decode": []}
            piece = {s: {k: [[] for _ in rs[s]] for k in whole} for s, _ in schedules}
            for _ in range(a.reps):  # everything interleaved in every repetition
                whole["encode"].append(timed(lambda: K.bagua_mxfp4_compress(dt, xp, n, cs, p, cp, S, -1, sp)))
                whole["middle"].append(timed(lambda: K.bagua_mxfp4_reduce_requantize(dt, rp, S, cs, p, None, 1, cp, S, r,
                                                                                     sp)))
                whole["decode"].append(timed(lambda: K.bagua_mxfp4_decompress(dt, cp, S, cs, p, yp, sp)))
                for s, _ in schedules:  # the op's order: every E, then every M, then every D
                    for q, (b, e) in enumerate(rs[s]):
                        piece[s]["encode"][q].append(timed(
                            lambda: K.bagua_mxfp4_compress_range(dt, xp, n, cs, p, cp, S, b, e, sp)))
                    for q, (b, e) in enumerate(rs[s]):
                        piece[s]["middle"][q].append(timed(
                            lambda: K.bagua_mxfp4_reduce_requantize_range(dt, rp, S, cs, p, 1, cp, S, r, b, e, sp)))
                    for q, (b, e) in enumerate(rs[s]):
                        piece[s]["decode"][q].append(timed(
                            lambda: K.bagua_mxfp4_decompress_range(dt, cp, S, cs, p, yp, b, e, sp)))
            row = {"chunk_elements": cs, "segment_bytes": S // p,
                   "unpieced_us": {k: round(median(v), 1) for k, v in whole.items()}}
            for s, _ in schedules:
                us = {k: [round(median(v), 1) for v in piece[s][k]] for k in whole}
                row[s] = {
                    "piece_blocks": [e - b for b, e in rs[s]],
                    "encode_piece_us": us["encode"], "middle_piece_us": us["middle"], "decode_piece_us": us["decode"],
                    "prefix_us": us["encode"][0],
                    "suffix_us": round(us["middle"][-1] + us["decode"][-1], 1),
                    "sum_us": {k: round(sum(us[k]), 1) for k in whole},
                    "sum_over_unpieced": {k: round(sum(us[k]) / row["unpieced_us"][k], 3) for k in whole}}
            out[f"{name}_p{p}"] = row
            del send, recv
        del x, y
    text = json.dumps(out)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
