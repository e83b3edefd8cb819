#!/usr/bin/env python3
"""Measurement: what error feedback costs the 1-bit encode.

At 2^26 f32 elements in one chunk, timed with device events around each call
(3 warm-up steps, then the median of 20, the variants interleaved step by step):

  plain    bagua_onebit_compress                     4.125 N bytes (the yardstick,
           measured in the same run; this change does not touch its kernel)
  ef       bagua_onebit_compress_ef                  12.125 N bytes: gradient read,
           carry read, carry written in place, bits
           (carry accesses default-policy and non-temporal, BAGUA_OB_EF_CARRY_NT)
  unfused  the same step from existing pieces, for contrast: torch add (g + r),
           plain encode of the sum, decode, torch sub (the materialised residual)

The two kernels of the plain and of the fused call (encode, finalize) are also
timed alone through the library's kernel-timing hook.  Writes the record (with the
HIP runtime version) to --out and, for a file under profiles/, its index line in
profiles/README.md.

    python tools/onebit_ef_probe.py [--log2n 26] [--out profiles/r07_onebit_ef.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bagua-core_amd"))

INDEX = ("| `{name}` | 1-bit encode with error feedback vs the plain encode in the same run, 2^{log2n} f32, one chunk: "
         "plain {plain:.1f} µs, fused {ef:.1f} µs ({ratio:.2f} of the plain encode's bytes/s; target 0.85), "
         "unfused add + encode + decode + sub {unfused:.1f} µs | `tools/onebit_ef_probe.py` |\n")


def hip_runtime_version() -> int:
    v = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipRuntimeGetVersion(ctypes.byref(v))
    return v.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_onebit_ef.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    K = N.K
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    S = K.bagua_onebit_compressed_bytes(n, 1)
    wsb = K.bagua_onebit_workspace_bytes(n, 1)
    out = torch.empty(S, dtype=torch.uint8, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    carry = {k: torch.zeros(n, device=dev) for k in ("ef", "ef_nt")}
    scale = {k: torch.zeros(4, device=dev) for k in ("ef", "ef_nt")}
    resid, v, dec = (torch.zeros(n, device=dev) for _ in range(3))

    def plain():
        N.check(K.bagua_onebit_compress(0, g.data_ptr(), n, n, 1, out.data_ptr(), S, ws.data_ptr(), wsb, -1, sp), "plain")

    def fused(key, nt):
        os.environ["BAGUA_OB_EF_CARRY_NT"] = nt
        N.check(K.bagua_onebit_compress_ef(0, g.data_ptr(), n, n, 1, out.data_ptr(), S, ws.data_ptr(), wsb, -1,
                                           carry[key].data_ptr(), scale[key].data_ptr(), sp), key)

    def unfused():
        torch.add(g, resid, out=v)
        N.check(K.bagua_onebit_compress(0, v.data_ptr(), n, n, 1, out.data_ptr(), S, ws.data_ptr(), wsb, -1, sp), "enc")
        N.check(K.bagua_onebit_decompress(0, out.data_ptr(), S, n, 1, dec.data_ptr(), sp), "dec")
        torch.sub(v, dec, out=resid)

    variants = {"plain": plain, "ef": lambda: fused("ef", "0"), "ef_nt": lambda: fused("ef_nt", "1"),
                "unfused": unfused}
    times = {k: [] for k in variants}
    for step in range(args.warmup + args.reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            b.synchronize()
            if step >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    # the kernels alone (encode, finalize), without dispatch gaps
    kernels = {}
    for name in ("plain", "ef", "ef_nt"):
        per = {}
        for step in range(args.warmup + args.reps):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2)]
            for a, b in evs:
                a.record(st)
                b.record(st)
            N.time_next_kernels(evs)
            variants[name]()
            torch.cuda.synchronize()
            names = N.timed_kernel_names()
            N.time_next_kernels([])
            if step >= args.warmup:
                for kname, (a, b) in zip(names, evs):
                    per.setdefault(kname, []).append(a.elapsed_time(b) * 1e3)
        kernels[name] = {k: round(statistics.median(u), 2) for k, u in per.items()}
    os.environ.pop("BAGUA_OB_EF_CARRY_NT", None)
    med = {k: statistics.median(u) for k, u in times.items()}
    bytes_moved = {"plain": 4.125 * n, "ef": 12.125 * n, "ef_nt": 12.125 * n, "unfused": (12 + 4.125 + 4.125 + 12) * n}
    rec = {"probe": "onebit_ef", "elements": n, "dtype": "f32", "chunks": 1, "warmup": args.warmup, "reps": args.reps,
           "timing": "device events around each call, median; variants interleaved per step",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
           "torch_hip": torch.version.hip, "kernel_us": kernels}
    for k in variants:
        rec[k] = {"us": round(med[k], 2), "min_us": round(min(times[k]), 2), "max_us": round(max(times[k]), 2),
                  "bytes": int(bytes_moved[k]), "gbps": round(bytes_moved[k] / (med[k] * 1e-6) / 1e9, 1)}
    best = "ef" if med["ef"] <= med["ef_nt"] else "ef_nt"
    rec["ef_best"] = best
    rec["ef_bandwidth_over_plain"] = round(rec[best]["gbps"] / rec["plain"]["gbps"], 3)
    rec["ef_default_bandwidth_over_plain"] = round(rec["ef"]["gbps"] / rec["plain"]["gbps"], 3)
    rec["target_bandwidth_over_plain"] = 0.85

    def encode_us(name):  # the encode kernel of a variant's two
        return next((u for k, u in kernels[name].items() if "encode" in k), None)
    if encode_us("plain") and encode_us("ef") and encode_us("ef_nt"):
        rec["ef_kernel_bandwidth_over_plain"] = {
            k: round((12.125 / encode_us(k)) / (4.125 / encode_us("plain")), 3) for k in ("ef", "ef_nt")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    prof = os.path.join(ROOT, "profiles")
    if os.path.dirname(os.path.abspath(args.out)) == prof:
        readme, name = os.path.join(prof, "README.md"), os.path.basename(args.out)
        text = open(readme).read()
        if f"`{name}`" not in text:
            with open(readme, "a") as f:
                f.write(INDEX.format(name=name, log2n=args.log2n, plain=med["plain"], ef=med["ef"],
                                     ratio=rec["ef_default_bandwidth_over_plain"], unfused=med["unfused"]))


if __name__ == "__main__":
    main()
