#!/usr/bin/env python3
"""Measurement: the MXFP6 codec's kernels beside the MXFP8 and the MXFP4 codec's (MXFP6.md).

Two buckets, both cut into 8 chunks as the op at 8 ranks cuts them: 2^26 f32 elements
(256 MiB) and 2^27 bf16 elements.  Every call's kernels are timed alone through the
library's kernel-timing hook (bagua_time_next_kernels: device events at the kernel's own
start and end, no dispatch gaps) and summed per call; 3 warm-up steps, then the median
of 20 with the minimum and the maximum, all variants of all three codecs interleaved step
by step in one run, their order rotated from step to step:

  <codec>_encode / _decode          compress and decompress of the whole bucket
  <codec>_middle_p2 / _p8 / _p16    the fused middle step on the own chunk of the same bucket cut
                                    into 2 / 8 / 16 chunks (tensor NULL, as the op calls it): the
                                    summation tree's BY = 2, 4 and 8 builds

The yardstick is the MXFP8 kernel of the same run: `ratio_mxfp8` beside `by_bytes`, the ratio of
the algorithmic bytes, an expectation, not a threshold.  Each kernel's fraction of the 8 TB/s HBM
roofline is its algorithmic bytes over time over 8e12.  Writes the record to --out and, for a
file under profiles/, its index line in profiles/README.md (--index FILE: only that, for a
record copied into profiles/).

    python tools/mxfp6_probe.py [--out profiles/r17_mxfp6.json]
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

HBM_BYTES_PER_S = 8e12
CODECS = ("mxfp6", "mxfp8", "mxfp4")
STEPS = ("encode", "decode", "middle_p2", "middle_p8", "middle_p16")
INDEX = ("| `{name}` | MXFP6 codec beside MXFP8 and MXFP4 in the same run, per kernel, 8 chunks, time over the MXFP8 "
         "kernel's (by bytes): 256 MiB f32 encode {fe:.1f} µs {fer:.2f} (0.95), decode {fd:.1f} µs {fdr:.2f} (0.95), "
         "fused middle step at p = 2 / 8 / 16 {fm2:.1f} / {fm8:.1f} / {fm16:.1f} µs "
         "{fm2r:.2f} / {fm8r:.2f} / {fm16r:.2f} (0.76); 2^27 bf16 encode {be:.1f} µs {ber:.2f} (0.92), decode {bd:.1f} "
         "µs {bdr:.2f} (0.92), middle {bm2:.1f} / {bm8:.1f} / {bm16:.1f} µs {bm2r:.2f} / "
         "{bm8r:.2f} / {bm16r:.2f} | `tools/mxfp6_probe.py` |\n")


def hip_runtime_version() -> int:
    v = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipRuntimeGetVersion(ctypes.byref(v))
    return v.value


def measure(N, dtype_code, tdtype, esz, n, warmup, reps):
    K = N.K
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(7)
    g = (torch.randn(n, device=dev, generator=gen) * 1e-3).to(tdtype)
    dec = torch.empty(n, dtype=tdtype, device=dev)
    variants = {}

    for p in (8, 2, 16):
        cs = n // p
        for codec in CODECS:
            size, comp, decomp, mid = (getattr(K, f"bagua_{codec}_{f}") for f in
                                       ("compressed_bytes", "compress", "decompress", "reduce_requantize"))
            S = size(cs, p)
            buf, recv, out = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(3))
            N.check(comp(dtype_code, g.data_ptr(), n, cs, p, recv.data_ptr(), S, -1, sp), f"{codec} recv")

            def enc(comp=comp, cs=cs, p=p, buf=buf, S=S, codec=codec):
                N.check(comp(dtype_code, g.data_ptr(), n, cs, p, buf.data_ptr(), S, -1, sp), f"{codec} encode")

            def dcd(decomp=decomp, cs=cs, p=p, recv=recv, S=S, codec=codec):
                N.check(decomp(dtype_code, recv.data_ptr(), S, cs, p, dec.data_ptr(), sp), f"{codec} decode")

            def mdl(mid=mid, cs=cs, p=p, recv=recv, out=out, S=S, codec=codec):
                N.check(mid(dtype_code, recv.data_ptr(), S, cs, p, None, 1, out.data_ptr(), S, p // 2, sp), f"{codec} middle")

            if p == 8:
                variants[f"{codec}_encode"] = (enc, n * esz + S)
                variants[f"{codec}_decode"] = (dcd, S + n * esz)
            variants[f"{codec}_middle_p{p}"] = (mdl, (p + 1) * (S // p))
    times = {k: [] for k in variants}
    kernel_names = {}
    order = list(variants)
    assert len(order) % 7, len(order)
    for step in range(warmup + reps):
        k = (step * 7) % len(order)  # the starting point rotates by a stride coprime to the count
        for name in order[k:] + order[:k]:
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(8)]
            for a, b in evs:
                a.record(st)
                b.record(st)
            N.time_next_kernels(evs)
            variants[name][0]()
            torch.cuda.synchronize()
            names = N.timed_kernel_names()
            N.time_next_kernels([])
            assert 0 < len(names) < 8, (name, names)
            kernel_names[name] = names
            if step >= warmup:
                times[name].append(sum(a.elapsed_time(b) for (a, b), _ in zip(evs, names)) * 1e3)
    rec = {"elements": n, "chunks": 8, "bytes_per_element": esz}
    for name, (_, nbytes) in variants.items():
        med = statistics.median(times[name])
        rec[name] = {"us": round(med, 2), "min_us": round(min(times[name]), 2), "max_us": round(max(times[name]), 2),
                     "bytes": int(nbytes), "hbm_roofline_fraction": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                     "kernels": kernel_names[name]}
    for s in STEPS:
        for other in ("mxfp8", "mxfp4"):
            rec[f"ratio_{other}_{s}"] = {"time": round(rec[f"mxfp6_{s}"]["us"] / rec[f"{other}_{s}"]["us"], 3),
                                         "by_bytes": round(rec[f"mxfp6_{s}"]["bytes"] / rec[f"{other}_{s}"]["bytes"], 3)}
    return rec


def write_index(rec, out):
    """the record's index row in profiles/README.md, below the last row of the probes' table (files
    named rNN_...), when `out` lies under profiles/ and has no row yet"""
    prof = os.path.join(ROOT, "profiles")
    if os.path.dirname(os.path.abspath(out)) != prof:
        return
    readme, name = os.path.join(prof, "README.md"), os.path.basename(out)
    lines = open(readme).read().splitlines(keepends=True)
    if any(f"`{name}`" in ln for ln in lines):
        return
    at = max((i for i, ln in enumerate(lines) if ln.startswith("| `r") and ln[4:6].isdigit()), default=len(lines) - 1) + 1
    vals = {"name": name}
    for t, r in (("f", rec["f32"]), ("b", rec["bf16"])):
        for key, s in (("e", "encode"), ("d", "decode"), ("m2", "middle_p2"), ("m8", "middle_p8"), ("m16", "middle_p16")):
            vals[t + key] = r[f"mxfp6_{s}"]["us"]
            vals[t + key + "r"] = r[f"ratio_mxfp8_{s}"]["time"]
    with open(readme, "w") as fh:
        fh.writelines(lines[:at] + [INDEX.format(**vals)] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_mxfp6.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    args = ap.parse_args()
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    rec = {"probe": "mxfp6", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels), summed per call, median with minimum and maximum; variants "
                     "interleaved per step, their order rotated from step to step",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
           "torch_hip": torch.version.hip,
           "f32": measure(N, N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32, args.warmup, args.reps),
           "bf16": measure(N, N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16, args.warmup, args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    write_index(rec, args.out)


if __name__ == "__main__":
    main()
