#!/usr/bin/env python3
"""Measurement: the MXFP8 codec's kernels beside the MinMax-UInt8 and the MXFP4 codec's (MXFP8.md).

Two buckets, both cut into 8 chunks as the op at 8 ranks cuts them: 2^26 f32 elements
(256 MiB) and 2^27 bf16 elements.  Every call's kernels are timed alone through the
library's kernel-timing hook (bagua_time_next_kernels: device events at the kernel's own
start and end, no dispatch gaps) and summed per call; 3 warm-up steps, then the median
of 20, all variants of all three codecs interleaved step by step in one run:

  <codec>_encode / _decode          compress and decompress of the whole bucket
  <codec>_middle_p2 / _p8 / _p16    the fused middle step on the own chunk of the same bucket cut
                                    into 2 / 8 / 16 chunks (tensor NULL, as the op calls it): the
                                    summation tree's BY = 2, 4 and 8 builds
  mxfp8_..._sw / _hw                the MXFP8 kernels with BAGUA_MXFP8_HWCVT=0 / 1 (the arithmetic
                                    or gfx950's FP8 conversions; same bytes)

By bytes MXFP8's fp32 encode + decode should take 0.72 of MinMax's time (10.06 N against
14 N) and bf16 0.76: `ratio_minmax`, an expectation, not a threshold.  Each kernel's fraction
of the 8 TB/s HBM roofline is its algorithmic bytes over time over 8e12.  Writes the record
to --out and, for a file under profiles/, its index line in profiles/README.md (--index FILE:
only that, for a record copied into profiles/).

    python tools/mxfp8_probe.py [--out profiles/r13_mxfp8.json]
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
INDEX = ("| `{name}` | MXFP8 codec beside MinMax-UInt8 and MXFP4 in the same run, per kernel, 8 chunks: 256 MiB f32 "
         "encode {fe:.1f} + decode {fd:.1f} µs against MinMax {fme:.1f} + {fmd:.1f} µs (ratio {fr:.2f}; 0.72 by bytes) "
         "and MXFP4 {f4e:.1f} + {f4d:.1f} µs, fused middle step at p = 8 {fm:.1f} µs (MinMax {fmm:.1f}, MXFP4 "
         "{f4m:.1f}); 2^27 bf16 encode {be:.1f} + decode {bd:.1f} µs against {bme:.1f} + {bmd:.1f} µs (ratio "
         "{br:.2f}; 0.76 by bytes), middle {bm:.1f} µs; hardware against arithmetic conversions per kernel | "
         "`tools/mxfp8_probe.py` |\n")


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

    def u8(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def mode(hw):
        if hw is None:
            os.environ.pop("BAGUA_MXFP8_HWCVT", None)
        else:
            os.environ["BAGUA_MXFP8_HWCVT"] = hw

    variants = {}
    for p in (8, 2, 16):
        cs = n // p
        S8, S4 = K.bagua_mxfp8_compressed_bytes(cs, p), K.bagua_mxfp4_compressed_bytes(cs, p)
        Sm = K.bagua_minmax_u8_compressed_bytes(dtype_code, cs, p)
        wsb = K.bagua_minmax_u8_workspace_bytes(cs, p)
        b8, r8, o8 = u8(S8), u8(S8), u8(S8)
        b4, r4, o4 = u8(S4), u8(S4), u8(S4)
        bm, rm, om, ws = u8(Sm), u8(Sm), u8(Sm), u8(wsb)
        N.check(K.bagua_mxfp8_compress(dtype_code, g.data_ptr(), n, cs, p, r8.data_ptr(), S8, -1, sp), "recv 8")
        N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, r4.data_ptr(), S4, -1, sp), "recv 4")
        N.check(K.bagua_minmax_u8_compress(dtype_code, g.data_ptr(), n, cs, p, rm.data_ptr(), Sm, ws.data_ptr(), wsb, -1,
                                           sp), "recv minmax")

        def enc8(hw, cs=cs, p=p, b8=b8, S8=S8):
            mode(hw)
            N.check(K.bagua_mxfp8_compress(dtype_code, g.data_ptr(), n, cs, p, b8.data_ptr(), S8, -1, sp), "mxfp8 encode")

        def dec8(hw, cs=cs, p=p, r8=r8, S8=S8):
            mode(hw)
            N.check(K.bagua_mxfp8_decompress(dtype_code, r8.data_ptr(), S8, cs, p, dec.data_ptr(), sp), "mxfp8 decode")

        def mid8(hw, cs=cs, p=p, r8=r8, o8=o8, S8=S8):
            mode(hw)
            N.check(K.bagua_mxfp8_reduce_requantize(dtype_code, r8.data_ptr(), S8, cs, p, None, 1, o8.data_ptr(), S8,
                                                    p // 2, sp), "mxfp8 middle")

        def enc4(cs=cs, p=p, b4=b4, S4=S4):
            N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, b4.data_ptr(), S4, -1, sp), "mxfp4 encode")

        def dec4(cs=cs, p=p, r4=r4, S4=S4):
            N.check(K.bagua_mxfp4_decompress(dtype_code, r4.data_ptr(), S4, cs, p, dec.data_ptr(), sp), "mxfp4 decode")

        def mid4(cs=cs, p=p, r4=r4, o4=o4, S4=S4):
            N.check(K.bagua_mxfp4_reduce_requantize(dtype_code, r4.data_ptr(), S4, cs, p, None, 1, o4.data_ptr(), S4,
                                                    p // 2, sp), "mxfp4 middle")

        def encm(cs=cs, p=p, bm=bm, Sm=Sm, ws=ws, wsb=wsb):
            N.check(K.bagua_minmax_u8_compress(dtype_code, g.data_ptr(), n, cs, p, bm.data_ptr(), Sm, ws.data_ptr(), wsb,
                                               -1, sp), "minmax encode")

        def decm(cs=cs, p=p, rm=rm, Sm=Sm):
            N.check(K.bagua_minmax_u8_decompress(dtype_code, rm.data_ptr(), Sm, cs, p, dec.data_ptr(), sp), "minmax decode")

        def midm(cs=cs, p=p, rm=rm, om=om, Sm=Sm, ws=ws, wsb=wsb):
            N.check(K.bagua_minmax_u8_reduce_requantize(dtype_code, rm.data_ptr(), Sm, cs, p, None, 1, om.data_ptr(), Sm,
                                                        p // 2, ws.data_ptr(), wsb, sp), "minmax middle")

        if p == 8:
            variants["minmax_encode"] = (encm, n * esz + Sm)
            variants["minmax_decode"] = (decm, Sm + n * esz)
            variants["mxfp4_encode"] = (enc4, n * esz + S4)
            variants["mxfp4_decode"] = (dec4, S4 + n * esz)
        variants[f"minmax_middle_p{p}"] = (midm, (p + 1) * (Sm // p))
        variants[f"mxfp4_middle_p{p}"] = (mid4, (p + 1) * (S4 // p))
        for suffix, hw in (("", None), ("_sw", "0"), ("_hw", "1")):
            if p == 8:
                variants["mxfp8_encode" + suffix] = (lambda hw=hw, f=enc8: f(hw), n * esz + S8)
                variants["mxfp8_decode" + suffix] = (lambda hw=hw, f=dec8: f(hw), S8 + n * esz)
            variants[f"mxfp8_middle_p{p}" + suffix] = (lambda hw=hw, f=mid8: f(hw), (p + 1) * (S8 // p))
    times = {k: [] for k in variants}
    kernel_names = {}
    order = list(variants)
    assert len(order) % 7, len(order)
    for step in range(warmup + reps):
        # the starting point rotates by a stride coprime to the count; the rotation is cyclic, so a
        # variant keeps its predecessor except at the wrap (MXFP8.md, "Measured", on what that leaves)
        k = (step * 7) % len(order)
        for name in order[k:] + order[:k]:
            fn = variants[name][0]
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(8)]
            for a, b in evs:
                a.record(st)
                b.record(st)
            N.time_next_kernels(evs)
            fn()
            torch.cuda.synchronize()
            names = N.timed_kernel_names()
            N.time_next_kernels([])
            assert 0 < len(names) < 8, (name, names)
            kernel_names[name] = names
            if step >= warmup:
                times[name].append(sum(a.elapsed_time(b) for (a, b), _ in zip(evs, names)) * 1e3)
    mode(None)
    rec = {"elements": n, "chunks": 8, "bytes_per_element": esz}
    for name, (_, nbytes) in variants.items():
        med = statistics.median(times[name])
        rec[name] = {"us": round(med, 2), "min_us": round(min(times[name]), 2), "max_us": round(max(times[name]), 2),
                     "bytes": int(nbytes), "hbm_roofline_fraction": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                     "kernels": kernel_names[name]}
    both = lambda c, s="": rec[c + "_encode" + s]["us"] + rec[c + "_decode" + s]["us"]  # noqa: E731
    for suffix in ("", "_sw", "_hw"):
        rec["ratio_minmax" + suffix] = round(both("mxfp8", suffix) / both("minmax"), 3)
    rec["ratio_mxfp4"] = round(both("mxfp8") / both("mxfp4"), 3)
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
    f, b = rec["f32"], rec["bf16"]
    at = max((i for i, ln in enumerate(lines) if ln.startswith("| `r") and ln[4:6].isdigit()), default=len(lines) - 1) + 1
    row = INDEX.format(name=name, fe=f["mxfp8_encode"]["us"], fd=f["mxfp8_decode"]["us"], fme=f["minmax_encode"]["us"],
                       fmd=f["minmax_decode"]["us"], fr=f["ratio_minmax"], f4e=f["mxfp4_encode"]["us"],
                       f4d=f["mxfp4_decode"]["us"], fm=f["mxfp8_middle_p8"]["us"], fmm=f["minmax_middle_p8"]["us"],
                       f4m=f["mxfp4_middle_p8"]["us"], be=b["mxfp8_encode"]["us"], bd=b["mxfp8_decode"]["us"],
                       bme=b["minmax_encode"]["us"], bmd=b["minmax_decode"]["us"], br=b["ratio_minmax"],
                       bm=b["mxfp8_middle_p8"]["us"])
    with open(readme, "w") as fh:
        fh.writelines(lines[:at] + [row] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_mxfp8.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    args = ap.parse_args()
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    rec = {"probe": "mxfp8", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels), summed per call, median; variants interleaved per step, "
                     "their order rotated from step to step",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
           "torch_hip": torch.version.hip, "expected_ratio_minmax_by_bytes": {"f32": 0.72, "bf16": 0.76},
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
