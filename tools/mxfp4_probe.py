#!/usr/bin/env python3
"""Measurement: the MXFP4 codec's kernels beside the MinMax-UInt8 codec's (MXFP4.md).

Two buckets, both cut into 8 chunks as the op at 8 ranks cuts them: 2^26 f32 elements
(256 MiB) and 2^27 bf16 elements.  Every call's kernels are timed alone through the
library's kernel-timing hook (bagua_time_next_kernels: device events at the kernel's own
start and end, no dispatch gaps) and summed per call; 3 warm-up steps, then the median
of 20, all variants interleaved step by step in one run:

  mxfp4 encode / decode / middle    bagua_mxfp4_compress, _decompress and the fused middle
                                    step at p = 8 (tensor NULL, as the op calls it)
  ... _sw / _hw                     the same with BAGUA_MXFP4_HWCVT=0 / 1 (the arithmetic
                                    or gfx950's FP4 conversions; same bytes)
  minmax encode / decode            bagua_minmax_u8_compress / _decompress, the yardstick

MXFP4 moves 9.06 N bytes per fp32 encode + decode against MinMax's 14 N, so its
encode + decode must not take longer than MinMax's: `ratio` <= 1.0.  Each kernel's
fraction of the 8 TB/s HBM roofline is its algorithmic bytes over time over 8e12.
Writes the record to --out and, for a file under profiles/, its index line in
profiles/README.md (--index FILE: only that, for a record copied into profiles/).

    python tools/mxfp4_probe.py [--out profiles/r08_mxfp4.json]
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
INDEX = ("| `{name}` | MXFP4 codec beside MinMax-UInt8 in the same run, per kernel, 8 chunks: 256 MiB f32 encode "
         "{fe:.1f} + decode {fd:.1f} µs against MinMax {fme:.1f} + {fmd:.1f} µs (ratio {fr:.2f}; bar 1.0), fused "
         "middle step at p = 8 {fm:.1f} µs; 2^27 bf16 encode {be:.1f} + decode {bd:.1f} µs against {bme:.1f} + "
         "{bmd:.1f} µs (ratio {br:.2f}), middle {bm:.1f} µs | `tools/mxfp4_probe.py` |\n")


def hip_runtime_version() -> int:
    v = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipRuntimeGetVersion(ctypes.byref(v))
    return v.value


def measure(N, dtype_code, tdtype, esz, n, p, warmup, reps):
    K = N.K
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    cs = n // p
    gen = torch.Generator(device=dev).manual_seed(7)
    g = (torch.randn(n, device=dev, generator=gen) * 1e-3).to(tdtype)
    dec = torch.empty(n, dtype=tdtype, device=dev)
    S = K.bagua_mxfp4_compressed_bytes(cs, p)
    mx, mx_recv, mx_out = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(3))
    Sm = K.bagua_minmax_u8_compressed_bytes(dtype_code, cs, p)
    wsb = K.bagua_minmax_u8_workspace_bytes(cs, p)
    mm = torch.empty(Sm, dtype=torch.uint8, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, mx_recv.data_ptr(), S, -1, sp), "recv")

    def mode(hw):
        if hw is None:
            os.environ.pop("BAGUA_MXFP4_HWCVT", None)
        else:
            os.environ["BAGUA_MXFP4_HWCVT"] = hw

    def mx_enc(hw):
        mode(hw)
        N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, sp), "mxfp4 encode")

    def mx_dec(hw):
        mode(hw)
        N.check(K.bagua_mxfp4_decompress(dtype_code, mx.data_ptr(), S, cs, p, dec.data_ptr(), sp), "mxfp4 decode")

    def mx_mid(hw):
        mode(hw)
        N.check(K.bagua_mxfp4_reduce_requantize(dtype_code, mx_recv.data_ptr(), S, cs, p, None, 1, mx_out.data_ptr(), S,
                                                p // 2, sp), "mxfp4 middle")

    def mm_enc():
        N.check(K.bagua_minmax_u8_compress(dtype_code, g.data_ptr(), n, cs, p, mm.data_ptr(), Sm, ws.data_ptr(), wsb, -1,
                                           sp), "minmax encode")

    def mm_dec():
        N.check(K.bagua_minmax_u8_decompress(dtype_code, mm.data_ptr(), Sm, cs, p, dec.data_ptr(), sp), "minmax decode")

    seg = S // p
    variants = {"minmax_encode": (mm_enc, n * esz + Sm), "minmax_decode": (mm_dec, Sm + n * esz)}
    for suffix, hw in (("", None), ("_sw", "0"), ("_hw", "1")):
        variants["mxfp4_encode" + suffix] = (lambda hw=hw: mx_enc(hw), n * esz + S)
        variants["mxfp4_decode" + suffix] = (lambda hw=hw: mx_dec(hw), S + n * esz)
        variants["mxfp4_middle_p8" + suffix] = (lambda hw=hw: mx_mid(hw), p * seg + seg)
    times = {k: [] for k in variants}
    kernel_names = {}
    for step in range(warmup + reps):
        for name, (fn, _) in variants.items():
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
    rec = {"elements": n, "chunks": p, "bytes_per_element": esz}
    for name, (_, nbytes) in variants.items():
        med = statistics.median(times[name])
        rec[name] = {"us": round(med, 2), "min_us": round(min(times[name]), 2), "max_us": round(max(times[name]), 2),
                     "bytes": int(nbytes), "hbm_roofline_fraction": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3),
                     "kernels": kernel_names[name]}
    for suffix in ("", "_sw", "_hw"):
        rec["ratio" + suffix] = round((rec["mxfp4_encode" + suffix]["us"] + rec["mxfp4_decode" + suffix]["us"]) /
                                      (rec["minmax_encode"]["us"] + rec["minmax_decode"]["us"]), 3)
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
    f32, b16 = rec["f32"], rec["bf16"]
    at = max((i for i, ln in enumerate(lines) if ln.startswith("| `r0")), default=len(lines) - 1) + 1
    row = INDEX.format(name=name, fe=f32["mxfp4_encode"]["us"], fd=f32["mxfp4_decode"]["us"],
                       fme=f32["minmax_encode"]["us"], fmd=f32["minmax_decode"]["us"], fr=f32["ratio"],
                       fm=f32["mxfp4_middle_p8"]["us"], be=b16["mxfp4_encode"]["us"], bd=b16["mxfp4_decode"]["us"],
                       bme=b16["minmax_encode"]["us"], bmd=b16["minmax_decode"]["us"], br=b16["ratio"],
                       bm=b16["mxfp4_middle_p8"]["us"])
    with open(readme, "w") as f:
        f.writelines(lines[:at] + [row] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_mxfp4.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    args = ap.parse_args()
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    rec = {"probe": "mxfp4", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels), summed per call, median; variants interleaved per step",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
           "torch_hip": torch.version.hip, "ratio_bar": 1.0,
           "f32": measure(N, N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32, 8, args.warmup, args.reps),
           "bf16": measure(N, N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16, 8, args.warmup, args.reps)}
    rec["meets_bar"] = bool(rec["f32"]["ratio"] <= 1.0 and rec["bf16"]["ratio"] <= 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    write_index(rec, args.out)


if __name__ == "__main__":
    main()
