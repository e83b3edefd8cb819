#!/usr/bin/env python3
"""Measurement: the MXFP8 codec's stochastic rounding (MXFP8.md, "Stochastic rounding").

The plain, error-feedback and stochastic encodes, the latter under both conversions
(BAGUA_MXFP8_HWCVT=1: one v_cvt_scalef32_sr_fp8_f32 per element; =0: mx8_quant_sr), and the
four middle steps at p = 8, per kernel through bagua_time_next_kernels, interleaved step by
step in one run with the order rotated from step to step, 3 warm-up steps and the median of 20
(minimum and maximum kept): 2^26 f32 elements (256 MiB) and 2^27 bf16, cut into 8 chunks.  The
stochastic encode moves the plain encode's bytes, so the plain mxfp8_encode_kernel of the same
run is its yardstick: everything above it is hash and rounding VALU.

    python tools/mxfp8_sr_probe.py [--out profiles/r16_mxfp8_sr.json]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bagua-core_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SWITCH = "BAGUA_MXFP8_HWCVT"
INDEX = ("| `{name}` | MXFP8 stochastic rounding beside the plain and error-feedback kernels in the same run, per "
         "kernel, 8 chunks, hardware / arithmetic rounding: 256 MiB f32 encode {fh:.1f} / {fa:.1f} µs against plain "
         "{fp:.1f} and EF {fe:.1f} µs, middle step at p = 8 {fmh:.1f} / {fma:.1f} against {fmp:.1f} and {fme:.1f} µs; "
         "2^27 bf16 {bh:.1f} / {ba:.1f} µs against {bp:.1f} and {be:.1f} µs, middle {bmh:.1f} / {bma:.1f} against "
         "{bmp:.1f} and {bme:.1f} µs | `tools/mxfp8_sr_probe.py` |\n")


def hip_runtime_version() -> int:
    v = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipRuntimeGetVersion(ctypes.byref(v))
    return v.value


def measure(N, torch, dtype_code, tdtype, esz, n, p, warmup, reps):
    K = N.K
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    cs = n // p
    gen = torch.Generator(device=dev).manual_seed(7)
    g = (torch.randn(n, device=dev, generator=gen) * 1e-3).to(tdtype)
    worker = torch.zeros(n, dtype=torch.float32, device=dev)
    server = torch.zeros(cs, dtype=torch.float32, device=dev)
    S = K.bagua_mxfp8_compressed_bytes(cs, p)
    seg = S // p
    mx, mx_recv, mx_out = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(3))
    N.check(K.bagua_mxfp8_compress(dtype_code, g.data_ptr(), n, cs, p, mx_recv.data_ptr(), S, -1, sp), "recv")
    key = K.bagua_mxfp4_sr_key(1, 0, 0, 0)
    args = (dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1)
    mid = (dtype_code, mx_recv.data_ptr(), S, cs, p)
    tail = (mx_out.data_ptr(), S, p // 2)
    # name -> (the switch's value or None for the default, call, kernel, bytes moved)
    variants = {
        "encode": (None, lambda: K.bagua_mxfp8_compress(*args, sp), "mxfp8_encode_kernel", n * esz + S),
        "encode_ef": (None, lambda: K.bagua_mxfp8_compress_ef(*args, worker.data_ptr(), sp), "mxfp8_encode_ef_kernel",
                      n * esz + 8 * n + S),
        "encode_sr_hw": ("1", lambda: K.bagua_mxfp8_compress_sr(*args, key, sp), "mxfp8_encode_kernel", n * esz + S),
        "encode_sr_arith": ("0", lambda: K.bagua_mxfp8_compress_sr(*args, key, sp), "mxfp8_encode_kernel", n * esz + S),
        "middle_p8": (None, lambda: K.bagua_mxfp8_reduce_requantize(*mid, None, 1, *tail, sp),
                      "mxfp8_reduce_encode_kernel", (p + 1) * seg),
        "middle_ef_p8": (None, lambda: K.bagua_mxfp8_reduce_requantize_ef(*mid, 1, *tail, server.data_ptr(), sp),
                         "mxfp8_reduce_encode_ef_kernel", (p + 1) * seg + 8 * cs),
        "middle_sr_hw_p8": ("1", lambda: K.bagua_mxfp8_reduce_requantize_sr(*mid, 1, *tail, key, sp),
                            "mxfp8_reduce_encode_kernel", (p + 1) * seg),
        "middle_sr_arith_p8": ("0", lambda: K.bagua_mxfp8_reduce_requantize_sr(*mid, 1, *tail, key, sp),
                               "mxfp8_reduce_encode_kernel", (p + 1) * seg),
    }
    order = list(variants)
    times = {k: [] for k in variants}
    for step in range(warmup + reps):
        for name in order[step % len(order):] + order[:step % len(order)]:  # rotated from step to step
            switch, fn, kernel, _ = variants[name]
            if switch is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = switch  # read at every launch
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2)]
            for a, b in evs:
                a.record(st)
                b.record(st)
            N.time_next_kernels(evs)
            N.check(fn(), name)
            torch.cuda.synchronize()
            names = N.timed_kernel_names()
            N.time_next_kernels([])
            assert names == [kernel], (name, names)
            if step >= warmup:
                times[name].append(evs[0][0].elapsed_time(evs[0][1]) * 1e3)
    os.environ.pop(SWITCH, None)
    rec = {"elements": n, "chunks": p, "bytes_per_element": esz}
    for name, (switch, _, kernel, nbytes) in variants.items():
        med = statistics.median(times[name])
        rec[name] = {"us": round(med, 2), "min_us": round(min(times[name]), 2), "max_us": round(max(times[name]), 2),
                     "bytes": int(nbytes), "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "kernel": kernel,
                     "hwcvt": switch or "default"}
    for arm in ("hw", "arith"):
        rec[f"encode_sr_{arm}_over_plain"] = round(rec[f"encode_sr_{arm}"]["us"] / rec["encode"]["us"], 3)
        rec[f"encode_sr_{arm}_over_ef"] = round(rec[f"encode_sr_{arm}"]["us"] / rec["encode_ef"]["us"], 3)
        rec[f"middle_sr_{arm}_over_plain"] = round(rec[f"middle_sr_{arm}_p8"]["us"] / rec["middle_p8"]["us"], 3)
        rec[f"middle_sr_{arm}_over_ef"] = round(rec[f"middle_sr_{arm}_p8"]["us"] / rec["middle_ef_p8"]["us"], 3)
    rec["encode_sr_hw_over_arith"] = round(rec["encode_sr_hw"]["us"] / rec["encode_sr_arith"]["us"], 3)
    rec["middle_sr_hw_over_arith"] = round(rec["middle_sr_hw_p8"]["us"] / rec["middle_sr_arith_p8"]["us"], 3)
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
    at = max((i for i, ln in enumerate(lines) if re.match(r"\| `r\d\d_", ln)), default=len(lines) - 1) + 1
    row = INDEX.format(name=name, fh=f["encode_sr_hw"]["us"], fa=f["encode_sr_arith"]["us"], fp=f["encode"]["us"],
                       fe=f["encode_ef"]["us"], fmh=f["middle_sr_hw_p8"]["us"], fma=f["middle_sr_arith_p8"]["us"],
                       fmp=f["middle_p8"]["us"], fme=f["middle_ef_p8"]["us"], bh=b["encode_sr_hw"]["us"],
                       ba=b["encode_sr_arith"]["us"], bp=b["encode"]["us"], be=b["encode_ef"]["us"],
                       bmh=b["middle_sr_hw_p8"]["us"], bma=b["middle_sr_arith_p8"]["us"], bmp=b["middle_p8"]["us"],
                       bme=b["middle_ef_p8"]["us"])
    with open(readme, "w") as fh:
        fh.writelines(lines[:at] + [row] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_mxfp8_sr.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    args = ap.parse_args()
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    import torch
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    rec = {"probe": "mxfp8_sr", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels), median; variants interleaved per step, order rotated",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
           "torch_hip": torch.version.hip,
           "f32": measure(N, torch, N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32, 8, args.warmup, args.reps),
           "bf16": measure(N, torch, N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16, 8, args.warmup, args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    write_index(rec, args.out)


if __name__ == "__main__":
    main()
