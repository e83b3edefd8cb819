#!/usr/bin/env python3
"""Measurement: the MXFP4 codec's error-feedback kernels beside the plain ones (MXFP4.md).

Two buckets, both cut into 8 chunks as the op at 8 ranks cuts them: 2^26 f32 elements
(256 MiB) and 2^27 bf16 elements.  Every call's kernels are timed alone through the
library's kernel-timing hook (bagua_time_next_kernels: device events at the kernel's own
start and end, no dispatch gaps); 3 warm-up steps, then the median of 20, all variants
interleaved step by step in one run:

  plain       bagua_mxfp4_compress, then bagua_mxfp4_decompress of its bytes
  ef          bagua_mxfp4_compress_ef (the residual's policy as the library picks it), then
              the same decode: what the residual traffic costs the kernel behind the encode
  ef_nt0/1    the same with BAGUA_MX_EF_RESIDUAL_NT=0 / 1 (default-policy or non-temporal
              residual loads and stores)
  middle      bagua_mxfp4_reduce_requantize at p = 8 (tensor NULL, as the op calls it)
  middle_ef   bagua_mxfp4_reduce_requantize_ef at p = 8

The yardstick is the plain encode's achieved bytes per second in the same run: the
error-feedback encode moves 12.53 N bytes for f32 (4 N gradient, 4 N + 4 N residual,
0.53 N out) against 4.53 N, the middle step (p + 1) * 0.53 * cs + 8 * cs.  Writes the
record to --out and, for a file under profiles/, its index line in profiles/README.md
(--index FILE: only that, for a record copied into profiles/).

    python tools/mxfp4_ef_probe.py [--out profiles/r09_mxfp4_ef.json]
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

INDEX = ("| `{name}` | MXFP4 error-feedback kernels beside the plain ones in the same run, per kernel, 8 chunks: "
         "256 MiB f32 encode {fe:.1f} µs ({fer:.2f} TB/s) against plain {fp:.1f} µs ({fpr:.2f} TB/s), middle step "
         "at p = 8 {fm:.1f} against {fmp:.1f} µs; 2^27 bf16 encode {be:.1f} µs ({ber:.2f} TB/s) against {bp:.1f} µs "
         "({bpr:.2f} TB/s), middle {bm:.1f} against {bmp:.1f} µs; residual policy A/B and the decode behind each "
         "encode | `tools/mxfp4_ef_probe.py` |\n")


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
    worker = torch.zeros(n, dtype=torch.float32, device=dev)
    server = torch.zeros(cs, dtype=torch.float32, device=dev)
    S = K.bagua_mxfp4_compressed_bytes(cs, p)
    seg = S // p
    mx, mx_recv, mx_out = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(3))
    N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, mx_recv.data_ptr(), S, -1, sp), "recv")

    def policy(nt):
        if nt is None:
            os.environ.pop("BAGUA_MX_EF_RESIDUAL_NT", None)
        else:
            os.environ["BAGUA_MX_EF_RESIDUAL_NT"] = nt

    def decode():
        N.check(K.bagua_mxfp4_decompress(dtype_code, mx.data_ptr(), S, cs, p, dec.data_ptr(), sp), "decode")

    def plain():
        N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, sp), "encode")
        decode()

    def ef(nt):
        policy(nt)
        N.check(K.bagua_mxfp4_compress_ef(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, worker.data_ptr(),
                                          sp), "ef encode")
        policy(None)
        decode()

    def middle():
        N.check(K.bagua_mxfp4_reduce_requantize(dtype_code, mx_recv.data_ptr(), S, cs, p, None, 1, mx_out.data_ptr(), S,
                                                p // 2, sp), "middle")

    def middle_ef():
        N.check(K.bagua_mxfp4_reduce_requantize_ef(dtype_code, mx_recv.data_ptr(), S, cs, p, 1, mx_out.data_ptr(), S,
                                                   p // 2, server.data_ptr(), sp), "ef middle")

    enc_b, enc_ef_b, dec_b = n * esz + S, n * esz + 8 * n + S, S + n * esz
    # variant -> (call, [(result name, kernel, algorithmic bytes)] in launch order)
    variants = {
        "plain": (plain, [("encode", "mxfp4_encode_kernel", enc_b), ("decode_after_encode", "mxfp4_decode_kernel", dec_b)]),
        "ef": (lambda: ef(None), [("encode_ef", "mxfp4_encode_ef_kernel", enc_ef_b),
                                  ("decode_after_encode_ef", "mxfp4_decode_kernel", dec_b)]),
        "ef_nt0": (lambda: ef("0"), [("encode_ef_nt0", "mxfp4_encode_ef_kernel", enc_ef_b),
                                     ("decode_after_encode_ef_nt0", "mxfp4_decode_kernel", dec_b)]),
        "ef_nt1": (lambda: ef("1"), [("encode_ef_nt1", "mxfp4_encode_ef_kernel", enc_ef_b),
                                     ("decode_after_encode_ef_nt1", "mxfp4_decode_kernel", dec_b)]),
        "middle": (middle, [("middle_p8", "mxfp4_reduce_encode_kernel", (p + 1) * seg)]),
        "middle_ef": (middle_ef, [("middle_ef_p8", "mxfp4_reduce_encode_ef_kernel", (p + 1) * seg + 8 * cs)]),
    }
    times = {r: [] for _, parts in variants.values() for r, _, _ in parts}
    for step in range(warmup + reps):
        for name, (fn, parts) in variants.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4)]
            for a, b in evs:
                a.record(st)
                b.record(st)
            N.time_next_kernels(evs)
            fn()
            torch.cuda.synchronize()
            names = N.timed_kernel_names()
            N.time_next_kernels([])
            assert names == [k for _, k, _ in parts], (name, names)  # the kernels the variant is meant to time
            if step >= warmup:
                for (a, b), (r, _, _) in zip(evs, parts):
                    times[r].append(a.elapsed_time(b) * 1e3)
    rec = {"elements": n, "chunks": p, "bytes_per_element": esz,
           "residual_policy_default": "nt" if n * (4 + esz) > (256 << 20) else "default"}
    for _, parts in variants.values():
        for r, kernel, nbytes in parts:
            med = statistics.median(times[r])
            rec[r] = {"us": round(med, 2), "min_us": round(min(times[r]), 2), "max_us": round(max(times[r]), 2),
                      "bytes": int(nbytes), "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "kernel": kernel}
    rec["encode_ef_rate_over_plain"] = round(rec["encode_ef"]["tb_per_s"] / rec["encode"]["tb_per_s"], 3)
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
    row = INDEX.format(name=name, fe=f32["encode_ef"]["us"], fer=f32["encode_ef"]["tb_per_s"], fp=f32["encode"]["us"],
                       fpr=f32["encode"]["tb_per_s"], fm=f32["middle_ef_p8"]["us"], fmp=f32["middle_p8"]["us"],
                       be=b16["encode_ef"]["us"], ber=b16["encode_ef"]["tb_per_s"], bp=b16["encode"]["us"],
                       bpr=b16["encode"]["tb_per_s"], bm=b16["middle_ef_p8"]["us"], bmp=b16["middle_p8"]["us"])
    with open(readme, "w") as f:
        f.writelines(lines[:at] + [row] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_mxfp4_ef.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    args = ap.parse_args()
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    rec = {"probe": "mxfp4_ef", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels), median; variants interleaved per step",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
           "torch_hip": torch.version.hip,
           "f32": measure(N, N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32, 8, args.warmup, args.reps),
           "bf16": measure(N, N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16, 8, args.warmup, args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    write_index(rec, args.out)


if __name__ == "__main__":
    main()
