#!/usr/bin/env python3
"""Measurement: the MXFP8 codec's error-feedback kernels beside the plain ones (MXFP8.md,
"Error feedback").  It follows tools/mxfp4_ef_probe.py.

Two buckets, both cut into 8 chunks as the op at 8 ranks cuts them: 2^26 f32 elements
(256 MiB) and 2^27 bf16 elements.  Every call's kernels are timed alone through the library's
kernel-timing hook (bagua_time_next_kernels: device events at the kernel's own start and end);
3 warm-up steps, then the median of 20 (minimum and maximum kept beside it), all variants
interleaved step by step in one run, their order rotated by one every step:

  plain         bagua_mxfp8_compress, then bagua_mxfp8_decompress of its bytes
  ef_nt0/1      bagua_mxfp8_compress_ef of the shipped build with BAGUA_MX_EF_RESIDUAL_NT=0 / 1
                (default-policy or non-temporal residual loads and stores), then the same decode
  alt_nt0/1     the same from a second build of the kernel library with the other rows per tile
                (--alt-lib; the shipped build has R = 8 for f32 and R = 4 for f16 / bf16, so the
                second one is built with -DBAGUA_MX8_EF_ROWS_F32=4 -DBAGUA_MX8_EF_ROWS_16=8)
  middle        bagua_mxfp8_reduce_requantize at p = 8 (tensor NULL, as the op calls it)
  middle_ef     bagua_mxfp8_reduce_requantize_ef at p = 8

The yardstick is the plain encode's achieved bytes per second in the same run: the
error-feedback encode moves 13.03 N bytes for f32 (4 N gradient, 4 N + 4 N residual, 1.03 N
out) against 5.03 N, 11.03 N against 3.03 N for 16-bit T.

    python tools/mxfp8_ef_probe.py --alt-lib ab_libs/mx8ef_rows/libbagua_kernels.so [--out FILE]
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

_vp = ctypes.c_void_p


def load(N, path):
    """a second build of the kernel library under its own handle, with the in-tree signatures"""
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in N.KERNEL_SIGNATURES.items():
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
    return lib


def arm(lib, events):
    n = len(events)
    st = (_vp * max(1, n))(*[a.cuda_event for a, _ in events])
    sp = (_vp * max(1, n))(*[b.cuda_event for _, b in events])
    assert lib.bagua_time_next_kernels(st, sp, n) == 0


def timed_names(lib):
    buf = ctypes.create_string_buffer(128)
    out = []
    for i in range(lib.bagua_timed_kernels()):
        assert lib.bagua_timed_kernel_name(i, buf, 128) == 0
        out.append(buf.value.decode())
    return out


def measure(N, alt, dtype_code, tdtype, esz, n, p, warmup, reps, rows):
    K = N.K
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sp = _vp(st.cuda_stream)
    cs = n // p
    gen = torch.Generator(device=dev).manual_seed(7)
    g = (torch.randn(n, device=dev, generator=gen) * 1e-3).to(tdtype)
    dec = torch.empty(n, dtype=tdtype, device=dev)
    worker = torch.zeros(n, dtype=torch.float32, device=dev)
    server = torch.zeros(cs, dtype=torch.float32, device=dev)
    S = K.bagua_mxfp8_compressed_bytes(cs, p)
    seg = S // p
    mx, mx_recv, mx_out = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(3))
    N.check(K.bagua_mxfp8_compress(dtype_code, g.data_ptr(), n, cs, p, mx_recv.data_ptr(), S, -1, sp), "recv")

    def decode():
        N.check(K.bagua_mxfp8_decompress(dtype_code, mx.data_ptr(), S, cs, p, dec.data_ptr(), sp), "decode")

    def plain():
        N.check(K.bagua_mxfp8_compress(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, sp), "encode")

    def ef(lib, nt):
        os.environ["BAGUA_MX_EF_RESIDUAL_NT"] = nt
        N.check(lib.bagua_mxfp8_compress_ef(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, worker.data_ptr(),
                                            sp), "ef encode")
        del os.environ["BAGUA_MX_EF_RESIDUAL_NT"]

    def middle():
        N.check(K.bagua_mxfp8_reduce_requantize(dtype_code, mx_recv.data_ptr(), S, cs, p, None, 1, mx_out.data_ptr(), S,
                                                p // 2, sp), "middle")

    def middle_ef():
        N.check(K.bagua_mxfp8_reduce_requantize_ef(dtype_code, mx_recv.data_ptr(), S, cs, p, 1, mx_out.data_ptr(), S,
                                                   p // 2, server.data_ptr(), sp), "ef middle")

    enc_b, enc_ef_b, dec_b = n * esz + S, n * esz + 8 * n + S, S + n * esz
    # variant -> [(library, call, result name, kernel, algorithmic bytes)] in launch order
    variants = {"plain": [(K, plain, "encode", "mxfp8_encode_kernel", enc_b),
                          (K, decode, "decode_after_encode", "mxfp8_decode_kernel", dec_b)],
                "middle": [(K, middle, "middle_p8", "mxfp8_reduce_encode_kernel", (p + 1) * seg)],
                "middle_ef": [(K, middle_ef, "middle_ef_p8", "mxfp8_reduce_encode_ef_kernel", (p + 1) * seg + 8 * cs)]}
    for tag, lib, r in (("ef", K, rows[0]), ("alt", alt, rows[1])):
        for nt in ("0", "1") if lib is not None else ():
            key = f"encode_ef_r{r}_nt{nt}"
            variants[f"{tag}_nt{nt}"] = [(lib, lambda lib=lib, nt=nt: ef(lib, nt), key, "mxfp8_encode_ef_kernel", enc_ef_b),
                                         (K, decode, "decode_after_" + key, "mxfp8_decode_kernel", dec_b)]
    order = list(variants)
    times = {part[2]: [] for parts in variants.values() for part in parts}
    for step in range(warmup + reps):
        for name in order[step % len(order):] + order[:step % len(order)]:
            for lib, fn, r, kernel, _ in variants[name]:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(st)
                ev[1].record(st)
                arm(lib, [ev])
                fn()
                torch.cuda.synchronize()
                names = timed_names(lib)
                arm(lib, [])
                assert names == [kernel], (name, names)  # the kernel the variant is meant to time
                if step >= warmup:
                    times[r].append(ev[0].elapsed_time(ev[1]) * 1e3)
    shipped_nt = "1" if n * (4 + esz) > (256 << 20) else "0"
    rec = {"elements": n, "chunks": p, "bytes_per_element": esz, "rows_shipped": rows[0], "rows_alt": rows[1],
           "residual_policy_default": "nt" if shipped_nt == "1" else "default"}
    for parts in variants.values():
        for _, _, r, kernel, nbytes in parts:
            med = statistics.median(times[r])
            rec[r] = {"us": round(med, 2), "min_us": round(min(times[r]), 2), "max_us": round(max(times[r]), 2),
                      "bytes": int(nbytes), "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3), "kernel": kernel}
    for r in rows if alt is not None else rows[:1]:
        for nt in ("0", "1"):
            rec[f"encode_ef_r{r}_nt{nt}_rate_over_plain"] = round(rec[f"encode_ef_r{r}_nt{nt}"]["tb_per_s"] /
                                                                  rec["encode"]["tb_per_s"], 3)
    rec["encode_ef_rate_over_plain"] = rec[f"encode_ef_r{rows[0]}_nt{shipped_nt}_rate_over_plain"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--alt-lib", default=None, help="a build of libbagua_kernels.so with the other rows per tile")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_mxfp8_ef.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    alt = load(N, args.alt_lib) if args.alt_lib else None
    v = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipRuntimeGetVersion(ctypes.byref(v))
    rec = {"probe": "mxfp8_ef", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels), median with min and max; variants interleaved per step, "
                     "order rotated by one every step",
           "device": torch.cuda.get_device_name(0), "hip_runtime_version": v.value, "torch_hip": torch.version.hip,
           "f32": measure(N, alt, N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32, 8, args.warmup, args.reps, (8, 4)),
           "bf16": measure(N, alt, N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16, 8, args.warmup, args.reps,
                           (4, 8))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
