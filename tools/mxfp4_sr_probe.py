#!/usr/bin/env python3
"""Measurement: the MXFP4 codec's stochastic rounding (MXFP4.md, "Stochastic rounding").

Two parts, one record:

  instruction   What gfx950's v_cvt_scalef32_sr_pk_fp4_f32 does with its seed operand, on the
                boundary table of tests/mxfp4_boundary_cases.py (every grid boundary, its
                neighbours in T, every scale byte) in f32, f16 and bf16, each value scaled by
                its block's plain scale byte as the kernels would scale it.  Seeds 0, all
                ones and the 32 single bits give, per grid region, the fraction at which each
                seed bit starts to round a value up (so which bits the instruction adds, and
                where); pairs (x, x) under random seeds tell whether the two packed elements
                share the seed; then every feeding of the contract's 16-bit r as
                seed = r << s (s = 0..16, low bits zero or one) is compared with the contract's
                code, element by element, with the element alone in either lane.  The
                instruction runs in the stand-alone program tools/mxfp4_sr_cvt_probe.hip.
  timing        The plain, error-feedback and stochastic encodes and the three middle steps at
                p = 8, per kernel through bagua_time_next_kernels, interleaved step by step in
                one run, 3 warm-up steps and the median of 20: 2^26 f32 elements (256 MiB)
                and 2^27 bf16.  The stochastic encode moves the plain encode's bytes, so the
                plain encode of the same run is its yardstick.

    python tools/mxfp4_sr_probe.py [--part instruction|timing|both] [--out profiles/r12_mxfp4_sr.json]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bagua-core_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CVT_SRC = os.path.join(ROOT, "tools", "mxfp4_sr_cvt_probe.hip")
CVT_EXE = os.path.join(ROOT, "tools", "mxfp4_sr_cvt_probe")
REGIONS = ("below 1 (fp4 denormal)", "1 to 2", "2 to 4", "4 to 6")

INDEX = ("| `{name}` | MXFP4 stochastic rounding: what `v_cvt_scalef32_sr_pk_fp4_f32` does with its seed on the "
         "boundary table (adopted: {adopted}), and the stochastic encode beside the plain and error-feedback ones in "
         "the same run, per kernel, 8 chunks: 256 MiB f32 {fs:.1f} µs against plain {fp:.1f} and EF {fe:.1f} µs, "
         "middle step at p = 8 {fms:.1f} against {fmp:.1f} and {fme:.1f} µs; 2^27 bf16 {bs:.1f} against {bp:.1f} and "
         "{be:.1f} µs, middle {bms:.1f} against {bmp:.1f} and {bme:.1f} µs | `tools/mxfp4_sr_probe.py` |\n")


# ---------------------------------------------------------------- instruction ----
def run_rows(x0, x1, scale_bits, seed):
    """one instruction per row; returns (nibble of x0, nibble of x1)"""
    if not os.path.exists(CVT_EXE):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", CVT_SRC, "-o", CVT_EXE], check=True)
    n = x0.size
    rows = np.zeros(n, dtype=[("x0", "<f4"), ("x1", "<f4"), ("scale", "<u4"), ("seed", "<u4")])
    rows["x0"], rows["x1"], rows["scale"], rows["seed"] = x0, x1, scale_bits, seed
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "rows.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(np.uint64(n).tobytes())
            f.write(rows.tobytes())
        subprocess.run([CVT_EXE, src, dst], check=True, timeout=120)
        out = np.fromfile(dst, np.uint8)
    assert out.size == n
    return out & 15, out >> 4


def table_elements(dtype):
    """the boundary table as the kernels feed the conversion: (x as f32, scale bits byte << 23, floor
    code, F, exact fraction, region, sign) per element"""
    import mxfp4_boundary_cases as B
    import mxfp4_reference as R
    import mxfp4_sr_reference as SR
    x = B.table(dtype).values()
    byte, _ = R.encode_blocks(x, dtype)
    e = byte.astype(np.int64) - 127
    y = np.ldexp(np.abs(x), -e[:, None])
    lo, F, step = SR.floor_code_and_fraction(y)
    q = y / step
    frac = q - np.floor(q)
    region = np.where(y < 1, 0, np.where(y < 2, 1, np.where(y < 4, 2, 3)))
    scale_bits = np.repeat(byte.astype(np.uint32) << 23, 32)
    return (x.astype(np.float32).ravel(), scale_bits, lo.ravel(), F.ravel(), frac.ravel(), region.ravel(),
            np.signbit(x).ravel())


def probe_instruction():
    import mxfp4_sr_reference as SR
    rec = {}
    for dtype, name in ((0, "f32"), (1, "f16"), (2, "bf16")):
        x, sb, lo, F, frac, region, sign = table_elements(dtype)
        n = x.size
        zero = np.zeros(n, np.float32)
        rng = np.random.default_rng(12 + dtype)
        key = SR.key(0x5EED, dtype)
        r = SR.rbits(key, np.arange(n, dtype=np.uint64)).astype(np.uint64)
        want = (lo + ((F + r.astype(np.int64)) >> 16)).astype(np.uint8) | np.where(sign, 8, 0).astype(np.uint8)
        # every row set of this dtype in one run of the program: tag -> (x0, x1, seed)
        sets = {"zero": (x, zero, np.zeros(n, np.uint32)), "ones": (x, zero, np.full(n, 0xFFFFFFFF, np.uint32))}
        for b in range(32):  # single bits: the element alone in lane 0
            sets[f"bit{b}"] = (x, zero, np.full(n, 1 << b, np.uint32))
        for k in range(8):   # do the two packed elements share the seed?  (x, x) under random seeds
            sets[f"pair{k}"] = (x, x, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        for s in range(17):  # the contract's r fed as seed = r << s (| low ones), the element alone in either lane
            for fill in (0, 1):
                seed = ((r << np.uint64(s)) | np.uint64(((1 << s) - 1) * fill)).astype(np.uint32)
                tag = f"r<<{s}" + ("|ones" if fill else "")
                sets[f"feed0 {tag}"] = (x, zero, seed)
                sets[f"feed1 {tag}"] = (zero, x, seed)
        g0, g1 = run_rows(np.concatenate([v[0] for v in sets.values()]), np.concatenate([v[1] for v in sets.values()]),
                          np.tile(sb, len(sets)), np.concatenate([v[2] for v in sets.values()]))
        got = {tag: (g0[i * n:(i + 1) * n], g1[i * n:(i + 1) * n]) for i, tag in enumerate(sets)}
        off = frac > 0
        base, ones = got["zero"][0], got["ones"][0]
        d = {"elements": int(n), "off_grid": int(off.sum()),
             "seed_0_truncates": int(((base & 7) == lo).sum()),
             "seed_0_sign_kept": int(((base & 8) != 0)[sign].sum()), "negative_elements": int(sign.sum()),
             "seed_ones_rounds_up_off_grid": int(((ones & 7)[off] == lo[off] + 1).sum()),
             "seed_ones_moves_grid_values": int(((ones & 7)[~off] != lo[~off]).sum())}
        bits = {}
        for b in range(32):
            up = (got[f"bit{b}"][0] & 7) == lo + 1
            per = {}
            for q, rn in enumerate(REGIONS):
                m = (region == q) & off
                if not m.any():
                    continue
                ups, stay = frac[m & up], frac[m & ~up]
                # the bit's weight in units of the grid step: a fraction f rounds up iff f + weight >= 1
                per[rn] = {"rounded_up": int(ups.size), "of": int(m.sum()),
                           "smallest_fraction_up": float(ups.min()) if ups.size else None,
                           "largest_fraction_staying": float(stay.max()) if stay.size else None}
            bits[str(b)] = per
        d["single_bit"] = bits
        d["pair_x_x_nibbles_differing"] = int(sum((got[f"pair{k}"][0] != got[f"pair{k}"][1]).sum() for k in range(8)))
        feeds = {}
        for s in range(17):
            for fill in (0, 1):
                tag = f"r<<{s}" + ("|ones" if fill else "")
                feeds[tag] = {"lane0_mismatches": int((got[f"feed0 {tag}"][0] != want).sum()),
                              "lane1_mismatches": int((got[f"feed1 {tag}"][1] != want).sum())}
        d["feeding_of_contract_r"] = feeds
        best = min(feeds, key=lambda t: feeds[t]["lane0_mismatches"])
        d["best_feeding"] = {"feeding": best, **feeds[best]}
        rec[name] = d
    return summarise_instruction(rec)


def summarise_instruction(rec):
    """which feedings reproduce the contract on the whole table in all three dtypes, per lane, and
    what follows for the kernels (also applied to a stored record: --summarise FILE)"""
    dts = [d for d in ("f32", "f16", "bf16") if d in rec]
    tags = list(rec[dts[0]]["feeding_of_contract_r"])
    for lane in ("lane0", "lane1"):
        rec[f"{lane}_exact_feedings"] = [t for t in tags if all(
            rec[d]["feeding_of_contract_r"][t][f"{lane}_mismatches"] == 0 for d in dts)]
    both = [t for t in rec["lane0_exact_feedings"] if t in rec["lane1_exact_feedings"]]
    rec["feedings_exact_in_both_lanes"] = both
    per_element = bool(rec["lane0_exact_feedings"]) and bool(rec["lane1_exact_feedings"])
    rec["contract_reproduced"] = {"one_conversion_per_pair": bool(both), "one_conversion_per_element": per_element}
    rec["adopted"] = False
    rec["why"] = ("no feeding of the contract's r reproduces its codes on the whole table" if not per_element else
                  "the contract is reproduced only with one conversion per element (the two lanes take overlapping "
                  "seed bits); that path is not built, so it has not been shown faster in the interleaved probe")
    return rec


# --------------------------------------------------------------------- timing ----
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
    S = K.bagua_mxfp4_compressed_bytes(cs, p)
    seg = S // p
    mx, mx_recv, mx_out = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(3))
    N.check(K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, mx_recv.data_ptr(), S, -1, sp), "recv")
    key = K.bagua_mxfp4_sr_key(1, 0, 0, 0)
    calls = {
        "encode": lambda: K.bagua_mxfp4_compress(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, sp),
        "encode_ef": lambda: K.bagua_mxfp4_compress_ef(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1,
                                                       worker.data_ptr(), sp),
        "encode_sr": lambda: K.bagua_mxfp4_compress_sr(dtype_code, g.data_ptr(), n, cs, p, mx.data_ptr(), S, -1, key, sp),
        "middle_p8": lambda: K.bagua_mxfp4_reduce_requantize(dtype_code, mx_recv.data_ptr(), S, cs, p, None, 1,
                                                             mx_out.data_ptr(), S, p // 2, sp),
        "middle_ef_p8": lambda: K.bagua_mxfp4_reduce_requantize_ef(dtype_code, mx_recv.data_ptr(), S, cs, p, 1,
                                                                   mx_out.data_ptr(), S, p // 2, server.data_ptr(), sp),
        "middle_sr_p8": lambda: K.bagua_mxfp4_reduce_requantize_sr(dtype_code, mx_recv.data_ptr(), S, cs, p, 1,
                                                                   mx_out.data_ptr(), S, p // 2, key, sp),
    }
    kernels = {"encode": "mxfp4_encode_kernel", "encode_ef": "mxfp4_encode_ef_kernel", "encode_sr": "mxfp4_encode_kernel",
               "middle_p8": "mxfp4_reduce_encode_kernel", "middle_ef_p8": "mxfp4_reduce_encode_ef_kernel",
               "middle_sr_p8": "mxfp4_reduce_encode_kernel"}
    nbytes = {"encode": n * esz + S, "encode_ef": n * esz + 8 * n + S, "encode_sr": n * esz + S,
              "middle_p8": (p + 1) * seg, "middle_ef_p8": (p + 1) * seg + 8 * cs, "middle_sr_p8": (p + 1) * seg}
    times = {k: [] for k in calls}
    for step in range(warmup + reps):
        for name, fn in calls.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2)]
            for a, b in evs:
                a.record(st)
                b.record(st)
            N.time_next_kernels(evs)
            N.check(fn(), name)
            torch.cuda.synchronize()
            names = N.timed_kernel_names()
            N.time_next_kernels([])
            assert names == [kernels[name]], (name, names)
            if step >= warmup:
                times[name].append(evs[0][0].elapsed_time(evs[0][1]) * 1e3)
    rec = {"elements": n, "chunks": p, "bytes_per_element": esz}
    for name in calls:
        med = statistics.median(times[name])
        rec[name] = {"us": round(med, 2), "min_us": round(min(times[name]), 2), "max_us": round(max(times[name]), 2),
                     "bytes": int(nbytes[name]), "tb_per_s": round(nbytes[name] / (med * 1e-6) / 1e12, 3),
                     "kernel": kernels[name]}
    rec["encode_sr_over_plain"] = round(rec["encode_sr"]["us"] / rec["encode"]["us"], 3)
    rec["encode_sr_over_ef"] = round(rec["encode_sr"]["us"] / rec["encode_ef"]["us"], 3)
    rec["middle_sr_over_plain"] = round(rec["middle_sr_p8"]["us"] / rec["middle_p8"]["us"], 3)
    rec["middle_sr_over_ef"] = round(rec["middle_sr_p8"]["us"] / rec["middle_ef_p8"]["us"], 3)
    return rec


def probe_timing(args):
    import torch
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    from bagua_core import _native as N
    return {"warmup": args.warmup, "reps": args.reps,
            "timing": "per kernel (bagua_time_next_kernels), median; variants interleaved per step",
            "device": torch.cuda.get_device_name(0), "hip_runtime_version": hip_runtime_version(),
            "torch_hip": torch.version.hip,
            "f32": measure(N, torch, N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32, 8, args.warmup, args.reps),
            "bf16": measure(N, torch, N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16, 8, args.warmup, args.reps)}


def write_index(rec, out):
    """the record's index row in profiles/README.md, below the last row of the probes' table (files
    named rNN_...), when `out` lies under profiles/ and has no row yet"""
    prof = os.path.join(ROOT, "profiles")
    if os.path.dirname(os.path.abspath(out)) != prof or "timing" not in rec:
        return
    readme, name = os.path.join(prof, "README.md"), os.path.basename(out)
    lines = open(readme).read().splitlines(keepends=True)
    if any(f"`{name}`" in ln for ln in lines):
        return
    f32, b16 = rec["timing"]["f32"], rec["timing"]["bf16"]
    at = max((i for i, ln in enumerate(lines) if re.match(r"\| `r\d\d_", ln)), default=len(lines) - 1) + 1
    row = INDEX.format(name=name, adopted="yes" if rec.get("instruction", {}).get("adopted") else "no",
                       fs=f32["encode_sr"]["us"], fp=f32["encode"]["us"], fe=f32["encode_ef"]["us"],
                       fms=f32["middle_sr_p8"]["us"], fmp=f32["middle_p8"]["us"], fme=f32["middle_ef_p8"]["us"],
                       bs=b16["encode_sr"]["us"], bp=b16["encode"]["us"], be=b16["encode_ef"]["us"],
                       bms=b16["middle_sr_p8"]["us"], bmp=b16["middle_p8"]["us"], bme=b16["middle_ef_p8"]["us"])
    with open(readme, "w") as f:
        f.writelines(lines[:at] + [row] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("instruction", "timing", "both"), default="both")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_mxfp4_sr.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    ap.add_argument("--summarise", default=None, help="redo the summary of a stored record's instruction part and exit")
    args = ap.parse_args()
    if args.summarise:
        rec = json.load(open(args.summarise))
        summarise_instruction(rec["instruction"])
        with open(args.summarise, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        return
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    rec = {"probe": "mxfp4_sr"}
    if os.path.exists(args.out):  # the two parts may be measured in separate runs
        rec.update(json.load(open(args.out)))
    if args.part in ("instruction", "both"):
        rec["instruction"] = probe_instruction()
    if args.part in ("timing", "both"):
        rec["timing"] = probe_timing(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    summary = {k: v for k, v in rec.items() if k != "instruction"}
    if "instruction" in rec:
        ins = rec["instruction"]
        summary["instruction"] = {k: (v if not isinstance(v, dict) else
                                      {kk: vv for kk, vv in v.items() if kk not in ("single_bit", "feeding_of_contract_r")})
                                  for k, v in ins.items()}
    print(json.dumps(summary))
    write_index(rec, args.out)


if __name__ == "__main__":
    main()
