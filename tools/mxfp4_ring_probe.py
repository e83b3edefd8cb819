#!/usr/bin/env python3
"""Measurement: the decentralized ring op with the MXFP4 codec, fused kernels beside the
composed op sequence (MXFP4.md, "Ring op").

Two buckets: 2^26 f32 elements (256 MiB) and 2^27 bf16 elements, each with its weight and
the two peer weights.  The op runs through its normal entry on loopback communicators, at
one rank and at two loopback ranks on the one GPU (kernel times only there: the transport
is a copy on the same device and its time means nothing).  Every kernel is timed alone
through the library's kernel-timing hook (bagua_time_next_kernels: device events at the
kernel's own start and end, no dispatch gaps), on rank 0's thread; 3 warm-up steps, then the
median of 20, all variants interleaved step by step in one run.  Before every call the four
tensors are restored from pristine copies, so every variant sees the same values and the
same cache state (the tail of the last copy, at most).

  p = 1  one_rank   mxfp4_ring_one_rank_kernel (BAGUA_ONE_RANK_FUSED=1, the default)
         mix_apply  mxfp4_ring_mix_kernel + mxfp4_ring_apply_kernel (BAGUA_ONE_RANK_FUSED=0)
         composed   BAGUA_MXFP4_RING_FUSED=0: 3 x addmul, encode, 3 x (decode, add)
  p = 2  mix_apply, composed

The yardstick is the composed sequence in the same run.  Its eleventh step, the clone W = t,
is a device-to-device copy that the hook does not see, so the composed kernel sum leaves it
out (the fused kernels write W themselves); at one rank the whole call is timed as well,
device events around it on the op's stream, and that figure includes the copy.  A kernel's
roofline share is its algorithmic bytes over its time against 8 TB/s.  Writes the record to
--out and, for a file under profiles/, its index line in profiles/README.md.

    python tools/mxfp4_ring_probe.py [--out profiles/r10_mxfp4_ring.json]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bagua-core_amd"))

PEAK_TB_S = 8.0
INDEX = ("| `{name}` | MXFP4 ring op, fused kernels against the composed sequence in the same run, per kernel, median "
         "of {reps}: 256 MiB f32 one rank {f1:.1f} µs in one kernel against {fc:.1f} µs composed ({fr:.2f}), two "
         "ranks mix {fm:.1f} + apply {fa:.1f} µs against {fc2:.1f} µs ({fr2:.2f}); 2^27 bf16 one rank {b1:.1f} "
         "against {bcm:.1f} µs ({br:.2f}), two ranks {bm:.1f} + {ba:.1f} against {bc2:.1f} µs ({br2:.2f}) | "
         "`tools/mxfp4_ring_probe.py` |\n")


def hip_runtime_version() -> int:
    v = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipRuntimeGetVersion(ctypes.byref(v))
    return v.value


def kernel_bytes(kernel, n, esz, S):
    """algorithmic bytes of one launch on a bucket of n elements"""
    return {"mxfp4_ring_one_rank_kernel": 8 * n * esz,
            "mxfp4_ring_mix_kernel": 4 * n * esz + S,
            "mxfp4_ring_apply_kernel": 3 * S + 7 * n * esz,
            "binary_kernel": 3 * n * esz,
            "mxfp4_encode_kernel": n * esz + S,
            "mxfp4_decode_kernel": S + n * esz}[kernel]


COMPOSED = ["binary_kernel"] * 3 + ["mxfp4_encode_kernel"] + ["mxfp4_decode_kernel", "binary_kernel"] * 3
VARIANTS = {
    "one_rank": ({"BAGUA_ONE_RANK_FUSED": "1"}, ["mxfp4_ring_one_rank_kernel"]),
    "mix_apply": ({"BAGUA_ONE_RANK_FUSED": "0"}, ["mxfp4_ring_mix_kernel", "mxfp4_ring_apply_kernel"]),
    "composed": ({"BAGUA_MXFP4_RING_FUSED": "0"}, COMPOSED),
}


def measure(bc, N, dtype_code, tdtype, esz, n, p, variants, warmup, reps):
    from bagua_core.communicator import loopback_communicators
    dev = torch.device("cuda", 0)
    comms = loopback_communicators(p, 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    pristine = [[(torch.randn(n, device=dev, generator=gen) * 1e-3).to(tdtype) for _ in range(4)] for _ in range(p)]
    work = [[torch.empty_like(x) for x in rank] for rank in pristine]
    raws = [[bc.BaguaTensorPy(x, f"r{r}.{k}").raw() for k, x in enumerate(work[r])] for r in range(p)]
    S = N.K.bagua_mxfp4_compressed_bytes(n, 1)
    st0 = torch.cuda.ExternalStream(comms[0].stream_ptr())
    times = {v: [[] for _ in VARIANTS[v][1]] for v in variants}
    calls = {v: [] for v in variants}

    def step(variant, keep):
        env, kernels = VARIANTS[variant]
        for r in range(p):
            for x, src in zip(work[r], pristine[r]):
                x.copy_(src)
        torch.cuda.synchronize()
        os.environ.update(env)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in kernels]
        for a, b in evs:
            a.record(st0)
            b.record(st0)
        whole = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        names, errs = [], []

        def rank(r):
            try:
                refs = [ctypes.byref(x) for x in raws[r]]
                if r == 0:
                    N.time_next_kernels(evs)
                    whole[0].record(st0)
                rc = N.C.bagua_decentralized_low_precision_synchronous(comms[r].handle, *refs, N.COMPRESSION_MXFP4)
                if r == 0:
                    whole[1].record(st0)
                    names.extend(N.timed_kernel_names())
                    N.time_next_kernels([])
                N.check(rc, f"{variant} rank {r}")
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=rank, args=(r,)) for r in range(p)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        torch.cuda.synchronize()
        for k in env:
            os.environ.pop(k)
        if errs:
            raise errs[0]
        assert names == kernels, (variant, names)  # the kernels the variant is meant to time
        if keep:
            for i, (a, b) in enumerate(evs):
                times[variant][i].append(a.elapsed_time(b) * 1e3)
            calls[variant].append(whole[0].elapsed_time(whole[1]) * 1e3)

    for s in range(warmup + reps):
        for v in variants:
            step(v, s >= warmup)
    rec = {"elements": n, "ranks": p, "bytes_per_element": esz, "segment_bytes": int(S)}
    for v in variants:
        ks = []
        for kernel, ts in zip(VARIANTS[v][1], times[v]):
            med, nbytes = statistics.median(ts), kernel_bytes(kernel, n, esz, S)
            rate = nbytes / (med * 1e-6) / 1e12
            ks.append({"kernel": kernel, "us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                       "bytes": int(nbytes), "tb_per_s": round(rate, 3), "roofline_share": round(rate / PEAK_TB_S, 3)})
        rec[v] = {"kernels": ks, "kernel_sum_us": round(sum(k["us"] for k in ks), 2)}
        if p == 1:  # the whole call, the clone of the composed sequence included
            rec[v]["call_us"] = round(statistics.median(calls[v]), 2)
    for v in variants:
        if v != "composed":
            rec[v]["kernel_sum_over_composed"] = round(rec[v]["kernel_sum_us"] / rec["composed"]["kernel_sum_us"], 3)
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
    at = max((i for i, ln in enumerate(lines) if re.match(r"\| `r\d\d_", ln)), default=len(lines) - 1) + 1
    f1, f2, b1, b2 = rec["f32_p1"], rec["f32_p2"], rec["bf16_p1"], rec["bf16_p2"]

    def us(r, v, i=None):
        return r[v]["kernel_sum_us"] if i is None else r[v]["kernels"][i]["us"]

    row = INDEX.format(name=name, reps=rec["reps"], f1=us(f1, "one_rank"), fc=us(f1, "composed"),
                       fr=f1["one_rank"]["kernel_sum_over_composed"], fm=us(f2, "mix_apply", 0), fa=us(f2, "mix_apply", 1),
                       fc2=us(f2, "composed"), fr2=f2["mix_apply"]["kernel_sum_over_composed"],
                       b1=us(b1, "one_rank"), bcm=us(b1, "composed"), br=b1["one_rank"]["kernel_sum_over_composed"],
                       bm=us(b2, "mix_apply", 0), ba=us(b2, "mix_apply", 1), bc2=us(b2, "composed"),
                       br2=b2["mix_apply"]["kernel_sum_over_composed"])
    with open(readme, "w") as f:
        f.writelines(lines[:at] + [row] + lines[at:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n-f32", type=int, default=26)
    ap.add_argument("--log2n-bf16", type=int, default=27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_mxfp4_ring.json"))
    ap.add_argument("--index", default=None, help="write the index row of an existing record and exit")
    args = ap.parse_args()
    if args.index:
        write_index(json.load(open(args.index)), args.index)
        return
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    import bagua_core as bc
    from bagua_core import _native as N
    for k in ("BAGUA_ONE_RANK_FUSED", "BAGUA_MXFP4_RING_FUSED"):
        os.environ.pop(k, None)
    rec = {"probe": "mxfp4_ring", "warmup": args.warmup, "reps": args.reps,
           "timing": "per kernel (bagua_time_next_kernels) on rank 0, median; variants interleaved per step; the "
                     "composed sequence's clone W = t is a copy the hook does not see (call_us includes it)",
           "peak_tb_per_s": PEAK_TB_S, "device": torch.cuda.get_device_name(0),
           "hip_runtime_version": hip_runtime_version(), "torch_hip": torch.version.hip}
    one, two = ("one_rank", "mix_apply", "composed"), ("mix_apply", "composed")
    for name, code, tdtype, esz, n in (("f32", N.DTYPE_F32, torch.float32, 4, 1 << args.log2n_f32),
                                       ("bf16", N.DTYPE_BF16, torch.bfloat16, 2, 1 << args.log2n_bf16)):
        rec[f"{name}_p1"] = measure(bc, N, code, tdtype, esz, n, 1, one, args.warmup, args.reps)
        rec[f"{name}_p2"] = measure(bc, N, code, tdtype, esz, n, 2, two, args.warmup, args.reps)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    write_index(rec, args.out)


if __name__ == "__main__":
    main()
