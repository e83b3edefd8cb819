"""Hand-built MinMax-UInt8 receive buffers for the fused reduce and ring-apply tests.

A compressor only ever emits well-formed headers, so the kernels that build their
dequantisation tables from *received* headers (reduce.hip build_luts, decentralized.hip
ring_apply_kernel) never see a degenerate one in the op tests.  Here the header values and
payload bytes are written directly: p segments in the wire format, stride `stride(cs)`
(a multiple of 32, as the op's buffers are: S % p == 0), header {T min, T max} at 0, zero
gap, payload at +32, zero slack.

Each named class applies to segment k; every other segment is benign (header -+1e-3,
uniform random bytes).  What a header decodes to follows K:424-432, K:465-467:
    scale = 255 / (max - min + 1e-7),  ub = rint(max * scale),  lb = ub - 255,
    value = (byte + lb) / scale, rounded to T.

  nan_min / nan_max / nan_both   NaN scale or NaN ub: the segment decodes to NaN
  neg_inf_min   {-inf, 1e-3}: scale +0, ub 0: -inf below byte 255, NaN at 255
  pos_inf_max   {-1e-3, +inf}, both_inf {-inf, +inf}: ub = rint(inf * 0) = NaN: all NaN
  inverted      {0.25, -0.25}: negative scale, values decrease with the byte
  empty_init    {+T_MAX, -T_MAX}, bytes 255: the encoder's header of a chunk with no valid
                element; NaN in f32 / bf16 (scale -0, 0 / -0).  In f16 the range is finite
                (scale -255/131008): byte 255 decodes to -65760, which rounds to -inf in f16
  constant      {0.5, 0.5}: scale 255e7
  huge_range    f32 / bf16 {-3e38, 3e38}: max - min overflows, scale +0: -inf and NaN.
                f16 {-65504, 65504} in EVERY segment with the extreme bytes on the first
                elements: the p-fold sum overflows f16 to +-inf when average = 0
  denormal      EVERY segment has the header {-denormal of T, 0} (byte 255 decodes to +0) and bytes
                near 255.  The
                format's 1e-7 keeps |scale| <= 2.55e9 (or >= 1e-7 / ulp = 3.6e16 through
                cancellation), so a decoded nonzero magnitude is at least 2.8e-17: denormal
                in f16 only, where the values are {-0, +0, -6e-8, -1.2e-7, ...} and the
                mean underflows to -0 (the sum cannot: f16 values add exactly in f32, and
                +0 + -0 = +0).  In f32 / bf16 no received buffer can make a decoded
                or reduced value denormal, and -0 cannot reach the reduced chunk at all
                (every partial sum starts as 0.0f + x, and +0 + -0 = +0): there the class
                yields +0 and the smallest magnitudes the format can carry.  (Denormals and
                -0 of f32 / bf16 are driven through bagua_reduce_chunks instead, which takes
                arbitrary values: test_gpu_reduce_edges.py.)
  signed_zero_min   (added for the min/max fold) EVERY segment {-denormal, +denormal} of T.  In
                f16 the reduced chunk with average = 1 is {+0, -0, positive denormals}: its
                minimum is -0 (header bits 0x8000), and every -0 sits behind a +0 in its
                16-byte vector, so a fold that compares floats (-0 < +0 is false) instead
                of ordered keys keeps +0.  f32 / bf16 cannot carry -0 (see `denormal`).
  inf_cancel    segment k {-inf, 1} decodes to -inf, segment (k + 1) % p {+inf, 1} (scale
                -0) to +inf on the same elements: the sum is NaN
  every_segment_nan   all p headers NaN: the reduced chunk is all NaN, the requantised
                header must be the init header {+T_MAX, -T_MAX}
  payload_all_0 / payload_all_255   benign header, constant payload
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np as NP

F32, F16, BF16 = 0, 1, 2
STORAGE = {F32: np.float32, F16: np.float16, BF16: np.uint16}
NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}

# chunk size of the crafted buffers: two full tiles, a partial tile and a sub-tile remainder
# of the fused kernels for every (dtype, tree width); a tile is 256 * 64 / BY elements
CS = 2 * 8192 + 8 * 37

CLASSES = ["nan_min", "nan_max", "nan_both", "neg_inf_min", "pos_inf_max", "both_inf", "inverted", "empty_init",
           "constant", "huge_range", "denormal", "inf_cancel", "every_segment_nan", "payload_all_0",
           "payload_all_255", "signed_zero_min"]
NAN, INF = float("nan"), float("inf")


def reduce_by(p: int) -> int:
    """width of the reference's summation tree (K:502-531)"""
    return 2 if p <= 4 else 4 if p <= 8 else 8 if p <= 16 else 16 if p <= 32 else 32


def positions(p: int) -> list[int]:
    """segment indices worth placing a hostile segment at: first, last, and the first segment
    of the tree's second round"""
    ks = {0, p - 1}
    if p > reduce_by(p):
        ks.add(reduce_by(p))
    return sorted(ks)


def stride(cs: int) -> int:
    return (cs + 31) // 32 * 32 + 32


def init_max(dtype: int) -> float:
    return float(NP.INIT_MAX[dtype])


def header_values(cls: str, dtype: int) -> tuple[float, float]:
    """{min, max} of the hostile segment of a one-segment class"""
    big = init_max(dtype)
    tiny = 6e-8 if dtype == F16 else 1e-40  # a denormal of T
    return {
        "benign": (-1e-3, 1e-3),
        "nan_min": (NAN, 1e-3), "nan_max": (-1e-3, NAN), "nan_both": (NAN, NAN),
        "neg_inf_min": (-INF, 1e-3), "pos_inf_max": (-1e-3, INF), "both_inf": (-INF, INF),
        "inverted": (0.25, -0.25),
        "empty_init": (big, -big),
        "constant": (0.5, 0.5),
        "huge_range": (-65504.0, 65504.0) if dtype == F16 else (-3e38, 3e38),
        "denormal": (-tiny, 0.0), "signed_zero_min": (-tiny, tiny),
        "inf_cancel": (-INF, 1.0),
        "every_segment_nan": (NAN, NAN),
        "payload_all_0": (-1e-3, 1e-3), "payload_all_255": (-1e-3, 1e-3),
    }[cls]


def zero_byte(dtype: int, mn: float, mx: float) -> int:
    """the payload byte that decodes to zero under the header {mn, mx} (-lb, K:465-467)"""
    h = NP.to_f32(NP.from_f32(np.array([mn, mx], np.float32), dtype), dtype)
    return int(-NP.qparams(h[0], h[1])[1])


def one_segment(cls: str, dtype: int, cs: int, rng) -> tuple[float, float, np.ndarray]:
    """(min, max, payload) of one hostile segment (the ring tests build one-segment buffers)"""
    mn, mx = header_values(cls, dtype)
    pay = rng.integers(0, 256, cs, dtype=np.uint8)
    if cls in ("empty_init", "payload_all_255"):
        pay[:] = 255
    elif cls == "payload_all_0":
        pay[:] = 0
    elif cls == "denormal":
        pay = rng.choice(np.array([255, 255, 255, 254, 253, 250, 128, 0], np.uint8), cs)
    elif cls == "signed_zero_min":
        pay = rng.choice(np.array([zero_byte(dtype, mn, mx), 255], np.uint8), cs)  # zero or the maximum
    return mn, mx, pay


def build_received(dtype: int, cs: int, segs) -> np.ndarray:
    """p segments (min, max, payload bytes) -> the receive buffer, p * stride(cs) bytes"""
    co, es = stride(cs), NP.esize(dtype)
    buf = np.zeros(len(segs) * co, np.uint8)
    for c, (mn, mx, pay) in enumerate(segs):
        with np.errstate(all="ignore"):
            h = NP.from_f32(np.array([mn, mx], np.float32), dtype)
        buf[c * co:c * co + 2 * es] = h.view(np.uint8)
        assert pay.size == cs and pay.dtype == np.uint8
        buf[c * co + 32:c * co + 32 + cs] = pay
    return buf


def crafted(cls: str, dtype: int, p: int, cs: int, k: int, seed: int = 0) -> np.ndarray:
    """The receive buffer of class `cls` with its hostile segment at index k."""
    rng = np.random.default_rng([seed, CLASSES.index(cls) if cls in CLASSES else 99, dtype, p, k])
    segs = [one_segment("benign", dtype, cs, rng) for _ in range(p)]
    if cls == "benign":
        return build_received(dtype, cs, segs)
    everywhere = cls in ("every_segment_nan", "denormal", "signed_zero_min") or (cls == "huge_range" and dtype == F16)
    for c in range(p) if everywhere else [k]:
        segs[c] = one_segment(cls, dtype, cs, rng)
    if cls == "inf_cancel":
        k2 = (k + 1) % p
        segs[k2] = (INF, 1.0, segs[k2][2])
        for c in (k, k2):
            segs[c][2][:cs // 2] = np.minimum(segs[c][2][:cs // 2], 254)  # +-inf, not the 0 / 0 of byte 255
    if cls == "huge_range" and dtype == F16:
        for c in range(p):  # every segment at its largest / smallest value on the same elements
            segs[c][2][0:16] = 254
            segs[c][2][16:32] = 0
    if cls == "denormal":
        for c in range(p):
            segs[c][2][0:32] = 255                       # all zero: +0
            segs[c][2][32:64] = 128 if c == k else 255   # one segment below zero (f16: its smallest denormal)
    if cls == "signed_zero_min":
        z = zero_byte(dtype, *header_values(cls, dtype))
        below = np.where(np.arange(32) % 4 == 0, z, max(z - 60, 0)).astype(np.uint8)
        for c in range(p):
            segs[c][2][0:32] = z                          # +0
            segs[c][2][32:64] = below if c == k else z    # f16: one smallest denormal below zero, behind a +0
    return build_received(dtype, cs, segs)


def to_f32(x: np.ndarray, dtype: int) -> np.ndarray:
    return NP.to_f32(x.view(STORAGE[dtype]), dtype)


def middle_step(backend, recv: np.ndarray, dtype: int, p: int, cs: int, target: int, average: bool):
    """The reference's middle step on a receive buffer (centralized_low_precision_synchronous.rs:40-60):
    decompress_from, reduce_{mean,sum}_inplace(target), compress(target).  Returns the decoded
    tensor (p * cs), the reduced chunk (cs) and the requantised segment laid out with this
    module's stride (header, zero gap, payload, zero slack)."""
    t = np.zeros(p * cs, STORAGE[dtype])
    backend.decompress_minmax_u8(recv, p, t, dtype)
    dec = t.copy()
    backend.reduce_chunks(t, dtype, p, target, bool(average))
    comp = backend.compress_minmax_u8(t, dtype, p, target)
    cof = comp.size // p
    seg = np.zeros(stride(cs), np.uint8)
    seg[:32 + cs] = comp[target * cof:target * cof + 32 + cs]
    assert not comp[target * cof + 32 + cs:(target + 1) * cof].any()
    return dec, t[target * cs:(target + 1) * cs].copy(), seg


def decode_segment(backend, seg: np.ndarray, dtype: int, cs: int) -> np.ndarray:
    out = np.zeros(cs, STORAGE[dtype])
    backend.decompress_minmax_u8(seg, 1, out, dtype)
    return out


def header_of(seg: np.ndarray, dtype: int) -> np.ndarray:
    """the two header values of a segment, as raw T storage"""
    return seg[:2 * NP.esize(dtype)].view(STORAGE[dtype]).copy()


def init_header(dtype: int) -> np.ndarray:
    m = init_max(dtype)
    return NP.from_f32(np.array([m, -m], np.float32), dtype)
