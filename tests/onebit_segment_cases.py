"""Hand-built 1-bit receive buffers for the fused middle step and the decoders.

Every received 1-bit segment the op tests see comes from the encoder, whose scale is
mean|x|: non-negative, NaN / inf only when the input was.  The kernels that turn a *received*
scale into their +-scale tables (onebit.hip onebit_reduce_encode_lut_kernel and
onebit_reduce_encode_kernel, onebit_ef.hip onebit_reduce_encode_ef_kernel) therefore never
meet a negative, -0, NaN, cancelling-inf, denormal or overflowing scale.  Here the scale and
the bit bytes are written directly: p segments in the wire format of DESIGN.md §4, stride
stride(p, cs) = onebit_compressed_size(p, cs) / p, f32 scale at byte 0, u32 count at byte 4,
bit tiles from byte 32 (128 B per 1024 elements; element sub * 256 + lane * 4 + e of a tile is
bit sub * 4 + e of the little-endian 16-bit field at byte 2 * lane), zero slack.

A named class applies to segment k; every other segment is benign (scale 1e-3 * (1 + c),
uniform random bit bytes -- the padding bits of the ragged last tile included).  A segment
decodes to bit ? -scale : +scale, stored in T.

  nan_scale         scale NaN: the segment and every reduced value is NaN
  neg_scale         -1e-3: a 0 bit decodes negative (the tables' sign tests flip)
  neg_zero_scale    -0: a 0 bit decodes to -0, a 1 bit to +0
  zero_scale        +0
  pos_inf / neg_inf +-inf
  inf_cancel        segment k +inf, segment (k + 1) % p -inf: NaN where their bits agree
                    (p = 1: only the +inf segment, no NaN)
  denormal_f32      1e-40: a denormal of f32, a denormal of bf16 (rounds to 2^-133), +-0 in f16
  denormal_16       3e-8: rounds to the smallest denormal of f16 (2^-24); normal in f32 / bf16
  overflow_16       f16 1e5, bf16 3.4e38: finite in f32, +-inf when stored in T.  f32: EVERY
                    segment 3.4e38, so the sum of two same-signed values overflows (p >= 2)
  equal_cancel      every segment has the scale 1e-3: for even p many sums are exactly +0
                    (x + -x = +0 in round-to-nearest), which must re-encode as bit 0
  every_segment_nan all p scales NaN
  bits_all_0 / bits_all_1   benign scale, constant bits
  bits_marker       in EVERY segment the field of lane l, tile t, segment c is
                    (l * 73 + t * 11 + c * 4099) & 0xffff: every lane and segment is
                    distinguishable, so a wrong transpose, nibble or pair index shows
  padding_bits_set  all bits past cs in the ragged last tile are 1 in EVERY segment: the
                    re-encoded padding bits must be 0 and the tile partial must not count them
  garbage_header    count field 0xFFFFFFFF and bytes 8..31 nonzero in EVERY segment:
                    decoders read only the scale
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np as NP

F32, F16, BF16 = 0, 1, 2
STORAGE = {F32: np.float32, F16: np.float16, BF16: np.uint16}
NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
TILE, TILE_BYTES = NP.OB_TILE, NP.OB_TILE_BYTES

# ten full tiles (the table paths) and one ragged tile (the per-element path).  With
# BAGUA_TUNE_OB_MIDDLE_BLOCKS=1 (four waves) every wave takes more than one loop trip, the
# last two-tile batch of waves 0-2 lacks its second tile and wave 3 has no third trip
CS = 10 * 1024 + 300

CLASSES = ["nan_scale", "neg_scale", "neg_zero_scale", "zero_scale", "pos_inf", "neg_inf", "inf_cancel",
           "denormal_f32", "denormal_16", "overflow_16", "equal_cancel", "every_segment_nan", "bits_all_0",
           "bits_all_1", "bits_marker", "padding_bits_set", "garbage_header"]
NAN, INF = float("nan"), float("inf")


def tiles_of(cs: int) -> int:
    return (cs + TILE - 1) // TILE


def stride(p: int, cs: int) -> int:
    return NP.onebit_compressed_size(p, cs) // p


def positions(p: int) -> list[int]:
    """segment indices worth placing the hostile segment at: 0, 1, p - 1, and for p > 8 the
    first segment of the second round (the wide path splits segments by parity into two
    tables and by c >= 8 into rounds)"""
    ks = {0, min(1, p - 1), p - 1}
    if p > 8:
        ks.add(8)
    return sorted(ks)


def benign_scale(c: int) -> float:
    return 1e-3 * (1 + c)


def hostile_scale(cls: str, dtype: int) -> float:
    """the scale of segment k"""
    return {
        "nan_scale": NAN, "neg_scale": -1e-3, "neg_zero_scale": -0.0, "zero_scale": 0.0,
        "pos_inf": INF, "neg_inf": -INF, "inf_cancel": INF,
        "denormal_f32": 1e-40, "denormal_16": 3e-8,
        "overflow_16": 1e5 if dtype == F16 else 3.4e38,
        "every_segment_nan": NAN,
    }[cls]


def pack_bits(neg: np.ndarray) -> np.ndarray:
    """sign flags of tiles * 1024 elements -> the bit bytes (tiles * 128)"""
    t = neg.size // TILE
    b = neg.astype(np.uint8).reshape(t, 4, 64, 4).transpose(0, 2, 1, 3).reshape(t, 64, 16)
    return np.packbits(b, axis=-1, bitorder="little").reshape(-1)


def unpack_bits(bits: np.ndarray) -> np.ndarray:
    """the bit bytes of whole tiles -> one flag per element (padding included)"""
    t = bits.size // TILE_BYTES
    b = np.unpackbits(bits.reshape(t, 64, 2), axis=-1, bitorder="little")
    return b.reshape(t, 64, 4, 4).transpose(0, 2, 1, 3).reshape(-1).astype(bool)


def marker_bits(c: int, tiles: int) -> np.ndarray:
    lane, t = np.meshgrid(np.arange(64), np.arange(tiles))
    field = ((lane * 73 + t * 11 + c * 4099) & 0xffff).astype("<u2")
    return field.reshape(-1).view(np.uint8).copy()


def build_received(cs: int, segs, garbage: bool = False) -> np.ndarray:
    """p segments (scale, bit bytes) -> the receive buffer, p * stride(p, cs) bytes"""
    p = len(segs)
    co, nb = stride(p, cs), tiles_of(cs) * TILE_BYTES
    buf = np.zeros(p * co, np.uint8)
    for c, (scale, bits) in enumerate(segs):
        assert bits.size == nb and bits.dtype == np.uint8
        seg = buf[c * co:(c + 1) * co]
        seg[0:4] = np.frombuffer(np.float32(scale).tobytes(), np.uint8)
        seg[4:8] = np.frombuffer(np.uint32(0xFFFFFFFF if garbage else cs).tobytes(), np.uint8)
        if garbage:
            seg[8:32] = 0xC0 + np.arange(24) + c
        seg[32:32 + nb] = bits
    return buf


def crafted(cls: str, dtype: int, p: int, cs: int, k: int, seed: int = 0) -> np.ndarray:
    """The receive buffer of class `cls` ("benign": none) with its hostile segment at index k."""
    rng = np.random.default_rng([seed, CLASSES.index(cls) if cls in CLASSES else 99, dtype, p, k, cs])
    tiles = tiles_of(cs)
    nb = tiles * TILE_BYTES
    segs = [[benign_scale(c), rng.integers(0, 256, nb, dtype=np.uint8)] for c in range(p)]
    if cls in ("nan_scale", "neg_scale", "neg_zero_scale", "zero_scale", "pos_inf", "neg_inf", "denormal_f32",
               "denormal_16", "inf_cancel"):
        segs[k][0] = hostile_scale(cls, dtype)
        if cls == "inf_cancel" and p > 1:
            segs[(k + 1) % p][0] = -INF
    elif cls == "overflow_16":
        for c in range(p) if dtype == F32 else [k]:
            segs[c][0] = hostile_scale(cls, dtype)
    elif cls == "equal_cancel":
        for c in range(p):
            segs[c][0] = 1e-3
    elif cls == "every_segment_nan":
        for c in range(p):
            segs[c][0] = NAN
    elif cls == "bits_all_0":
        segs[k][1][:] = 0
    elif cls == "bits_all_1":
        segs[k][1][:] = 0xff
    elif cls == "bits_marker":
        for c in range(p):
            segs[c][1] = marker_bits(c, tiles)
    elif cls == "padding_bits_set":
        pad = pack_bits(np.arange(tiles * TILE) >= cs)
        for c in range(p):
            segs[c][1] |= pad
    else:
        assert cls in ("benign", "garbage_header"), cls
    return build_received(cs, segs, garbage=cls == "garbage_header")


def scales_of(recv: np.ndarray, p: int) -> np.ndarray:
    co = recv.size // p
    return np.array([recv[c * co:c * co + 4].view(np.float32)[0] for c in range(p)], np.float32)


def bits_of(recv: np.ndarray, p: int, cs: int) -> np.ndarray:
    """[p][tiles * 1024] sign flags of a receive buffer, padding included"""
    co, nb = recv.size // p, tiles_of(cs) * TILE_BYTES
    return np.stack([unpack_bits(recv[c * co + 32:c * co + 32 + nb]) for c in range(p)])


def to_f32(x: np.ndarray, dtype: int) -> np.ndarray:
    return NP.to_f32(x.view(STORAGE[dtype]), dtype)


def decode(backend, recv: np.ndarray, dtype: int, p: int, cs: int) -> np.ndarray:
    t = np.zeros(p * cs, STORAGE[dtype])
    backend.decompress_onebit(recv, p, t, dtype)
    return t


def middle_step(backend, recv: np.ndarray, dtype: int, p: int, cs: int, target: int, average):
    """The reference's middle step on a receive buffer: decompress_onebit, reduce_chunks(target),
    compress_onebit(target).  Returns the decoded tensor (p * cs), the reduced chunk (cs) and
    the re-encoded target segment (stride(p, cs) bytes)."""
    t = decode(backend, recv, dtype, p, cs)
    dec = t.copy()
    backend.reduce_chunks(t, dtype, p, target, bool(average))
    comp = backend.compress_onebit(t, dtype, p, target)
    co = comp.size // p
    assert co == stride(p, cs)
    return dec, t[target * cs:(target + 1) * cs].copy(), comp[target * co:(target + 1) * co].copy()


def ef_middle_step(backend, recv: np.ndarray, dtype: int, p: int, cs: int, target: int, average,
                   carry: np.ndarray, scale: float):
    """The server half of onebit_ef_reference.centralized_step on a receive buffer and a server
    state (carry[cs], scale): decompress, reduce, compensate, compress(target) of the
    compensated chunk as f32.  Returns the segment, the new carry and the new scale."""
    import onebit_ef_reference as REF
    t = decode(backend, recv, dtype, p, cs)
    backend.reduce_chunks(t, dtype, p, target, bool(average))
    with np.errstate(all="ignore"):
        v2 = REF.compensate(NP.to_f32(t[target * cs:(target + 1) * cs], dtype), dtype, carry,
                            np.array([scale], np.float32), cs)
    full = np.zeros(p * cs, np.float32)
    full[target * cs:(target + 1) * cs] = v2
    buf = np.zeros(recv.size, np.uint8)
    backend.compress_onebit(full, F32, p, target, out=buf)
    co = stride(p, cs)
    seg = buf[target * co:(target + 1) * co].copy()
    return seg, v2, seg[:4].view(np.float32)[0]


def segment_mismatch(got: np.ndarray, want: np.ndarray) -> str:
    """'' when two segments are equal: bit for bit, except that a NaN scale of `want` only asks
    for a NaN scale (any sign or payload: x86 and gfx950 generate different default NaNs)"""
    gs, ws = got[:4].view(np.float32)[0], want[:4].view(np.float32)[0]
    if np.isnan(ws):
        if not np.isnan(gs):
            return f"scale {gs!r}, expected NaN"
    elif not np.array_equal(got[:4], want[:4]):
        return f"scale {gs!r} ({got[:4]}), expected {ws!r} ({want[:4]})"
    bad = np.nonzero(got[4:] != want[4:])[0]
    if bad.size:
        return f"{bad.size} bytes differ, first at {bad[:5] + 4}: {got[4:][bad[:5]]} vs {want[4:][bad[:5]]}"
    return ""
