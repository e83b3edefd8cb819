"""Independent numpy statement of the MXFP6 (E2M3) codec (MXFP6.md).

TEST INFRASTRUCTURE ONLY.  Float64 throughout, as mxfp8_reference.py: a shared exponent from
`np.frexp`, the nearest of the 32 E2M3 magnitudes by distance, ties to the even code, and
the six-bit packing by `np.packbits` -- no bit trick and no word assembly in common with the
kernels.  The middle step and the composed ops are mxfp8_reference's, which take this
module's compress and decompress in place of their own (tests/test_gpu_mxfp6.py).

Arrays follow oracle_np: F32 float32, F16 float16, BF16 uint16 bit patterns.
"""
from __future__ import annotations

import numpy as np

from mxfp8_reference import (BF16, BLOCK, F16, F32, MAX_FINITE, NAN_BITS, NAN_SCALE, STORAGE, blocks,  # noqa: F401
                             piece_range, scale_bytes)
from oracle import oracle_np as NP

BLOCK_BYTES = 24


def code_value(code: int) -> float:
    """the magnitude of code & 0x1F"""
    e, m = (code >> 3) & 3, code & 7
    return m * 2.0 ** -3 if e == 0 else (8 + m) * 2.0 ** (e - 4)


GRID = np.array([code_value(c) for c in range(32)])   # 0 .. 7.5, ascending with their codes


def payload_bytes(cs: int) -> int:
    return (BLOCK_BYTES * blocks(cs) + 31) // 32 * 32


def segment_bytes(cs: int) -> int:
    return scale_bytes(cs) + payload_bytes(cs)


def compressed_bytes(cs: int, n_chunks: int) -> int:
    return n_chunks * segment_bytes(cs)


def shared_exponent(amax: np.ndarray) -> np.ndarray:
    """e per block: amax = m * 2^k, m in [0.5, 1): k - 3 if m <= 0.9375 else k - 2, at least -127"""
    m, k = np.frexp(amax)
    e = np.maximum(np.where(m <= 0.9375, k - 3, k - 2), -127)
    return np.where(amax == 0, -127, e).astype(np.int64)


def nearest_code(y: np.ndarray) -> np.ndarray:
    """index of the E2M3 magnitude nearest to y (0 <= y <= 7.5), ties to the even code"""
    lo = np.clip(np.searchsorted(GRID, y, side="right") - 1, 0, 31)
    hi = np.minimum(lo + 1, 31)
    dlo, dhi = y - GRID[lo], GRID[hi] - y
    even = np.where(lo % 2 == 0, lo, hi)
    return np.where((hi == lo) | (dlo < dhi), lo, np.where(dhi < dlo, hi, even)).astype(np.uint8)


def encode_blocks(x: np.ndarray, dtype: int):
    """x: (nb, 32) float64 values of T (NaN, inf allowed) -> (scale bytes (nb,), codes (nb, 32))"""
    x = np.asarray(x, np.float64).reshape(-1, BLOCK)
    nan = np.isnan(x).any(axis=1)
    a = np.abs(np.where(np.isnan(x), 0.0, x))
    a = np.where(np.isinf(a), MAX_FINITE[dtype], a)
    e = shared_exponent(a.max(axis=1))
    y = np.ldexp(a, -e[:, None])
    assert (y <= 7.5).all()
    codes = (nearest_code(y) | (np.signbit(x).astype(np.uint8) << 5)).astype(np.uint8)
    scale = (e + 127).astype(np.uint8)
    scale[nan] = NAN_SCALE
    codes[nan] = 0
    return scale, codes


def pack(codes: np.ndarray) -> np.ndarray:
    """(nb, 32) codes -> (nb, 24) bytes: element j in bits [6j, 6j + 6) of the little-endian 192"""
    bits = np.unpackbits(np.asarray(codes, np.uint8).reshape(-1, BLOCK, 1), axis=2, bitorder="little")[:, :, :6]
    return np.packbits(bits.reshape(-1, 192), axis=1, bitorder="little")


def unpack(payload: np.ndarray) -> np.ndarray:
    bits = np.unpackbits(np.asarray(payload, np.uint8).reshape(-1, BLOCK_BYTES), axis=1, bitorder="little")
    return np.packbits(bits.reshape(-1, BLOCK, 6), axis=2, bitorder="little").reshape(-1, BLOCK)


def decode_blocks(scale: np.ndarray, codes: np.ndarray, dtype: int) -> np.ndarray:
    """(nb,) scale bytes, (nb, 32) codes -> (nb, 32) values as stored in T (STORAGE[dtype])"""
    scale = np.asarray(scale, np.uint8)
    codes = np.asarray(codes, np.uint8).reshape(-1, BLOCK)
    mag = GRID[codes & 0x1F] * np.ldexp(1.0, scale.astype(np.int64) - 127)[:, None]
    v = np.copysign(np.minimum(mag, MAX_FINITE[dtype]), np.where(codes & 0x20, -1.0, 1.0))
    out = NP.from_f32(v.astype(np.float32).ravel(), dtype).reshape(-1, BLOCK)  # the f32 step is exact
    out.view(np.uint32 if dtype == F32 else np.uint16)[scale == NAN_SCALE] = NAN_BITS[dtype]
    return out


def compress(t: np.ndarray, dtype: int, n_chunks: int, target: int = -1, out: np.ndarray | None = None,
             num_elem: int | None = None) -> np.ndarray:
    """The compressed buffer of tensor t (allocated size t.size, num_elem valid elements).
    target >= 0: only that chunk's segment is written (into `out`, or a zero buffer)."""
    cs = t.size // n_chunks
    nb, sb, seg = blocks(cs), scale_bytes(cs), segment_bytes(cs)
    buf = np.zeros(n_chunks * seg, np.uint8) if out is None else out
    x = NP.to_f32(t, dtype).astype(np.float64)
    x[t.size if num_elem is None else num_elem:] = 0.0  # invalid elements count as +0
    for c in (range(n_chunks) if target < 0 else [target]):
        scale, codes = encode_blocks(np.pad(x[c * cs:(c + 1) * cs], (0, nb * BLOCK - cs)), dtype)
        s = buf[c * seg:(c + 1) * seg]
        s[:] = 0
        s[:nb] = scale
        s[sb:sb + BLOCK_BYTES * nb] = pack(codes).ravel()
    return buf


def decompress(buf: np.ndarray, n_chunks: int, t: np.ndarray, dtype: int) -> np.ndarray:
    """Decodes into t (every element of every chunk), returns t."""
    cs = t.size // n_chunks
    nb, sb, seg = blocks(cs), scale_bytes(cs), segment_bytes(cs)
    for c in range(n_chunks):
        s = buf[c * seg:(c + 1) * seg]
        t[c * cs:(c + 1) * cs] = decode_blocks(s[:nb], unpack(s[sb:sb + BLOCK_BYTES * nb]), dtype).ravel()[:cs]
    return t
