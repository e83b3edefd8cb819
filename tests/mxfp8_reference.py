"""Independent numpy statement of the MXFP8 (E4M3) codec (MXFP8.md).

TEST INFRASTRUCTURE ONLY.  Float64 throughout: every T value, every power of two
(`np.ldexp`) and every product of the two is exact in float64, so the rules are stated
as they read -- a shared exponent from `np.frexp`, the nearest of the 127 E4M3 magnitudes
by distance, ties to the even code -- with no bit tricks in common with the kernels.  The
chunk reduce and the elementwise steps of the composed ops are oracle_np's.

Arrays follow oracle_np: F32 float32, F16 float16, BF16 uint16 bit patterns.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np as NP

F32, F16, BF16 = 0, 1, 2
BLOCK = 32
GRANULE = 128
NAN_SCALE = 0xFF
NAN_CODE = 0x7F
MAX_FINITE = {F32: float(np.finfo(np.float32).max), F16: 65504.0,
              BF16: float(np.uint32(0x7F7F0000).view(np.float32))}
NAN_BITS = {F32: np.uint32(0x7FC00000), F16: np.uint16(0x7E00), BF16: np.uint16(0x7FC0)}
STORAGE = {F32: np.float32, F16: np.float16, BF16: np.uint16}
TAPERED = 0x10000


def code_value(code: int) -> float:
    """the magnitude of element byte `code` & 0x7F (below 0x7F)"""
    e, m = (code >> 3) & 15, code & 7
    return m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)


# the 127 magnitudes 0 .. 448, ascending with their codes
GRID = np.array([code_value(c) for c in range(127)])


# ------------------------------------------------------------------ sizes ----
def align32(v: int) -> int:
    return (v + 31) // 32 * 32


def blocks(cs: int) -> int:
    return (cs + BLOCK - 1) // BLOCK


def scale_bytes(cs: int) -> int:
    return align32(blocks(cs))


def payload_bytes(cs: int) -> int:
    return 32 * blocks(cs)


def segment_bytes(cs: int) -> int:
    return scale_bytes(cs) + payload_bytes(cs)


def compressed_bytes(cs: int, n_chunks: int) -> int:
    return n_chunks * segment_bytes(cs)


def piece_range(cs: int, pieces: int, piece: int):
    """blocks [begin, end) of piece `piece`: equal parts, or tapered (edge weights 0, 1, 3, ...,
    2(k - 1)) from three pieces on; edges rounded up to the granule of 128 blocks"""
    count, nb = pieces & 0xFFFF, blocks(cs)

    def clip(b):
        return min((b + GRANULE - 1) // GRANULE * GRANULE, nb)

    if count >= 3 and pieces & TAPERED:
        w = 2 * (count - 1)
        edges = [0]
        for j in range(1, count + 1):
            edges.append(nb if j >= count else clip(max(-(-nb * (2 * j - 1) // w), edges[-1] + GRANULE)))
        return edges[piece], edges[piece + 1]
    length = clip(-(-nb // count))
    return min(piece * length, nb), min((piece + 1) * length, nb)


# ----------------------------------------------------------------- blocks ----
def shared_exponent(amax: np.ndarray) -> np.ndarray:
    """e per block: amax = m * 2^k, m in [0.5, 1): k - 9 if m <= 0.875 else k - 8, at least -127"""
    m, k = np.frexp(amax)
    e = np.where(m <= 0.875, k - 9, k - 8)
    e = np.maximum(e, -127)
    return np.where(amax == 0, -127, e).astype(np.int64)


def nearest_code(y: np.ndarray) -> np.ndarray:
    """index of the E4M3 magnitude nearest to y (0 <= y <= 448), ties to the even code"""
    lo = np.clip(np.searchsorted(GRID, y, side="right") - 1, 0, 126)
    hi = np.minimum(lo + 1, 126)
    dlo, dhi = y - GRID[lo], GRID[hi] - y
    even = np.where(lo % 2 == 0, lo, hi)
    return np.where((hi == lo) | (dlo < dhi), lo, np.where(dhi < dlo, hi, even)).astype(np.uint8)


def scaled(x: np.ndarray, dtype: int):
    """(e per block, |x| * 2^-e) of (nb, 32) float64 values of T; NaN counts as 0, inf as the largest finite T"""
    a = np.abs(np.where(np.isnan(x), 0.0, x))
    a = np.where(np.isinf(a), MAX_FINITE[dtype], a)
    e = shared_exponent(a.max(axis=1))
    return e, np.ldexp(a, -e[:, None])


def encode_blocks(x: np.ndarray, dtype: int):
    """x: (nb, 32) float64 values of T (NaN, inf allowed) -> (scale bytes (nb,), payload (nb, 32))"""
    x = np.asarray(x, np.float64).reshape(-1, BLOCK)
    sign = np.signbit(x)
    nan = np.isnan(x).any(axis=1)
    e, y = scaled(x, dtype)
    assert (y <= 448.0).all()
    payload = (nearest_code(y) | (sign.astype(np.uint8) << 7)).astype(np.uint8)
    scale = (e + 127).astype(np.uint8)
    scale[nan] = NAN_SCALE
    payload[nan] = 0
    return scale, payload


def decode_blocks(scale: np.ndarray, payload: np.ndarray, dtype: int) -> np.ndarray:
    """(nb,) scale bytes, (nb, 32) payload -> (nb, 32) values as stored in T (STORAGE[dtype])"""
    scale = np.asarray(scale, np.uint8)
    payload = np.asarray(payload, np.uint8).reshape(-1, BLOCK)
    code = payload & 0x7F
    mag = GRID[np.minimum(code, 126)] * np.ldexp(1.0, scale.astype(np.int64) - 127)[:, None]
    mag = np.minimum(mag, MAX_FINITE[dtype])
    v = np.copysign(mag, np.where(payload & 0x80, -1.0, 1.0))
    out = NP.from_f32(v.astype(np.float32).ravel(), dtype).reshape(-1, BLOCK)  # the f32 step is exact
    bits = out.view(np.uint32 if dtype == F32 else np.uint16)
    bits[(code == NAN_CODE) | (scale == NAN_SCALE)[:, None]] = NAN_BITS[dtype]
    return out


# ------------------------------------------------------------------ codec ----
def compress(t: np.ndarray, dtype: int, n_chunks: int, target: int = -1, out: np.ndarray | None = None,
             num_elem: int | None = None) -> np.ndarray:
    """The compressed buffer of tensor t (allocated size t.size, num_elem valid elements).
    target >= 0: only that chunk's segment is written (into `out`, or a zero buffer)."""
    n = t.size
    cs = n // n_chunks
    num_elem = n if num_elem is None else num_elem
    nb, sb, seg = blocks(cs), scale_bytes(cs), segment_bytes(cs)
    buf = np.zeros(n_chunks * seg, np.uint8) if out is None else out
    x = NP.to_f32(t, dtype).astype(np.float64)
    x[num_elem:] = 0.0  # invalid elements count as +0
    for c in (range(n_chunks) if target < 0 else [target]):
        blk = np.zeros(nb * BLOCK, np.float64)
        blk[:cs] = x[c * cs:(c + 1) * cs]
        scale, payload = encode_blocks(blk, dtype)
        s = buf[c * seg:(c + 1) * seg]
        s[:] = 0
        s[:nb] = scale
        s[sb:sb + 32 * nb] = payload.ravel()
    return buf


def decompress(buf: np.ndarray, n_chunks: int, t: np.ndarray, dtype: int) -> np.ndarray:
    """Decodes into t (every element of every chunk), returns t."""
    cs = t.size // n_chunks
    nb, sb, seg = blocks(cs), scale_bytes(cs), segment_bytes(cs)
    for c in range(n_chunks):
        s = buf[c * seg:(c + 1) * seg]
        v = decode_blocks(s[:nb], s[sb:sb + 32 * nb], dtype).ravel()[:cs]
        t[c * cs:(c + 1) * cs] = v
    return t


def reduce_requantize(recv: np.ndarray, n_chunks: int, cs: int, dtype: int, target: int, average: bool,
                      out: np.ndarray | None = None):
    """The centralized op's middle step, composed: decode, oracle_np.reduce_chunks, encode of
    chunk `target`.  Returns (buffer with segment `target` written, tensor with chunk `target` reduced)."""
    t = np.zeros(n_chunks * cs, STORAGE[dtype])
    decompress(recv, n_chunks, t, dtype)
    NP.reduce_chunks(t, dtype, n_chunks, target, average)
    buf = compress(t, dtype, n_chunks, target, out=out)
    return buf, t


# -------------------------------------------------------------------- ops ----
def centralized(inputs: list, dtype: int, average: bool = True, num_elem: int | None = None) -> list:
    """centralized_low_precision_synchronous.rs:30-71 with this codec (op order of oracle/simulate.py)"""
    p = len(inputs)
    ts = [x.copy() for x in inputs]
    send = [compress(t, dtype, p, -1, num_elem=num_elem) for t in ts]
    S = send[0].size
    assert S % p == 0
    cnt = S // p
    recv = [np.concatenate([send[j][r * cnt:(r + 1) * cnt] for j in range(p)]) for r in range(p)]
    slots = []
    for r in range(p):
        decompress(recv[r], p, ts[r], dtype)
        NP.reduce_chunks(ts[r], dtype, p, r, average)
        buf = compress(ts[r], dtype, p, r, num_elem=num_elem)
        slots.append(buf[r * cnt:(r + 1) * cnt].copy())
    gathered = np.concatenate(slots)
    for r in range(p):
        decompress(gathered, p, ts[r], dtype)
    return ts


def decentralized(ts: list, weights: list, lefts: list, rights: list, dtype: int):
    """decentralized_low_precision_synchronous.rs:42-152 with this codec; returns the updated
    (t, weight, left, right) lists"""
    p = len(ts)
    ts, weights = [t.copy() for t in ts], [w.copy() for w in weights]
    lefts, rights = [x.copy() for x in lefts], [x.copy() for x in rights]
    f13, f53 = float(np.float32(1.0 / 3.0)), float(np.float32(-5.0 / 3.0))
    comps = []
    for r in range(p):
        NP.addmul_inplace(ts[r], lefts[r], dtype, f13)
        NP.addmul_inplace(ts[r], rights[r], dtype, f13)
        NP.addmul_inplace(ts[r], weights[r], dtype, f53)
        comps.append(compress(ts[r], dtype, 1, -1))
    for r in range(p):
        lpeer, rpeer = (r + p - 1) % p, (r + 1) % p
        decompress(comps[lpeer], 1, ts[r], dtype)
        NP.add_inplace(lefts[r], ts[r], dtype)
        decompress(comps[rpeer], 1, ts[r], dtype)
        NP.add_inplace(rights[r], ts[r], dtype)
        decompress(comps[r], 1, ts[r], dtype)
        NP.add_inplace(ts[r], weights[r], dtype)
        weights[r][...] = ts[r]
    return ts, weights, lefts, rights
