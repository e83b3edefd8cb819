"""Independent numpy statement of the MXFP4 codec's stochastic rounding (MXFP4.md,
"Stochastic rounding").

TEST INFRASTRUCTURE ONLY.  The key and the words are integer arithmetic on Python ints and
numpy uint64 / uint32; the rounding is float64, where y = |x| * 2^-e, y / step and
(q - n) * 2^16 are all exact, stated as the rule reads with no bit tricks in common with the
kernels.  Everything else of a block -- scale byte, NaN blocks, clamps, invalid elements --
is mxfp4_reference's.
"""
from __future__ import annotations

import numpy as np

import mxfp4_reference as R
from oracle import oracle_np as NP

M64 = (1 << 64) - 1
BLOCK = R.BLOCK


# -------------------------------------------------------------------- key ----
def sm64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed: int, step: int, rank: int = 0, stage: int = 0) -> int:
    return sm64(sm64(sm64(seed & M64) ^ (step & M64)) ^ (2 * rank + stage))


def fmix32(h: np.ndarray) -> np.ndarray:
    h = np.asarray(h, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def words(k: int, pair: np.ndarray) -> np.ndarray:
    """the 32-bit word of each element pair j >> 1"""
    k0, k1 = k & 0xFFFFFFFF, k >> 32
    pair = np.asarray(pair, np.uint64)
    return (fmix32((pair + np.uint64(k0)) & np.uint64(0xFFFFFFFF)) ^ np.uint64(k1)).astype(np.uint32)


def rbits(k: int, j: np.ndarray) -> np.ndarray:
    """r of the elements with index j (uint32) in the whole tensor"""
    j = np.asarray(j, np.uint64) & np.uint64(0xFFFFFFFF)
    w = words(k, j >> np.uint64(1)).astype(np.uint64)
    return np.where(j & np.uint64(1), w >> np.uint64(16), w & np.uint64(0xFFFF)).astype(np.uint32)


# ----------------------------------------------------------------- blocks ----
def floor_code_and_fraction(y: np.ndarray):
    """y in [0, 6]: (the code of the grid value at or below y, F = floor(frac * 2^16), the grid's step there)"""
    step = np.where(y < 2.0, 0.5, np.where(y < 4.0, 1.0, 2.0))
    q = y / step
    n = np.floor(q)
    F = np.floor((q - n) * 65536.0).astype(np.int64)
    lo = np.searchsorted(R.GRID, n * step, side="left")
    assert np.array_equal(R.GRID[lo], n * step)
    return lo.astype(np.int64), F, step


def encode_blocks_sr(x: np.ndarray, dtype: int, r: np.ndarray):
    """x: (nb, 32) float64 values of T, r: (nb, 32) 16-bit values -> (scale bytes, payload (nb, 16))"""
    x = np.asarray(x, np.float64).reshape(-1, BLOCK)
    r = np.asarray(r, np.int64).reshape(-1, BLOCK)
    sign = np.signbit(x)
    nan = np.isnan(x).any(axis=1)
    a = np.abs(np.where(np.isnan(x), 0.0, x))
    a = np.where(np.isinf(a), R.MAX_FINITE[dtype], a)
    e = R.shared_exponent(a.max(axis=1))
    y = np.ldexp(a, -e[:, None])
    assert (y <= 6.0).all()
    lo, F, _ = floor_code_and_fraction(y)
    code = lo + ((F + r) >> 16)
    assert (code <= 7).all()  # 6 is a grid value: rounding up never saturates
    nib = code.astype(np.uint8) | (sign.astype(np.uint8) << 3)
    payload = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    scale = (e + 127).astype(np.uint8)
    scale[nan] = R.NAN_SCALE
    payload[nan] = 0
    return scale, payload


# ------------------------------------------------------------------ codec ----
def compress_sr(t: np.ndarray, dtype: int, n_chunks: int, k: int, target: int = -1, out: np.ndarray | None = None,
                num_elem: int | None = None) -> np.ndarray:
    """mxfp4_reference.compress under key k; element `i` of chunk `c` has index c * cs + i"""
    n = t.size
    cs = n // n_chunks
    num_elem = n if num_elem is None else num_elem
    nb, sb, seg = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    buf = np.zeros(n_chunks * seg, np.uint8) if out is None else out
    x = NP.to_f32(t, dtype).astype(np.float64)
    x[num_elem:] = 0.0
    for c in (range(n_chunks) if target < 0 else [target]):
        blk = np.zeros(nb * BLOCK, np.float64)
        blk[:cs] = x[c * cs:(c + 1) * cs]
        j = np.uint64(c * cs) + np.arange(nb * BLOCK, dtype=np.uint64)
        scale, payload = encode_blocks_sr(blk, dtype, rbits(k, j))
        s = buf[c * seg:(c + 1) * seg]
        s[:] = 0
        s[:nb] = scale
        s[sb:sb + 16 * nb] = payload.ravel()
    return buf


def reduce_requantize_sr(recv: np.ndarray, n_chunks: int, cs: int, dtype: int, target: int, average: bool, k: int,
                         out: np.ndarray | None = None):
    """decode, oracle_np.reduce_chunks, compress_sr of chunk `target`"""
    t = np.zeros(n_chunks * cs, R.STORAGE[dtype])
    R.decompress(recv, n_chunks, t, dtype)
    NP.reduce_chunks(t, dtype, n_chunks, target, average)
    return compress_sr(t, dtype, n_chunks, k, target, out=out), t


def centralized_sr(inputs: list, dtype: int, average: bool, seeds, steps, num_elem: int | None = None) -> list:
    """mxfp4_reference.centralized with both encodes stochastic: rank r encodes under
    key(seeds[r], steps[r], r, 0) and re-encodes its own chunk under key(seeds[r], steps[r], r, 1)"""
    p = len(inputs)
    seeds = [seeds] * p if np.isscalar(seeds) else list(seeds)
    steps = [steps] * p if np.isscalar(steps) else list(steps)
    ts = [x.copy() for x in inputs]
    send = [compress_sr(ts[r], dtype, p, key(seeds[r], steps[r], r, 0), num_elem=num_elem) for r in range(p)]
    cnt = send[0].size // p
    recv = [np.concatenate([send[j][r * cnt:(r + 1) * cnt] for j in range(p)]) for r in range(p)]
    slots = []
    for r in range(p):
        R.decompress(recv[r], p, ts[r], dtype)
        NP.reduce_chunks(ts[r], dtype, p, r, average)
        buf = compress_sr(ts[r], dtype, p, key(seeds[r], steps[r], r, 1), r, num_elem=num_elem)
        slots.append(buf[r * cnt:(r + 1) * cnt].copy())
    gathered = np.concatenate(slots)
    for r in range(p):
        R.decompress(gathered, p, ts[r], dtype)
    return ts
