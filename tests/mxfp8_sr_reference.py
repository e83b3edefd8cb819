"""Independent numpy statement of MXFP8 stochastic rounding (MXFP8.md).  TEST INFRASTRUCTURE ONLY.  Float64 and
integers, where y = |x| * 2^-e, y / step and (q - n) * 2^16 are exact; scale byte, NaN blocks, clamps and the decode
are mxfp8_reference's, the key and r are mxfp4_sr_reference's."""
import numpy as np

import mxfp8_reference as R
from mxfp4_sr_reference import key, rbits  # noqa: F401  (key: for the tests)
from oracle import oracle_np as NP


def floor_code_and_fraction(y):
    """y in [0, 448]: (n + 8 (Ey + 6), the code at or below y; F = floor(frac * 2^16); the step s = 2^(Ey - 3) there)"""
    ey = np.where(y > 0, np.maximum(np.frexp(y)[1] - 1, -6), -6).astype(np.int64)
    q = np.ldexp(y, 3 - ey)
    n = np.floor(q)
    lo = n.astype(np.int64) + 8 * (ey + 6)
    assert np.array_equal(R.GRID[lo], np.ldexp(n, ey - 3))
    return lo, np.floor((q - n) * 65536.0).astype(np.int64), np.ldexp(1.0, ey - 3)


def encode_blocks_sr(x, dtype, r):
    """x: (nb, 32) float64 values of T, r: their 16-bit draws -> (scale bytes, payload (nb, 32))"""
    x = np.asarray(x, np.float64).reshape(-1, R.BLOCK)
    nan = np.isnan(x).any(axis=1)
    e, y = R.scaled(x, dtype)
    lo, F, _ = floor_code_and_fraction(y)
    code = lo + ((F + np.asarray(r, np.int64).reshape(x.shape)) >> 16)
    assert (code <= 126).all()  # 448 is a grid value: rounding up never saturates
    payload = (code | (np.signbit(x) << 7)).astype(np.uint8)
    scale = (e + 127).astype(np.uint8)
    scale[nan], payload[nan] = R.NAN_SCALE, 0
    return scale, payload


def encode_sr(x, dtype, cs, k, j0):
    """the segment of one chunk: x its cs values (float64), element i having index j0 + i in the tensor"""
    nb = R.blocks(cs)
    blk = np.zeros(nb * R.BLOCK)
    blk[:cs] = x
    seg = np.zeros(R.segment_bytes(cs), np.uint8)
    seg[:nb], pay = encode_blocks_sr(blk, dtype, rbits(k, np.uint64(j0) + np.arange(blk.size, dtype=np.uint64)))
    seg[R.scale_bytes(cs):] = pay.ravel()
    return seg


def compress_sr(t, dtype, n_chunks, k, target=-1, out=None, num_elem=None):
    """mxfp8_reference.compress under key k; element i of chunk c has index c * cs + i"""
    cs = t.size // n_chunks
    seg = R.segment_bytes(cs)
    buf = np.zeros(n_chunks * seg, np.uint8) if out is None else out
    x = NP.to_f32(t, dtype).astype(np.float64)
    x[t.size if num_elem is None else num_elem:] = 0.0
    for c in (range(n_chunks) if target < 0 else [target]):
        buf[c * seg:(c + 1) * seg] = encode_sr(x[c * cs:(c + 1) * cs], dtype, cs, k, c * cs)
    return buf


def reduce_requantize_sr(recv, p, cs, dtype, target, average, k, out=None, num_elem=None):
    """decode, oracle_np.reduce_chunks, compress_sr of chunk `target` (into `out`, or a zero buffer)"""
    t = R.decompress(recv, p, np.zeros(p * cs, R.STORAGE[dtype]), dtype)
    NP.reduce_chunks(t, dtype, p, target, average)
    return compress_sr(t, dtype, p, k, target, out=out, num_elem=num_elem)


def centralized_sr(inputs, dtype, average, seed, step, num_elem=None):
    """mxfp8_reference.centralized with rank r encoding under key(seed, step, r, 0) and re-encoding under key(.., r, 1)"""
    p, cs = len(inputs), inputs[0].size // len(inputs)
    send = np.stack([compress_sr(x, dtype, p, key(seed, step, r, 0), num_elem=num_elem) for r, x in enumerate(inputs)])
    gathered = np.zeros_like(send[0])
    for r in range(p):  # rank r receives segment r of every rank and re-encodes the reduced chunk r
        reduce_requantize_sr(send.reshape(p, p, -1)[:, r].ravel(), p, cs, dtype, r, average, key(seed, step, r, 1),
                             out=gathered, num_elem=num_elem)
    return [R.decompress(gathered, p, x.copy(), dtype) for x in inputs]
