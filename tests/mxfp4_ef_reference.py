"""Reference of the MXFP4 codec's error feedback (MXFP4.md, "Error feedback"), composed
from tests/mxfp4_reference.py and the oracle.

TEST INFRASTRUCTURE ONLY.  Nothing here computes a codec step itself: the rule is two f32
array operations around `mxfp4_reference.encode_blocks` / `decode_blocks`, and the reduce of
the op is the oracle's (`backend` is oracle.oracle_c or oracle.oracle_np).

State (float32, zero before the first step): worker residual[n], server residual[cs].

  v  = x + e                       one f32 add
  vc = v if NaN else clip(v, +-M)  M the largest finite T (encode_blocks only clamps inf)
  (scale, nibbles) = encode_blocks(vc)
  d  = decode_blocks(...) as stored in T, read back as f32
  e' = vc - d, or +0 for every element of a NaN block
"""
from __future__ import annotations

import numpy as np

import mxfp4_reference as R
from oracle import oracle_np as NP

BLOCK = R.BLOCK


class WorkerState:
    def __init__(self, n: int, p: int = 1):
        self.residual = np.zeros(n, np.float32)


class OpState:
    """one rank's state of the op"""

    def __init__(self, n: int, p: int):
        self.worker = np.zeros(n, np.float32)
        self.server = np.zeros(n // p, np.float32)


def ef_blocks(x32: np.ndarray, e: np.ndarray, dtype: int):
    """x32, e: (nb, 32) float32 -> (scale (nb,), payload (nb, 16), e' (nb, 32) float32)"""
    m = np.float32(R.MAX_FINITE[dtype])
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(x32, np.float32) + np.asarray(e, np.float32)).astype(np.float32)
        vc = np.where(np.isnan(v), v, np.clip(v, -m, m)).astype(np.float32)
        scale, payload = R.encode_blocks(vc.astype(np.float64), dtype)
        d = NP.to_f32(R.decode_blocks(scale, payload, dtype).ravel(), dtype).astype(np.float32).reshape(-1, BLOCK)
        new = (vc - d).astype(np.float32)
    new[scale == R.NAN_SCALE] = 0.0
    return scale, payload, new


def encode_chunk_ef(x32: np.ndarray, residual: np.ndarray, dtype: int, seg: np.ndarray) -> None:
    """one chunk (cs f32 values, its residual updated in place) into its segment"""
    cs = x32.size
    nb, sb = R.blocks(cs), R.scale_bytes(cs)
    xb = np.zeros(nb * BLOCK, np.float32)
    eb = np.zeros(nb * BLOCK, np.float32)
    xb[:cs] = x32
    eb[:cs] = residual
    scale, payload, new = ef_blocks(xb.reshape(-1, BLOCK), eb.reshape(-1, BLOCK), dtype)
    seg[:] = 0
    seg[:nb] = scale
    seg[sb:sb + 16 * nb] = payload.ravel()
    residual[...] = new.ravel()[:cs]


def compress_ef(x: np.ndarray, dtype: int, n_chunks: int, st: WorkerState) -> np.ndarray:
    """one codec step: the compressed buffer; st.residual updated in place"""
    cs = x.size // n_chunks
    seg = R.segment_bytes(cs)
    buf = np.zeros(n_chunks * seg, np.uint8)
    x32 = NP.to_f32(x, dtype).astype(np.float32)
    for c in range(n_chunks):
        encode_chunk_ef(x32[c * cs:(c + 1) * cs], st.residual[c * cs:(c + 1) * cs], dtype, buf[c * seg:(c + 1) * seg])
    return buf


def middle_ef(backend, recv: np.ndarray, p: int, cs: int, dtype: int, target: int, average: bool,
              residual: np.ndarray) -> np.ndarray:
    """the op's middle step: decode the p received segments, the oracle's reduce_chunks into
    chunk `target`, the rule with the server residual; returns segment `target`"""
    t = np.zeros(p * cs, R.STORAGE[dtype])
    R.decompress(recv, p, t, dtype)
    backend.reduce_chunks(t, dtype, p, target, average)
    seg = np.zeros(R.segment_bytes(cs), np.uint8)
    encode_chunk_ef(NP.to_f32(t[target * cs:(target + 1) * cs], dtype).astype(np.float32), residual, dtype, seg)
    return seg


def centralized_step(backend, xs: list, dtype: int, states: list, average: bool = True):
    """one step of the op over p = len(xs) ranks: (outputs, sent buffers); states updated"""
    p = len(xs)
    n = xs[0].size
    cs = n // p
    ts = [x.copy() for x in xs]
    send = [compress_ef(ts[r], dtype, p, _Worker(states[r].worker)) for r in range(p)]
    cnt = send[0].size // p
    recv = [np.concatenate([send[j][r * cnt:(r + 1) * cnt] for j in range(p)]) for r in range(p)]
    slots = [middle_ef(backend, recv[r], p, cs, dtype, r, average, states[r].server) for r in range(p)]
    gathered = np.concatenate(slots)
    for r in range(p):
        R.decompress(gathered, p, ts[r], dtype)
    return ts, send


class _Worker:
    def __init__(self, residual):
        self.residual = residual
