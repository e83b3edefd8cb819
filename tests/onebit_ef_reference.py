"""Reference of the 1-bit codec's error feedback, composed from the oracle.

TEST INFRASTRUCTURE ONLY.  Nothing here computes a codec step itself: the
compensation is three f32 array operations and every compress, decompress and
reduce is the oracle's (`backend` is oracle.oracle_c or oracle.oracle_np, same
function names), in the op order of oracle/simulate.py.

State (all float32, zero before the first step):
  worker: carry[n], scales[p]        server: carry[cs], scale[1]
The carry holds the previous step's compensated values; the residual is rebuilt
from it and the previous scale:

  d = stored(carry < 0 ? -s : +s, T)      what the receiver decoded last step
  v = x + (carry - d)                     compensated value; carry = v
  segment = compress_onebit(v as F32)     whatever T is
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np as NP

F32 = 0


def stored(v: np.ndarray, dt: int) -> np.ndarray:
    """v as it reads back after a store to dtype dt"""
    return NP.to_f32(NP.from_f32(np.asarray(v, np.float32), dt), dt).astype(np.float32)


def compensate(x32: np.ndarray, dt: int, carry: np.ndarray, scales: np.ndarray, cs: int) -> np.ndarray:
    s = np.repeat(np.asarray(scales, np.float32), cs)
    d = stored(np.where(carry < 0, -s, s).astype(np.float32), dt)
    r = (carry - d).astype(np.float32)
    return (x32 + r).astype(np.float32)


def header_scales(buf: np.ndarray, p: int) -> np.ndarray:
    co = buf.size // p
    return np.array([np.frombuffer(buf[c * co:c * co + 4].tobytes(), np.float32)[0] for c in range(p)], np.float32)


class WorkerState:
    def __init__(self, n: int, p: int):
        self.carry = np.zeros(n, np.float32)
        self.scales = np.zeros(p, np.float32)


class OpState:
    """one rank's state of the op"""

    def __init__(self, n: int, p: int):
        self.wc = np.zeros(n, np.float32)
        self.ws = np.zeros(p, np.float32)
        self.sc = np.zeros(n // p, np.float32)
        self.ss = np.zeros(1, np.float32)


def compress_ef(backend, x: np.ndarray, dt: int, n_chunks: int, st: WorkerState) -> np.ndarray:
    """one codec step: the compressed buffer; st updated in place"""
    cs = x.size // n_chunks
    v = compensate(NP.to_f32(x, dt), dt, st.carry, st.scales, cs)
    st.carry[...] = v
    buf = backend.compress_onebit(v, F32, n_chunks)
    st.scales[...] = header_scales(buf, n_chunks)
    return buf


def centralized_step(backend, xs: list, dt: int, states: list, average: bool = True):
    """one step of the op over p = len(xs) ranks: (outputs, sent buffers); states updated"""
    p = len(xs)
    n = xs[0].size
    cs = n // p
    ts = [x.copy() for x in xs]
    send = []
    for r in range(p):
        st = states[r]
        v = compensate(NP.to_f32(ts[r], dt), dt, st.wc, st.ws, cs)
        st.wc[...] = v
        buf = backend.compress_onebit(v, F32, p)
        st.ws[...] = header_scales(buf, p)
        send.append(buf)
    S = send[0].size
    cnt = S // p
    recv = [np.concatenate([send[j][r * cnt:(r + 1) * cnt] for j in range(p)]) for r in range(p)]
    slots = []
    for r in range(p):
        st = states[r]
        backend.decompress_onebit(recv[r], p, ts[r], dt)
        backend.reduce_chunks(ts[r], dt, p, r, average)
        v2 = compensate(NP.to_f32(ts[r][r * cs:(r + 1) * cs], dt), dt, st.sc, st.ss, cs)
        st.sc[...] = v2
        full = np.zeros(n, np.float32)
        full[r * cs:(r + 1) * cs] = v2
        buf = np.zeros(S, np.uint8)
        backend.compress_onebit(full, F32, p, r, out=buf)
        slot = buf[r * cnt:(r + 1) * cnt].copy()
        st.ss[0] = np.frombuffer(slot[:4].tobytes(), np.float32)[0]
        slots.append(slot)
    gathered = np.concatenate(slots)
    for r in range(p):
        backend.decompress_onebit(gathered, p, ts[r], dt)
    return ts, send


def appendix_inputs(p: int, cs: int, dt: int) -> list:
    """the issue's inputs: rank r's gradient standard_normal(n) * 1e-3 + 0.0005 * r from
    default_rng(p), rounded to the dtype"""
    rng = np.random.default_rng(p)
    n = p * cs
    return [NP.from_f32((rng.standard_normal(n) * 1e-3 + 0.0005 * r).astype(np.float32), dt) for r in range(p)]
