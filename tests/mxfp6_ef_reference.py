"""Reference of the MXFP6 codec's error feedback (MXFP6.md, "Error feedback"), composed from
tests/mxfp6_reference.py and the oracle.  TEST INFRASTRUCTURE ONLY.  State (float32, zero before
the first step): worker residual[n], server residual[cs]; the state classes are
mxfp8_ef_reference's.  Its functions are bound to the 8-bit codec's layout (a byte per element),
so the four below restate them over the six-bit packing.

  v = x + e;  vc = v if NaN else clip(v, +-M);  (scale, codes) = encode_blocks(vc)
  d = decode_blocks(...) as stored in T, read back as f32;  e' = vc - d, +0 in a NaN block
"""
import numpy as np

import mxfp6_reference as R
from mxfp8_ef_reference import OpState, WorkerState  # noqa: F401
from oracle import oracle_np as NP


def ef_blocks(x32, e, dtype):
    """x32, e: (nb, 32) float32 -> (scale (nb,), payload (nb, 24), e' (nb, 32) float32)"""
    m = np.float32(R.MAX_FINITE[dtype])
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(x32, np.float32) + np.asarray(e, np.float32)).astype(np.float32)
        vc = np.where(np.isnan(v), v, np.clip(v, -m, m)).astype(np.float32)
        scale, codes = R.encode_blocks(vc.astype(np.float64), dtype)
        d = NP.to_f32(R.decode_blocks(scale, codes, dtype).ravel(), dtype).astype(np.float32).reshape(-1, 32)
        new = (vc - d).astype(np.float32)
    new[scale == R.NAN_SCALE] = 0.0
    return scale, R.pack(codes), new


def encode_chunk_ef(x32, residual, dtype, seg):
    cs = x32.size
    nb, sb = R.blocks(cs), R.scale_bytes(cs)
    xe = np.zeros((2, nb * 32), np.float32)
    xe[0, :cs], xe[1, :cs] = x32, residual
    seg[:] = 0
    seg[:nb], payload, new = ef_blocks(xe[0].reshape(-1, 32), xe[1].reshape(-1, 32), dtype)
    seg[sb:sb + R.BLOCK_BYTES * nb] = payload.ravel()
    residual[...] = new.ravel()[:cs]


def compress_ef(x, dtype, n_chunks, st):
    """one codec step: the compressed buffer; st.residual (or the array st) updated in place"""
    res, cs = getattr(st, "residual", st), x.size // n_chunks
    seg = R.segment_bytes(cs)
    buf = np.zeros(n_chunks * seg, np.uint8)
    x32 = NP.to_f32(x, dtype).astype(np.float32)
    for c in range(n_chunks):
        encode_chunk_ef(x32[c * cs:(c + 1) * cs], res[c * cs:(c + 1) * cs], dtype, buf[c * seg:(c + 1) * seg])
    return buf


def middle_ef(backend, recv, p, cs, dtype, target, average, residual):
    """decode the p received segments, the oracle's reduce_chunks, the rule with the server residual: segment `target`"""
    t = np.zeros(p * cs, R.STORAGE[dtype])
    R.decompress(recv, p, t, dtype)
    backend.reduce_chunks(t, dtype, p, target, average)
    seg = np.zeros(R.segment_bytes(cs), np.uint8)
    encode_chunk_ef(NP.to_f32(t[target * cs:(target + 1) * cs], dtype).astype(np.float32), residual, dtype, seg)
    return seg


def centralized_step(backend, xs, dtype, states, average=True):
    """one step of the op over p = len(xs) ranks: (outputs, sent buffers); states updated"""
    p, cs = len(xs), xs[0].size // len(xs)
    ts = [x.copy() for x in xs]
    send = [compress_ef(ts[r], dtype, p, states[r].worker) for r in range(p)]
    cnt = send[0].size // p
    recv = [np.concatenate([s[r * cnt:(r + 1) * cnt] for s in send]) for r in range(p)]
    got = np.concatenate([middle_ef(backend, recv[r], p, cs, dtype, r, average, states[r].server) for r in range(p)])
    return [R.decompress(got, p, t, dtype) for t in ts], send
