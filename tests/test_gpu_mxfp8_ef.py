"""GPU tests of the MXFP8 codec's error feedback (MXFP8.md, "Error feedback"): the two HIP
kernels, the comm op on the loopback transport and the bucket path, byte for byte (payload)
and bit for bit (residuals, results) against the composition in tests/mxfp8_ef_reference.py
after every step, with the hardware conversions and with the arithmetic (BAGUA_MXFP8_HWCVT)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import mxfp8_ef_reference as REF
import mxfp8_reference as R
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_mxfp8 import bc, dev_at, grads, hostile_inputs, received, same_bytes, u8
from test_gpu_op_edges import KernelNames

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
TILE = 2048  # elements of the worker step's wave tile: 8 rows of 256 f32, 4 rows of 512 f16 / bf16


@pytest.fixture(autouse=True, params=["1", "0"], ids=["hw", "arith"])
def conversion(request, monkeypatch):
    monkeypatch.setenv("BAGUA_MXFP8_HWCVT", request.param)
    for k in ("BAGUA_MX_EF_RESIDUAL_NT", "BAGUA_TUNE_MX8_ENCODE_BLOCKS", "BAGUA_TUNE_MX8_MIDDLE_BLOCKS"):
        monkeypatch.delenv(k, raising=False)


def step_grads(rng, n, dtype, r=0):
    """block-wise magnitudes plus a per-rank offset; no -0 (x + (+0) is +0, so only then is step 0 the plain codec's)"""
    x = NP.to_f32(grads(rng, n, dtype), dtype) + np.float32(0.0005 * r)
    x = NP.to_f32(NP.from_f32(x.astype(np.float32), dtype), dtype)
    x[x == 0] = 0.0
    return NP.from_f32(x.astype(np.float32), dtype)


# ------------------------------------------------------------------ codec ----
# one element, the block edge, one wave tile and its edge, chunks that start off 16 B with a ragged
# tail, several workgroups, one workgroup walking the grid-stride loop, a gradient view one element
# into its allocation (guarded loads, vector residual)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_chunks,cs,offset,blocks", [
    (1, 1, 0, None), (1, 31, 0, None), (1, 32, 0, None), (1, 33, 0, None), (1, TILE, 0, None), (1, TILE + 1, 0, None),
    (3, 4100, 0, None), (8, 20000, 0, None), (8, 20000, 0, "1"), (2, 4096, 1, None)])
def test_codec_steps_match_reference(bc, dtype, n_chunks, cs, offset, blocks, monkeypatch):
    if blocks:
        monkeypatch.setenv("BAGUA_TUNE_MX8_ENCODE_BLOCKS", blocks)
    n = n_chunks * cs
    rng = np.random.default_rng(1000 * dtype + n)
    state = bc.MXFP8ErrorFeedbackState(n, n_chunks, 0)
    ref = REF.WorkerState(n)
    for step in range(4):
        x = step_grads(rng, n, dtype)
        xt = dev_at(x, dtype, offset)
        assert (xt.data_ptr() % 16 != 0) == bool(offset)
        t = bc.BaguaTensorPy(xt, "g")
        got = t.compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        same_bytes(got, REF.compress_ef(x, dtype, n_chunks, ref), f"step {step}: payload")
        if step == 0:  # zero state (and no -0 in the input): the plain codec's bytes
            same_bytes(got, t.compress("MXFP8", n_chunks, -1).to_numpy_u8(), "step 0 against the plain codec")
        same_bytes(host(state.worker_residual, F32), ref.residual, f"step {step}: residual")
        same_bytes(host(xt, dtype), x, "the gradient is read only")
    assert ref.residual.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_chunk_with_a_residual_only_4_byte_aligned(bc, dtype):
    """bagua_mxfp8_compress_ef on one chunk with residual + cs, cs = 4097 (the composed middle step's call)"""
    cs = 4097
    rng = np.random.default_rng(55 + dtype)
    res = torch.zeros(2 * cs, dtype=torch.float32, device="cuda")
    assert (res.data_ptr() + 4 * cs) % 16 == 4
    ref = REF.WorkerState(cs)
    S = R.compressed_bytes(cs, 1)
    for step in range(3):
        x = step_grads(rng, cs, dtype)
        out = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
        assert bc._native.K.bagua_mxfp8_compress_ef(dtype, dev(x, dtype).data_ptr(), cs, cs, 1, out.data_ptr(), S, -1,
                                                    res.data_ptr() + 4 * cs, None) == OK
        same_bytes(u8(out), REF.compress_ef(x, dtype, 1, ref), f"step {step}: payload")
        same_bytes(host(res, F32)[cs:], ref.residual, f"step {step}: residual")
        assert not host(res, F32)[:cs].any(), "the residual before the chunk's is untouched"


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_inputs(bc, dtype):
    """step 0 ordinary gradients, step 1 the hostile tensor, step 2 ordinary again: a NaN block
    resets its residuals to +0, +-inf and the largest finite T clamp, -0 is encoded as +0"""
    cases, p = hostile_inputs(dtype)
    rng = np.random.default_rng(3 + dtype)
    for name, bad in cases.items():
        n = bad.size
        cs = n // p
        nb, seg = R.blocks(cs), R.segment_bytes(cs)
        state = bc.MXFP8ErrorFeedbackState(n, p, 0)
        ref = REF.WorkerState(n)
        for step, x in enumerate([step_grads(rng, n, dtype), bad, step_grads(rng, n, dtype)]):
            got = bc.BaguaTensorPy(dev(x, dtype), "g").compress_with_error_feedback(p, state).to_numpy_u8()
            same_bytes(got, REF.compress_ef(x, dtype, p, ref), f"{name}, step {step}: payload")
            res = host(state.worker_residual, F32)
            same_bytes(res, ref.residual, f"{name}, step {step}: residual")
            assert np.isfinite(res).all(), f"{name}, step {step}: the state must stay finite"
            scales = np.concatenate([got[c * seg:c * seg + nb] for c in range(p)])
            if step == 1 and name.startswith("nan"):  # one NaN block per chunk, its residuals +0 bits
                j = int(np.nonzero(np.isnan(NP.to_f32(bad, dtype)))[0][0])
                assert (scales == 0xFF).sum() == p and not res[j - j % 32:j - j % 32 + 8].view(np.uint32).any(), name
            assert step != 2 or 0xFF not in scales
        if name == "minus zero only":  # a fresh state: -0 + (+0) = +0, no sign bit in any byte
            fresh = bc.MXFP8ErrorFeedbackState(n, p, 0)
            assert not bc.BaguaTensorPy(dev(bad, dtype), "g").compress_with_error_feedback(p, fresh).to_numpy_u8().any()


# ------------------------------------------------------------ middle step ----
# p = 2, 5, 16: one per BY (2, 4, 8), 5 with a partly filled second round of the tree
@pytest.mark.parametrize("average", [1, 0])
@pytest.mark.parametrize("p", [2, 5, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step(bc, dtype, p, average):
    """four steps against middle_ef; steps 1 and 3 take the plain middle step's hostile segments:
    a NaN block in segment 0 (its residuals reset) and, on f16, a sum that leaves the range (clamped)"""
    for cs in (33, 4097):
        rng = np.random.default_rng(100 * dtype + 7 * p + cs)
        target, seg = p // 2, R.segment_bytes(cs)
        res = torch.zeros(cs + 1, dtype=torch.float32, device="cuda")[1 if cs == 33 else 0:][:cs]  # 33: 4-B aligned only
        ref = np.zeros(cs, np.float32)
        for step in range(4):
            recv = received(rng, p, cs, dtype) if step % 2 else R.compress(step_grads(rng, p * cs, dtype), dtype, p)
            S = recv.size
            rt = torch.from_numpy(recv).cuda()
            out = torch.full((S,), 0xCD, dtype=torch.uint8, device="cuda")
            what = f"p={p} cs={cs} average={average} step {step}"
            assert bc._native.K.bagua_mxfp8_reduce_requantize_ef(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(),
                                                                 S, target, res.data_ptr(), None) == OK, what
            want = np.full(S, 0xCD, np.uint8)
            want[target * seg:(target + 1) * seg] = REF.middle_ef(NP, recv, p, cs, dtype, target, bool(average), ref)
            same_bytes(u8(out), want, what)
            same_bytes(host(res, F32), ref, what + ": residual")
            assert np.isfinite(ref).all() and (step or ref.any())
            if step % 2:  # received() plants its NaN at element 37 of the p * cs
                b = 37 % cs // 32
                assert want[target * seg + b] == 0xFF and not ref[32 * b:32 * b + 32].view(np.uint32).any()


# ------------------------------------------------- the op on the loopback transport ----
def _raws(st):
    return [st._raw(t) for t in st.tensors()]


@pytest.mark.parametrize("p,dtype,cs,misalign_rank", [(1, F32, 15007, None), (2, BF16, 20000, 1), (4, F16, 8192, None)])
def test_op_matches_reference(bc, p, dtype, cs, misalign_rank):
    """three steps against centralized_step; a misaligned tensor on one rank; at one rank the op
    runs as a bucket op through BaguaCommBackendPy, otherwise through the C entry"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    n = p * cs
    rng = np.random.default_rng(p * 1000 + dtype * 10 + cs)
    comms = loopback_communicators(p, 0)
    states = [bc.MXFP8ErrorFeedbackState(n, p, 0) for _ in range(p)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    names = KernelNames(N, comms[0])
    if p == 1:
        bt = bc.BaguaTensorPy(torch.zeros(n, device="cuda"), "g")
        bk = bc.BaguaBucketPy("mxfp8_ef_bucket", [bt])
        bk.append_centralized_synchronous_op(comms[0], None, average=True, compression="MXFP8", error_feedback=states[0])
        assert type(bk.ops()[0]).__name__ == "CentralizedMXFP8ErrorFeedback" and "MXFP8ErrorFeedbackState" in repr(states[0])
        backend = bc.BaguaCommBackendPy(4, 0)
        backend.register_ordered_buckets([bk])
    for step in range(3):
        xs = [step_grads(rng, n, dtype, r) for r in range(p)]
        want, _ = REF.centralized_step(NP, xs, dtype, refs, True)
        ts = [dev_at(x, dtype, 1 if r == misalign_rank else 0) for r, x in enumerate(xs)]
        torch.cuda.synchronize()

        def rank(r):
            raw, sr = bc.BaguaTensorPy(ts[r], f"g{r}").raw(), _raws(states[r])
            with names if r == 0 and step == 0 else contextlib.nullcontext():  # rank 0's first step: its kernels' names
                N.check(N.C.bagua_centralized_mxfp8_error_feedback(comms[r].handle, ctypes.byref(raw), 1,
                                                                   ctypes.byref(sr[0]), ctypes.byref(sr[1])), f"rank {r}")

        if p == 1:
            ts = [bt.torch_tensor().copy_(ts[0])]
            ev = torch.cuda.Event()
            ev.record()
            backend.mark_communication_ready(bt, ev.cuda_event)
            assert backend.wait_pending_comm_ops() == 1
        else:
            run_ranks(rank, p)
        for r in range(p):
            same_bytes(host(ts[r], dtype), want[r], f"step {step} rank {r}: result")
            same_bytes(host(states[r].worker_residual, F32), refs[r].worker, f"step {step} rank {r}: worker residual")
            same_bytes(host(states[r].server_residual, F32), refs[r].server, f"step {step} rank {r}: server residual")
    assert p == 1 or names.names == ["mxfp8_encode_ef_kernel", "mxfp8_reduce_encode_ef_kernel", "mxfp8_decode_kernel"]
    assert states[0].zero_() is states[0] and not host(states[0].worker_residual, F32).any()


# ---------------------------------------------- refusals: nothing is launched ----
def test_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comm, n = loopback_communicators(1, 0)[0], 4096
    g = torch.ones(n, device="cuda")
    bk = bc.BaguaBucketPy("mx8refuse", [bc.BaguaTensorPy(g, "mx8refuse.g")])
    st = bc.MXFP8ErrorFeedbackState(n, 1, 0)

    def append(bucket, state, codec="MXFP8", **kw):
        bucket.append_centralized_synchronous_op(comm, kw.pop("intra", None), compression=codec, error_feedback=state, **kw)

    with pytest.raises(RuntimeError, match="does not fit"):
        append(bk, bc.MXFP8ErrorFeedbackState(2048, 1, 0))
    for other in (bc.MXFP4ErrorFeedbackState(n, 1, 0), bc.OneBitErrorFeedbackState(n, 1, 0)):
        with pytest.raises(NotImplementedError):  # a state of another codec
            append(bk, other)
    with pytest.raises(NotImplementedError):
        append(bk, st, codec="MXFP4")
    with pytest.raises(NotImplementedError, match="hierarchical"):
        append(bk, st, intra=comm, hierarchical=True)
    assert bk.ops() == []
    append(bk, st)
    other = bc.BaguaBucketPy("mx8refuse2", [bc.BaguaTensorPy(torch.ones(n, device="cuda"), "mx8refuse2.g")])
    with pytest.raises(RuntimeError, match="one state, one op"):
        append(other, st)
    assert len(bk.ops()) == 1 and other.ops() == []
    # the C entries: a partly valid tensor, 17 segments, the residual checked first, a target chunk
    raw, sr, out = bc.BaguaTensorPy(g, "g").raw(), _raws(st), N.bagua_tensor_t()
    partly = N.bagua_tensor_t(raw.ptr, n - 8, n, raw.dtype, raw.device_id)
    assert N.C.bagua_centralized_mxfp8_error_feedback(comm.handle, ctypes.byref(partly), 1, ctypes.byref(sr[0]),
                                                      ctypes.byref(sr[1])) == UNSUPPORTED
    assert N.C.bagua_tensor_compress_mxfp8_error_feedback(ctypes.byref(partly), 1, 0, ctypes.byref(sr[0]),
                                                          ctypes.byref(out)) == UNSUPPORTED
    p, cs, S = 17, 64, R.compressed_bytes(64, 17)
    buf, seg = (torch.zeros(S, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = torch.zeros(cs, dtype=torch.float32, device="cuda")
    middle, ptrs = N.K.bagua_mxfp8_reduce_requantize_ef, (buf.data_ptr(), S, cs, p, 1, seg.data_ptr(), S, 0)
    assert middle(F32, *ptrs, res.data_ptr(), None) == UNSUPPORTED and middle(F32, *ptrs, None, None) == INVALID_ARG
    assert N.K.bagua_mxfp8_compress_ef(F32, g.data_ptr(), n, n, 1, seg.data_ptr(), S, 0, res.data_ptr(), None) == INVALID_ARG
    torch.cuda.synchronize()
    assert float(g.sum()) == float(n) and not seg.any() and not res.any() and not any(t.any() for t in st.tensors())
