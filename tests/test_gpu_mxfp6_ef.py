"""GPU tests of the MXFP6 codec's error feedback (MXFP6.md, "Error feedback"): the two HIP
kernels, the comm op on the loopback transport and the bucket path, byte for byte (segments,
slack included) and bit for bit (residuals, results) against the composition in
tests/mxfp6_ef_reference.py after every step."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import mxfp6_ef_reference as REF
import mxfp6_reference as R
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_mxfp6 import received
from test_gpu_mxfp8 import bc, dev_at, hostile_inputs, same_bytes, u8  # noqa: F401
from test_gpu_mxfp8_ef import step_grads
from test_gpu_op_edges import KernelNames
from test_mxfp6_cpu import tie_table

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
TILE = 2048  # elements of the worker step's wave tile: 8 rows of 256 f32, 4 rows of 512 f16 / bf16
# one element, the block's and the tile's edges, three tiles and a ragged third block; the block counts
# 1, 2, 4, 5, 64, 65 and 195 leave every payload slack: 8, 16, 24 and 0 bytes (nb mod 4 = 1, 2, 3, 0)
SIZES = [1, 31, 32, 33, 127, 128, 129, TILE - 1, TILE, TILE + 1, 3 * TILE + 69]


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in ("BAGUA_MX_EF_RESIDUAL_NT", "BAGUA_TUNE_MX6_ENCODE_BLOCKS", "BAGUA_TUNE_MX6_MIDDLE_BLOCKS"):
        monkeypatch.delenv(k, raising=False)


def worker_steps(bc, dtype, n_chunks, cs, steps, what, offset=0):
    """compress_with_error_feedback step by step against compress_ef, step 0 against the plain codec as well;
    yields each step's bytes and residual"""
    n = n_chunks * cs
    state, ref = bc.MXFP6ErrorFeedbackState(n, n_chunks, 0), REF.WorkerState(n)
    for step, x in enumerate(steps):
        xt = dev_at(x, dtype, offset)
        t = bc.BaguaTensorPy(xt, "g")
        got = t.compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        same_bytes(got, REF.compress_ef(x, dtype, n_chunks, ref), f"{what} step {step}: segments")
        if step == 0 and not np.signbit(NP.to_f32(x, dtype)[NP.to_f32(x, dtype) == 0]).any():
            same_bytes(got, t.compress("MXFP6", n_chunks, -1).to_numpy_u8(), f"{what} step 0 against the plain codec")
        same_bytes(host(state.worker_residual, F32), ref.residual, f"{what} step {step}: residual")
        same_bytes(host(xt, dtype), x, "the gradient is read only")
        yield got, host(state.worker_residual, F32)


# ------------------------------------------------------------------ codec ----
# with three chunks of odd size the second and third start off 16 B in gradient and residual
@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_worker_step_sizes(bc, dtype, nt, monkeypatch):
    monkeypatch.setenv("BAGUA_MX_EF_RESIDUAL_NT", nt)
    rng = np.random.default_rng(1000 * dtype + int(nt))
    for n_chunks in (1, 3):
        for cs in SIZES:
            xs = [step_grads(rng, n_chunks * cs, dtype) for _ in range(3)]
            res = list(worker_steps(bc, dtype, n_chunks, cs, xs, f"p={n_chunks} cs={cs}"))[-1][1]
            assert res.any() or cs == 1  # (a block of one element may be encoded exactly)
    # a gradient 4 B off 16-B alignment under a vector residual, tiles whole and ragged
    xs = [step_grads(rng, 4 * TILE + 80, dtype) for _ in range(2)]
    assert len(list(worker_steps(bc, dtype, 2, 2 * TILE + 40, xs, "misaligned", offset=1 if dtype == F32 else 2))) == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_chunk_with_a_residual_only_4_byte_aligned(bc, dtype):
    """bagua_mxfp6_compress_ef on one chunk with residual + cs, cs = 4097 (the composed middle step's call)"""
    cs = 4097
    rng = np.random.default_rng(55 + dtype)
    res = torch.zeros(2 * cs, dtype=torch.float32, device="cuda")
    assert (res.data_ptr() + 4 * cs) % 16 == 4
    ref = REF.WorkerState(cs)
    S = R.compressed_bytes(cs, 1)
    for step in range(3):
        x = step_grads(rng, cs, dtype)
        out = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
        assert bc._native.K.bagua_mxfp6_compress_ef(dtype, dev(x, dtype).data_ptr(), cs, cs, 1, out.data_ptr(), S, -1,
                                                    res.data_ptr() + 4 * cs, None) == OK
        same_bytes(u8(out), REF.compress_ef(x, dtype, 1, ref), f"step {step}: segment")
        same_bytes(host(res, F32)[cs:], ref.residual, f"step {step}: residual")
        assert not host(res, F32)[:cs].any(), "the residual before the chunk's is untouched"


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_inputs(bc, dtype):
    """ordinary gradients, the hostile tensor, ordinary again: a NaN block resets its residuals to +0, +-inf
    and the largest finite T clamp, -0 is encoded as +0; the tie table goes first, onto a zero state, and third"""
    cases, p = hostile_inputs(dtype)
    cases["ties"] = NP.from_f32(tie_table(dtype)[0].astype(np.float32).ravel(), dtype)
    rng = np.random.default_rng(3 + dtype)
    for name, bad in cases.items():
        n = bad.size
        cs = n // p
        nb, seg = R.blocks(cs), R.segment_bytes(cs)
        fine = [step_grads(rng, n, dtype) for _ in range(2)]
        steps = [bad, fine[0], bad] if name == "ties" else [fine[0], bad, fine[1]]
        for step, (got, res) in enumerate(worker_steps(bc, dtype, p, cs, steps, name)):
            assert np.isfinite(res).all(), f"{name}, step {step}: the state must stay finite"
            scales = np.concatenate([got[c * seg:c * seg + nb] for c in range(p)])
            if step == 1 and name.startswith("nan"):  # one NaN block per chunk, all 32 residuals +0 bits
                j = int(np.nonzero(np.isnan(NP.to_f32(bad, dtype)))[0][0])
                assert (scales == 0xFF).sum() == p and not res[j - j % 32:min(j - j % 32 + 32, cs)].view(np.uint32).any(), name
            assert step != 2 or 0xFF not in scales


# ------------------------------------------------------------ middle step ----
# p = 2, 5, 16: one per BY (2, 4, 8), 5 with a partly filled second round of the tree
def middle_steps(bc, dtype, p, average, sizes):
    """three steps against middle_ef; step 1 takes the plain middle step's hostile segments: a NaN block in
    segment 0 (its residuals reset) and, on f16, a sum that leaves the range (clamped)"""
    for cs in sizes:
        rng = np.random.default_rng(100 * dtype + 7 * p + cs)
        target, seg = p // 2, R.segment_bytes(cs)
        res = torch.zeros(cs + 1, dtype=torch.float32, device="cuda")[1 if cs == 33 else 0:][:cs]
        ref = np.zeros(cs, np.float32)
        for step in range(3):
            recv = received(rng, p, cs, dtype) if step == 1 else R.compress(step_grads(rng, p * cs, dtype), dtype, p)
            S = recv.size
            rt = torch.from_numpy(recv).cuda()
            out = torch.full((S,), 0xCD, dtype=torch.uint8, device="cuda")
            what = f"p={p} cs={cs} average={average} step {step}"
            assert bc._native.K.bagua_mxfp6_reduce_requantize_ef(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(),
                                                                 S, target, res.data_ptr(), None) == OK, what
            want = np.full(S, 0xCD, np.uint8)
            want[target * seg:(target + 1) * seg] = REF.middle_ef(NP, recv, p, cs, dtype, target, bool(average), ref)
            same_bytes(u8(out), want, what)
            same_bytes(host(res, F32), ref, what + ": residual")
            assert np.isfinite(ref).all() and (step or ref.any())
            if step == 1:  # received() plants its NaN at element 37 of the p * cs
                b = 37 % cs // 32
                assert want[target * seg + b] == 0xFF and not ref[32 * b:32 * b + 32].view(np.uint32).any()


@pytest.mark.parametrize("average", [1, 0])
@pytest.mark.parametrize("p", [2, 5, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step(bc, dtype, p, average):
    """cs = 33: two blocks, the second ragged, a residual that is only 4-B aligned; 8193 + 64: two workgroups,
    259 blocks"""
    middle_steps(bc, dtype, p, average, (33, 8193 + 64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_workgroup_walks_the_grid_stride_loops(bc, dtype, monkeypatch):
    """the grid caps at one workgroup: ten wave tiles (the last ragged) for the four waves of the worker step,
    259 blocks for the 256 lanes of the middle step, so both loops take a second turn"""
    monkeypatch.setenv("BAGUA_TUNE_MX6_ENCODE_BLOCKS", "1")
    monkeypatch.setenv("BAGUA_TUNE_MX6_MIDDLE_BLOCKS", "1")
    cs = 9 * TILE + 69
    rng = np.random.default_rng(70 + dtype)
    xs = [step_grads(rng, cs, dtype) for _ in range(3)]
    assert list(worker_steps(bc, dtype, 1, cs, xs, f"one workgroup cs={cs}"))[-1][1].any()
    middle_steps(bc, dtype, 5, 1, (8193 + 64,))


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
    states = [bc.MXFP6ErrorFeedbackState(n, p, 0) for _ in range(p)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    names = KernelNames(N, comms[0])
    if p == 1:
        bt = bc.BaguaTensorPy(torch.zeros(n, device="cuda"), "g")
        bk = bc.BaguaBucketPy("mxfp6_ef_bucket", [bt])
        bk.append_centralized_synchronous_op(comms[0], None, average=True, compression="MXFP6", error_feedback=states[0])
        assert type(bk.ops()[0]).__name__ == "CentralizedMXFP6ErrorFeedback" and "MXFP6ErrorFeedbackState" in repr(states[0])
        assert bk.ops()[0].native().kind == N.BUCKET_OP_CENTRALIZED_MXFP6_ERROR_FEEDBACK == 10
        backend = bc.BaguaCommBackendPy(4, 0)
        backend.register_ordered_buckets([bk])
    for step in range(3):
        xs = [step_grads(rng, n, dtype, r) for r in range(p)]
        want, sent = REF.centralized_step(NP, xs, dtype, refs, True)
        if step == 0:  # zero state: the plain op's wire bytes
            for r in range(p):
                same_bytes(sent[r], R.compress(xs[r], dtype, p), f"rank {r}: step 0 on the wire")
        ts = [dev_at(x, dtype, 1 if r == misalign_rank else 0) for r, x in enumerate(xs)]
        torch.cuda.synchronize()

        def rank(r):
            raw, sr = bc.BaguaTensorPy(ts[r], f"g{r}").raw(), _raws(states[r])
            with names if r == 0 and step == 0 else contextlib.nullcontext():  # rank 0's first step: its kernels' names
                N.check(N.C.bagua_centralized_mxfp6_error_feedback(comms[r].handle, ctypes.byref(raw), 1,
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
    assert p == 1 or names.names == ["mxfp6_encode_ef_kernel", "mxfp6_reduce_encode_ef_kernel", "mxfp6_decode_kernel"]
    assert states[0].zero_() is states[0] and not host(states[0].worker_residual, F32).any()


# ---------------------------------------------- refusals: nothing is launched ----
def test_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comm, n = loopback_communicators(1, 0)[0], 4096
    g = torch.ones(n, device="cuda")
    bk = bc.BaguaBucketPy("mx6refuse", [bc.BaguaTensorPy(g, "mx6refuse.g")])
    st = bc.MXFP6ErrorFeedbackState(n, 1, 0)

    def append(bucket, state, codec="MXFP6", **kw):
        bucket.append_centralized_synchronous_op(comm, kw.pop("intra", None), compression=codec, error_feedback=state, **kw)

    with pytest.raises(RuntimeError, match="does not fit"):
        append(bk, bc.MXFP6ErrorFeedbackState(2048, 1, 0))
    for other in (bc.MXFP4ErrorFeedbackState(n, 1, 0), bc.MXFP8ErrorFeedbackState(n, 1, 0), bc.OneBitErrorFeedbackState(n, 1, 0)):
        with pytest.raises(NotImplementedError):  # a state of another codec
            append(bk, other)
    with pytest.raises(NotImplementedError):
        append(bk, st, codec="MXFP8")
    with pytest.raises(NotImplementedError, match="hierarchical"):
        append(bk, st, intra=comm, hierarchical=True)
    with pytest.raises(NotImplementedError):  # no stochastic rounding for this codec, alone or beside error feedback
        append(bk, st, stochastic_rounding=bc.MXFP8StochasticRounding(7))
    assert bk.ops() == []
    # the C entries: a partly valid tensor, a missing residual, 17 segments, the residual checked first
    raw, sr, out = bc.BaguaTensorPy(g, "g").raw(), _raws(st), N.bagua_tensor_t()
    partly = N.bagua_tensor_t(raw.ptr, n - 8, n, raw.dtype, raw.device_id)
    op = N.C.bagua_centralized_mxfp6_error_feedback
    assert op(comm.handle, ctypes.byref(partly), 1, ctypes.byref(sr[0]), ctypes.byref(sr[1])) == UNSUPPORTED
    assert op(comm.handle, ctypes.byref(raw), 1, ctypes.byref(sr[0]), None) == INVALID_ARG
    assert N.C.bagua_tensor_compress_mxfp6_error_feedback(ctypes.byref(partly), 1, 0, ctypes.byref(sr[0]),
                                                          ctypes.byref(out)) == UNSUPPORTED
    p, cs, S17, S = 17, 64, R.compressed_bytes(64, 17), R.compressed_bytes(n, 1)
    buf, seg = (torch.zeros(max(S, S17) + 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = torch.zeros(n, dtype=torch.float32, device="cuda")
    bp, sp, rp = buf.data_ptr(), seg.data_ptr(), res.data_ptr()
    middle, worker = N.K.bagua_mxfp6_reduce_requantize_ef, N.K.bagua_mxfp6_compress_ef
    assert middle(F32, bp, S17, cs, p, 1, sp, S17, 0, rp, None) == UNSUPPORTED
    assert middle(F32, bp, S17, cs, p, 1, sp, S17, 0, None, None) == INVALID_ARG
    # the middle step's buffers: short input, short output, input and output off 16 B
    for b, bs, o, osz in ((bp, S - 1, sp, S), (bp, S, sp, S - 1), (bp + 8, S, sp, S), (bp, S, sp + 8, S)):
        assert middle(F32, b, bs, n, 1, 1, o, osz, 0, rp, None) == INVALID_ARG
    # the worker step: a target chunk, a partly valid tensor, no residual, a short and a misaligned output
    for num, target, o, osz, r in ((n, 0, sp, S, rp), (n - 8, -1, sp, S, rp), (n, -1, sp, S, None), (n, -1, sp, S - 1, rp),
                                   (n, -1, sp + 4, S, rp)):
        assert worker(F32, g.data_ptr(), num, n, 1, o, osz, target, r, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert float(g.sum()) == float(n) and not seg.any() and not res.any() and not any(t.any() for t in st.tensors())
