"""GPU tests of the MXFP4 codec's error feedback (MXFP4.md, "Error feedback"): the two HIP
kernels, the comm op on the loopback transport and the bucket path, byte for byte (payload)
and bit for bit (residuals, results) against the composition in tests/mxfp4_ef_reference.py
after every step."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mxfp4_ef_reference as REF
import mxfp4_reference as R
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_mxfp4 import dev_at, grads, hostile_inputs, received, same_bytes, u8
from test_gpu_op_edges import KernelNames

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


def f32_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def step_grads(rng, n, dtype, r=0):
    """gradients of one step: block-wise magnitudes (grads) plus a per-rank offset; values that
    round to -0 in T become +0 (x + (+0) turns a -0 into +0, so only then is step 0 the plain
    codec's; test_signed_zeros_and_a_zero_chunk covers -0)"""
    x = NP.to_f32(grads(rng, n, dtype), dtype) + np.float32(0.0005 * r)
    x = NP.to_f32(NP.from_f32(x.astype(np.float32), dtype), dtype)
    x[x == 0] = 0.0
    return NP.from_f32(x.astype(np.float32), dtype)


# ------------------------------------------------------------------ codec ----
# one block, the block edge, one f32 wave tile (2048) and its edge, the 16-bit wave tile's edge
# (4096 + 1), a ragged tail whose chunks start off 16 B (4100 elements of 2 B), several workgroups
SHAPES = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 2048), (1, 2049), (4, 4097), (3, 4100), (8, 20000)]


def codec_steps(bc, dtype, n_chunks, cs, steps=4, offset=0):
    n = n_chunks * cs
    rng = np.random.default_rng(1000 * dtype + n)
    state = bc.MXFP4ErrorFeedbackState(n, n_chunks, 0)
    ref = REF.WorkerState(n)
    for step in range(steps):
        x = step_grads(rng, n, dtype)
        xt = dev_at(x, dtype, offset)
        assert (xt.data_ptr() % 16 != 0) == bool(offset)
        t = bc.BaguaTensorPy(xt, "g")
        if step == 0:
            plain = t.compress("MXFP4", n_chunks, -1).to_numpy_u8()
        got = t.compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        want = REF.compress_ef(x, dtype, n_chunks, ref)
        same_bytes(got, want, f"step {step}: payload")
        if step == 0:  # zero state (and no -0 in the input): the plain codec's bytes
            same_bytes(got, plain, "step 0 against the plain codec")
        same_bytes(f32_host(state.worker_residual), ref.residual, f"step {step}: residual")
        same_bytes(host(xt, dtype), x, "the gradient is read only")
    assert ref.residual.any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_chunks,cs", SHAPES)
def test_codec_steps_match_reference(bc, dtype, n_chunks, cs):
    codec_steps(bc, dtype, n_chunks, cs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_codec_one_workgroup_walks_the_grid_stride_loop(bc, dtype, monkeypatch):
    monkeypatch.setenv("BAGUA_TUNE_MX_ENCODE_BLOCKS", "1")
    codec_steps(bc, dtype, 8, 20000)


@pytest.mark.parametrize("dtype", DTYPES)
def test_codec_misaligned_gradient_view(bc, dtype):
    """the gradient starts one element into its allocation: guarded loads, vector residual"""
    codec_steps(bc, dtype, 2, 4096, offset=1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_chunk_with_a_residual_only_4_byte_aligned(bc, dtype):
    """bagua_mxfp4_compress_ef on chunk 1 alone with residual + cs, cs = 4097 (the composed middle step's call)"""
    K = bc._native.K
    cs = 4097
    rng = np.random.default_rng(55 + dtype)
    res = torch.zeros(2 * cs, dtype=torch.float32, device="cuda")
    assert (res.data_ptr() + 4 * cs) % 16 == 4
    ref = REF.WorkerState(cs)
    S = R.compressed_bytes(cs, 1)
    for step in range(3):
        x = step_grads(rng, cs, dtype)
        xt = dev(x, dtype)
        out = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
        assert K.bagua_mxfp4_compress_ef(dtype, xt.data_ptr(), cs, cs, 1, out.data_ptr(), S, -1,
                                         res.data_ptr() + 4 * cs, None) == OK
        same_bytes(u8(out), REF.compress_ef(x, dtype, 1, ref), f"step {step}: payload")
        got = f32_host(res)
        same_bytes(got[cs:], ref.residual, f"step {step}: residual")
        assert not got[:cs].any(), "the residual before the chunk's is untouched"


# --------------------------------------------------------- hostile inputs ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_inputs(bc, dtype):
    """step 0 ordinary gradients, step 1 the hostile tensor, step 2 ordinary again: a NaN block
    resets its residuals and the step after it is clean"""
    cases, p = hostile_inputs(dtype)
    rng = np.random.default_rng(3 + dtype)
    for name, bad in cases.items():
        n = bad.size
        cs = n // p
        state = bc.MXFP4ErrorFeedbackState(n, p, 0)
        ref = REF.WorkerState(n)
        for step, x in enumerate([step_grads(rng, n, dtype), bad, step_grads(rng, n, dtype)]):
            got = bc.BaguaTensorPy(dev(x, dtype), "g").compress_with_error_feedback(p, state).to_numpy_u8()
            same_bytes(got, REF.compress_ef(x, dtype, p, ref), f"{name}, step {step}: payload")
            res = f32_host(state.worker_residual)
            same_bytes(res, ref.residual, f"{name}, step {step}: residual")
            assert np.isfinite(res).all(), f"{name}, step {step}: the state must stay finite"
            if step == 1 and name.startswith("nan"):
                nanpos = np.nonzero(np.isnan(NP.to_f32(bad, dtype)))[0]
                for j in nanpos:
                    c, b = j // cs, (j % cs) // 32
                    blk = res[c * cs + 32 * b:min(c * cs + 32 * b + 32, (c + 1) * cs)]
                    assert not blk.view(np.uint32).any(), f"{name}: the NaN block's residuals are +0"
                assert got[:R.blocks(cs)].tolist().count(0xFF) == 1
            if step == 2:
                assert 0xFF not in got[:R.blocks(cs)].tolist() and 0xFF not in got[R.segment_bytes(cs):][:R.blocks(cs)].tolist()


def test_signed_zeros_and_a_zero_chunk(bc):
    p, cs = 3, 2048 + 7
    n = p * cs
    rng = np.random.default_rng(9)
    state = bc.MXFP4ErrorFeedbackState(n, p, 0)
    ref = REF.WorkerState(n)
    for step in range(4):
        x = step_grads(rng, n, F32)
        x[::5] = 0.0
        x[1::5] = -0.0
        x[cs:2 * cs] = 0.0 if step % 2 == 0 else -0.0
        got = bc.BaguaTensorPy(dev(x, F32), "g").compress_with_error_feedback(p, state).to_numpy_u8()
        same_bytes(got, REF.compress_ef(x, F32, p, ref), f"step {step}: payload")
        same_bytes(f32_host(state.worker_residual), ref.residual, f"step {step}: residual")


# ------------------------------------------------------------ middle step ----
def middle_case(bc, dtype, p, cs, average, steps=2, seed=0):
    """-> [(segment bytes, residual)] per step, each compared with the reference composition"""
    K = bc._native.K
    rng = np.random.default_rng(100 * dtype + 7 * p + cs + seed)
    target = p // 2
    res = torch.zeros(cs, dtype=torch.float32, device="cuda")
    ref = np.zeros(cs, np.float32)
    seg = R.segment_bytes(cs)
    outs = []
    for step in range(steps):
        # step 0 ordinary segments; then, where they fit, the plain middle step's hostile ones (a NaN
        # block in segment 0, on f16 a sum that leaves the range)
        hostile = step > 0 and p * cs > 64
        recv = received(rng, p, cs, dtype) if hostile else R.compress(step_grads(rng, p * cs, dtype), dtype, p)
        S = recv.size
        rt = torch.from_numpy(recv).cuda()
        out = torch.full((S,), 0xCD, dtype=torch.uint8, device="cuda")
        what = f"p={p} cs={cs} average={average} step {step}"
        assert K.bagua_mxfp4_reduce_requantize_ef(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(), S, target,
                                                  res.data_ptr(), None) == OK, what
        want = np.full(S, 0xCD, np.uint8)
        want[target * seg:(target + 1) * seg] = REF.middle_ef(NP, recv, p, cs, dtype, target, bool(average), ref)
        got = u8(out)
        same_bytes(got, want, what)
        same_bytes(f32_host(res), ref, what + ": residual")
        outs.append((got[target * seg:(target + 1) * seg].copy(), f32_host(res).copy()))
    return outs


@pytest.mark.parametrize("average", [1, 0])
@pytest.mark.parametrize("p", list(range(1, 17)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step(bc, dtype, p, average):
    for cs in (33, 4100):
        middle_case(bc, dtype, p, cs, average)


def test_middle_step_refuses_17_segments(bc):
    K = bc._native.K
    p, cs = 17, 64
    S = R.compressed_bytes(cs, p)
    buf = torch.zeros(S, dtype=torch.uint8, device="cuda")
    out = torch.zeros(S, dtype=torch.uint8, device="cuda")
    res = torch.zeros(cs, dtype=torch.float32, device="cuda")
    assert K.bagua_mxfp4_reduce_requantize_ef(F32, buf.data_ptr(), S, cs, p, 1, out.data_ptr(), S, 0, res.data_ptr(),
                                              None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any() and not res.any()


# ------------------------------------------- the arithmetic in place of the conversions ----
def hwcvt_cases(bc):
    """what the child process (BAGUA_MXFP4_HWCVT=0) and this process both compute"""
    out = {}
    for dtype in DTYPES:
        for n_chunks, cs in ((1, 33), (3, 4100)):
            n = n_chunks * cs
            rng = np.random.default_rng(17 + dtype + n)
            state = bc.MXFP4ErrorFeedbackState(n, n_chunks, 0)
            ref = REF.WorkerState(n)
            for step in range(3):
                x = step_grads(rng, n, dtype)
                got = bc.BaguaTensorPy(dev(x, dtype), "g").compress_with_error_feedback(n_chunks, state).to_numpy_u8()
                same_bytes(got, REF.compress_ef(x, dtype, n_chunks, ref), f"dtype {dtype} cs {cs} step {step}")
                out[f"enc_{dtype}_{cs}_{step}"] = got
                out[f"res_{dtype}_{cs}_{step}"] = f32_host(state.worker_residual).view(np.uint32).copy()
        for p in (2, 8):
            for step, (seg, res) in enumerate(middle_case(bc, dtype, p, 4100, 1)):
                out[f"mid_{dtype}_{p}_{step}"] = seg
                out[f"midres_{dtype}_{p}_{step}"] = res.view(np.uint32).copy()
    return out


def test_arithmetic_path_in_child_process(bc, tmp_path):
    path = str(tmp_path / "sw.npz")
    env = dict(os.environ, BAGUA_MXFP4_HWCVT="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "mxfp4_ef_child.py"), path], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.environ.get("BAGUA_MXFP4_HWCVT", "1") != "0"
    here = hwcvt_cases(bc)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(here)
        for k in here:
            same_bytes(z[k], here[k], k)


# ------------------------------------------------- the op on the loopback transport ----
def _raws(st):
    return [st._raw(t) for t in st.tensors()]


def run_op_steps(bc, p, dtype, cs, average, steps=3, misalign_rank=None):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    n = p * cs
    rng = np.random.default_rng(p * 1000 + dtype * 10 + cs)
    comms = loopback_communicators(p, 0)
    states = [bc.MXFP4ErrorFeedbackState(n, p, 0) for _ in range(p)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    names = []
    for step in range(steps):
        xs = [step_grads(rng, n, dtype, r) for r in range(p)]
        want, _ = REF.centralized_step(NP, xs, dtype, refs, bool(average))
        ts = [dev_at(x, dtype, 1 if r == misalign_rank else 0) for r, x in enumerate(xs)]
        torch.cuda.synchronize()

        def rank(r):
            raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
            sr = _raws(states[r])
            if r == 0 and step == 0:
                with KernelNames(N, comms[0]) as k:
                    rc = N.C.bagua_centralized_mxfp4_error_feedback(comms[r].handle, ctypes.byref(raw), average,
                                                                    ctypes.byref(sr[0]), ctypes.byref(sr[1]))
                names.extend(k.names)
            else:
                rc = N.C.bagua_centralized_mxfp4_error_feedback(comms[r].handle, ctypes.byref(raw), average,
                                                                ctypes.byref(sr[0]), ctypes.byref(sr[1]))
            N.check(rc, f"rank {r}")

        run_ranks(rank, p)
        outs = [host(t, dtype) for t in ts]
        for r in range(p):
            same_bytes(outs[r], want[r], f"step {step} rank {r}: result")
            same_bytes(outs[r], outs[0], f"step {step}: rank {r} against rank 0")
            same_bytes(f32_host(states[r].worker_residual), refs[r].worker, f"step {step} rank {r}: worker residual")
            same_bytes(f32_host(states[r].server_residual), refs[r].server, f"step {step} rank {r}: server residual")
    return names


def check_fused_path(names, p):
    assert "mxfp4_encode_ef_kernel" in names and "mxfp4_decode_kernel" in names, names
    assert "mxfp4_encode_kernel" not in names and "mxfp4_reduce_encode_kernel" not in names, names
    if p <= 16:
        assert "mxfp4_reduce_encode_ef_kernel" in names and "reduce_chunks_kernel" not in names, names
        assert len(names) == 3, names
    else:
        assert "reduce_chunks_kernel" in names and "mxfp4_reduce_encode_ef_kernel" not in names, names
        assert names.count("mxfp4_encode_ef_kernel") == 2 and names.count("mxfp4_decode_kernel") == 2, names


@pytest.mark.parametrize("p,dtype,cs", [(1, F32, 70000), (2, F32, 40000), (3, F32, 3072), (4, F16, 8192),
                                        (8, BF16, 20000), (16, F32, 4096)])
def test_op_matches_reference(bc, p, dtype, cs):
    check_fused_path(run_op_steps(bc, p, dtype, cs, 1), p)


def test_op_sum(bc):
    run_op_steps(bc, 4, F32, 5000, 0)


def test_op_more_ranks_than_the_fused_middle_step(bc):
    """17 chunks: the middle step composed from decode + reduce + the worker encode on the own chunk"""
    check_fused_path(run_op_steps(bc, 17, F32, 1536, 1, steps=2), 17)


def test_op_misaligned_gradient_on_one_rank(bc):
    run_op_steps(bc, 2, F32, 40000, 1, steps=2, misalign_rank=1)


# ------------------------------------------------------------ bucket path ----
def test_bucket_path_scattered(bc):
    from bagua_core.bucket import CentralizedMXFP4ErrorFeedback
    from bagua_core.communicator import loopback_communicators
    p, dtype = 2, F32
    sizes = [3000, 5192]
    n = sum(sizes)
    rng = np.random.default_rng(606)
    comms = loopback_communicators(p, 0)
    steps_x = [[step_grads(rng, n, dtype, r) for r in range(p)] for _ in range(2)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    wants = [REF.centralized_step(NP, xs, dtype, refs, True)[0] for xs in steps_x]
    parts, gaps, states, buckets = [], [], [], []
    for r in range(p):
        a = torch.zeros(sizes[0], device="cuda")
        gaps.append(torch.empty(4096, device="cuda"))  # keeps the two tensors apart
        b = torch.zeros(sizes[1], device="cuda")
        parts.append([a, b])
        bk = bc.BaguaBucketPy(f"mxef{r}", [bc.BaguaTensorPy(a, f"r{r}.a"), bc.BaguaTensorPy(b, f"r{r}.b")])
        st = bc.MXFP4ErrorFeedbackState(n, p, 0)
        bk.append_centralized_synchronous_op(comms[r], None, hierarchical=False, average=True, compression="MXFP4",
                                             error_feedback=st)
        ops = bk.ops()
        assert len(ops) == 1 and isinstance(ops[0], CentralizedMXFP4ErrorFeedback) and ops[0].state is st
        assert "MXFP4ErrorFeedbackState" in repr(st) and len(st.tensors()) == 2
        states.append(st)
        buckets.append(bk)

    def run_step(xs):
        for r in range(p):
            parts[r][0].copy_(torch.from_numpy(xs[r][:sizes[0]]))
            parts[r][1].copy_(torch.from_numpy(xs[r][sizes[0]:]))
        torch.cuda.synchronize()
        run_ranks(lambda r: buckets[r].execute_ops(), p)
        torch.cuda.synchronize()
        return [np.concatenate([parts[r][0].cpu().numpy(), parts[r][1].cpu().numpy()]) for r in range(p)]

    first = None
    for step, xs in enumerate(steps_x):
        outs = run_step(xs)
        first = first or outs
        for r in range(p):
            same_bytes(outs[r], wants[step][r], f"step {step} rank {r}")
    for r in range(p):
        same_bytes(f32_host(states[r].worker_residual), refs[r].worker, f"rank {r}: worker residual")
        same_bytes(f32_host(states[r].server_residual), refs[r].server, f"rank {r}: server residual")
        states[r].zero_()
    again = run_step(steps_x[0])
    for r in range(p):
        same_bytes(again[r], first[r], f"rank {r}: zeroed state must reproduce step 1")


# ---------------------------------------------- refusals: nothing is launched ----
def test_python_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    comm = loopback_communicators(1, 0)[0]
    g = torch.ones(4096, device="cuda")
    bk = bc.BaguaBucketPy("mxrefuse", [bc.BaguaTensorPy(g, "mxrefuse.g")])
    st = bc.MXFP4ErrorFeedbackState(4096, 1, 0)
    ob = bc.OneBitErrorFeedbackState(4096, 1, 0)
    with pytest.raises(NotImplementedError):   # a state of the wrong kind for the codec
        bk.append_centralized_synchronous_op(comm, None, compression="MXFP4", error_feedback=ob)
    with pytest.raises(NotImplementedError):
        bk.append_centralized_synchronous_op(comm, None, compression="OneBitSignScale", error_feedback=st)
    with pytest.raises(NotImplementedError, match="OneBitSignScale"):
        bk.append_centralized_synchronous_op(comm, None, compression="MinMaxUInt8", error_feedback=st)
    with pytest.raises(NotImplementedError, match="OneBitSignScale"):
        bk.append_centralized_synchronous_op(comm, None, compression=None, error_feedback=st)
    with pytest.raises(NotImplementedError, match="hierarchical"):
        bk.append_centralized_synchronous_op(comm, comm, hierarchical=True, compression="MXFP4", error_feedback=st)
    with pytest.raises(RuntimeError, match="does not fit"):
        bk.append_centralized_synchronous_op(comm, None, compression="MXFP4",
                                             error_feedback=bc.MXFP4ErrorFeedbackState(2048, 1, 0))
    assert bk.ops() == []
    bk.append_centralized_synchronous_op(comm, None, compression="MXFP4", error_feedback=st)
    other = bc.BaguaBucketPy("mxrefuse2", [bc.BaguaTensorPy(torch.ones(4096, device="cuda"), "mxrefuse2.g")])
    with pytest.raises(RuntimeError, match="one state, one op"):
        other.append_centralized_synchronous_op(comm, None, compression="MXFP4", error_feedback=st)
    assert len(bk.ops()) == 1 and other.ops() == []
    with pytest.raises(RuntimeError, match="error-feedback state is for"):
        bc.BaguaTensorPy(g, "g").compress_with_error_feedback(1, bc.MXFP4ErrorFeedbackState(2048, 1, 0))
    torch.cuda.synchronize()
    assert float(g.sum()) == 4096.0
    assert all(float(t.abs().sum()) == 0.0 for t in st.tensors() + ob.tensors())


def test_native_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comm = loopback_communicators(1, 0)[0]
    n = 4096
    g = torch.ones(n, device="cuda")
    st = bc.MXFP4ErrorFeedbackState(n, 1, 0)
    op = N.C.bagua_centralized_mxfp4_error_feedback

    def call(raw, sr):
        return op(comm.handle, ctypes.byref(raw), 1, ctypes.byref(sr[0]), ctypes.byref(sr[1]))

    raw = bc.BaguaTensorPy(g, "g").raw()
    good = _raws(st)
    small = _raws(bc.MXFP4ErrorFeedbackState(n // 2, 1, 0))
    for i in range(2):  # each state tensor in turn: wrong size, wrong dtype, wrong device, misaligned, absent
        for field, value in (("num_elem", None), ("dtype", N.DTYPE_F16), ("device_id", 1)):
            sr = _raws(st)
            if value is None:
                sr[i] = small[i]
            else:
                setattr(sr[i], field, value)
            assert call(raw, sr) == INVALID_ARG, (i, field)
        sr = _raws(st)
        sr[i].ptr += 4
        assert call(raw, sr) == INVALID_ARG, (i, "alignment")
        sr = _raws(st)
        sr[i] = N.bagua_tensor_t()
        assert call(raw, sr) == INVALID_ARG, (i, "absent")
    partly = N.bagua_tensor_t(raw.ptr, n - 8, n, raw.dtype, raw.device_id)
    assert call(partly, good) == UNSUPPORTED
    ints = N.bagua_tensor_t(raw.ptr, n, n, N.DTYPE_I64, raw.device_id)
    assert call(ints, good) == UNSUPPORTED
    out = N.bagua_tensor_t()
    assert N.C.bagua_tensor_compress_mxfp4_error_feedback(ctypes.byref(partly), 1, 0, ctypes.byref(good[0]),
                                                          ctypes.byref(out)) == UNSUPPORTED
    assert N.C.bagua_tensor_compress_mxfp4_error_feedback(ctypes.byref(raw), 1, 0, ctypes.byref(small[0]),
                                                          ctypes.byref(out)) == INVALID_ARG
    torch.cuda.synchronize()
    assert float(g.sum()) == float(n) and all(float(t.abs().sum()) == 0.0 for t in st.tensors())
    # the native bucket: hierarchical mode, another codec, a missing residual, a present scale field
    bk = bc.BaguaBucketPy("mx_native_refuse", [bc.BaguaTensorPy(g, "mx_native_refuse.g")])

    def nop(**kw):
        args = dict(kind=N.BUCKET_OP_CENTRALIZED_MXFP4_ERROR_FEEDBACK, average=1, compression=N.COMPRESSION_MXFP4,
                    fused=1, comm=comm.handle.value, ef_worker_carry=good[0], ef_server_carry=good[1])
        args.update(kw)
        return N.bagua_bucket_op_t(**args)

    def append(o):
        return N.C.bagua_bucket_append_op(bk.handle, ctypes.byref(o))

    assert append(nop(intranode=comm.handle.value)) == UNSUPPORTED
    assert append(nop(compression=N.COMPRESSION_ONEBIT)) == UNSUPPORTED
    assert append(nop(compression=N.COMPRESSION_MINMAX_UINT8)) == UNSUPPORTED
    assert append(nop(ef_server_carry=N.bagua_tensor_t())) == INVALID_ARG
    assert append(nop(ef_worker_carry=N.bagua_tensor_t())) == INVALID_ARG
    assert append(nop(ef_worker_scales=good[1])) == INVALID_ARG
    assert append(nop(ef_server_scale=good[1])) == INVALID_ARG
    assert N.C.bagua_bucket_num_ops(bk.handle) == 0
    assert append(nop()) == OK and N.C.bagua_bucket_num_ops(bk.handle) == 1


def test_ranks_disagreeing_on_error_feedback(bc, monkeypatch):
    """rank 0 runs the op with error feedback, rank 1 the plain MXFP4 op: with the schedule
    check on, both get BAGUA_ERR_INVALID_ARG before any byte is exchanged"""
    monkeypatch.setenv("BAGUA_CHECK_SCHEDULE", "1")
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    p, cs = 2, 40000
    n = p * cs
    rng = np.random.default_rng(8)
    xs = [step_grads(rng, n, F32, r) for r in range(p)]
    comms = loopback_communicators(p, 0)
    ts = [dev(x, F32) for x in xs]
    st = bc.MXFP4ErrorFeedbackState(n, p, 0)
    torch.cuda.synchronize()
    rcs = [None] * p

    def rank(r):
        raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
        if r == 0:
            sr = _raws(st)
            rcs[r] = N.C.bagua_centralized_mxfp4_error_feedback(comms[r].handle, ctypes.byref(raw), 1,
                                                                ctypes.byref(sr[0]), ctypes.byref(sr[1]))
        else:
            rcs[r] = N.C.bagua_centralized_low_precision_synchronous(comms[r].handle, ctypes.byref(raw), 1,
                                                                     N.COMPRESSION_MXFP4)

    run_ranks(rank, p)
    assert rcs == [INVALID_ARG] * p, rcs
    for r in range(p):
        same_bytes(host(ts[r], F32), xs[r], f"rank {r} changed")
    assert all(float(t.abs().sum()) == 0.0 for t in st.tensors())
