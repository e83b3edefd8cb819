"""GPU tests of the 1-bit codec's error feedback: the HIP kernels (onebit_ef.hip), the
comm op on the loopback transport and the bucket path, bit for bit against the
oracle composition in tests/onebit_ef_reference.py -- payload, carry and scales
after every step."""
import ctypes

import numpy as np
import pytest
import torch

import onebit_ef_reference as REF
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


def f32_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def grads(rng, n, dt, r=0):
    return NP.from_f32((rng.standard_normal(n) * 1e-3 + 0.0005 * r).astype(np.float32), dt)


def check_worker(state, ref, what):
    assert bits_equal(f32_host(state.worker_carry), ref.carry), f"{what}: carry"
    assert bits_equal(f32_host(state.worker_scales), ref.scales), f"{what}: scales"


# ---- codec -----------------------------------------------------------------
SHAPES = [(1, 1), (1, 1023), (1, 1024), (1, 1025), (4, 1025), (3, 4096 + 4), (8, 20000)]


@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("n_chunks,cs", SHAPES)
def test_codec_steps_match_reference(bc, oracle_c, dt, n_chunks, cs):
    n = n_chunks * cs
    rng = np.random.default_rng(1000 * dt + n)
    state = bc.OneBitErrorFeedbackState(n, n_chunks, 0)
    ref = REF.WorkerState(n, n_chunks)
    for step in range(4):
        x = grads(rng, n, dt)
        t = bc.BaguaTensorPy(dev(x, dt), "g")
        if step == 0:  # zero state: the plain codec's bytes
            plain = t.compress("OneBitSignScale", n_chunks, -1).to_numpy_u8()
        got = t.compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        want = REF.compress_ef(oracle_c, x, dt, n_chunks, ref)
        assert np.array_equal(got, want), f"step {step}: payload"
        if step == 0:
            assert np.array_equal(got, plain)
        check_worker(state, ref, f"step {step}")
        assert bits_equal(host(t.torch_tensor(), dt), x), "the gradient is read only"


@pytest.mark.parametrize("dt", [F32, BF16])
def test_codec_unaligned_gradient_view(bc, oracle_c, dt):
    """the gradient starts one element into its allocation: the guarded load path"""
    n_chunks, cs = 2, 3000
    n = n_chunks * cs
    rng = np.random.default_rng(77 + dt)
    state = bc.OneBitErrorFeedbackState(n, n_chunks, 0)
    ref = REF.WorkerState(n, n_chunks)
    for step in range(4):
        x = grads(rng, n, dt)
        base = dev(np.concatenate([x[:1], x]), dt)
        view = base[1:]
        assert view.data_ptr() % 16 != 0
        got = bc.BaguaTensorPy(view, "g").compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        assert np.array_equal(got, REF.compress_ef(oracle_c, x, dt, n_chunks, ref)), step
        check_worker(state, ref, f"step {step}")


def test_codec_signed_zeros_and_a_zero_chunk(bc, oracle_c):
    n_chunks, cs = 3, 2048 + 7
    n = n_chunks * cs
    rng = np.random.default_rng(9)
    state = bc.OneBitErrorFeedbackState(n, n_chunks, 0)
    ref = REF.WorkerState(n, n_chunks)
    for step in range(4):
        x = grads(rng, n, F32)
        x[::5] = 0.0
        x[1::5] = -0.0
        x[cs:2 * cs] = 0.0 if step % 2 == 0 else -0.0  # chunk 1 all zero: scale 0
        got = bc.BaguaTensorPy(dev(x, F32), "g").compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        assert np.array_equal(got, REF.compress_ef(oracle_c, x, F32, n_chunks, ref)), step
        check_worker(state, ref, f"step {step}")


# ---- range form --------------------------------------------------------------
@pytest.mark.parametrize("pieces", [3, 4])  # 5 tiles per chunk: [0,2) [2,4) [4,5), and with 4 an empty [5,5)
@pytest.mark.parametrize("dt", [F32, F16])
def test_range_form_equals_whole_call(bc, dt, pieces):
    N = bc._native
    n_chunks, cs = 4, 5000
    n = n_chunks * cs
    rng = np.random.default_rng(31 + dt)
    S = N.K.bagua_onebit_compressed_bytes(cs, n_chunks)
    wsb = N.K.bagua_onebit_workspace_bytes(cs, n_chunks)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    whole = bc.OneBitErrorFeedbackState(n, n_chunks, 0)
    pieced = bc.OneBitErrorFeedbackState(n, n_chunks, 0)
    for step in range(2):
        g = dev(grads(rng, n, dt), dt)
        want = bc.BaguaTensorPy(g, "g").compress_with_error_feedback(n_chunks, whole).to_numpy_u8()
        out = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        seen = []
        for q in range(pieces):
            tb, te = ctypes.c_int(), ctypes.c_int()
            N.check(N.K.bagua_onebit_piece_range(cs, pieces, q, ctypes.byref(tb), ctypes.byref(te)), "range")
            seen.append((tb.value, te.value))
            N.check(N.K.bagua_onebit_encode_range_ef(dt, g.data_ptr(), n, cs, n_chunks, out.data_ptr(), S, ws.data_ptr(),
                                                     wsb, tb.value, te.value, pieced.worker_carry.data_ptr(),
                                                     pieced.worker_scales.data_ptr(), None), "encode range")
        assert seen[:3] == [(0, 2), (2, 4), (4, 5)] and (pieces == 3 or seen[3] == (5, 5))
        N.check(N.K.bagua_onebit_finalize_ef(ws.data_ptr(), wsb, n, cs, n_chunks, out.data_ptr(), S,
                                             pieced.worker_scales.data_ptr(), None), "finalize")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), step
        assert bits_equal(f32_host(pieced.worker_carry), f32_host(whole.worker_carry)), step
        assert bits_equal(f32_host(pieced.worker_scales), f32_host(whole.worker_scales)), step


# ---- the op on the loopback transport ------------------------------------------
def _state_raws(N, st):
    return [st._raw(t) for t in st.tensors()]


def _run_op_steps(bc, oracle_c, p, dt, cs, pieces, average, steps=3):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    n = p * cs
    rng = np.random.default_rng(p * 1000 + dt * 10 + cs)
    comms = loopback_communicators(p, 0)
    states = [bc.OneBitErrorFeedbackState(n, p, 0) for _ in range(p)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    for step in range(steps):
        xs = [grads(rng, n, dt, r) for r in range(p)]
        want, _ = REF.centralized_step(oracle_c, xs, dt, refs, bool(average))
        ts = [dev(x, dt) for x in xs]
        torch.cuda.synchronize()

        def rank(r):
            raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
            sr = _state_raws(N, states[r])
            N.check(N.C.bagua_centralized_onebit_error_feedback(comms[r].handle, ctypes.byref(raw), average,
                                                                *[ctypes.byref(s) for s in sr], pieces), f"rank {r}")

        run_ranks(rank, p)
        outs = [host(t, dt) for t in ts]
        for r in range(p):
            assert bits_equal(outs[r], want[r]), f"step {step} rank {r}: result"
            assert bits_equal(outs[r], outs[0]), f"step {step}: rank {r} differs from rank 0"
            for name, got in zip(("wc", "ws", "sc", "ss"), states[r].tensors()):
                assert bits_equal(f32_host(got), getattr(refs[r], name)), f"step {step} rank {r}: {name}"


@pytest.mark.parametrize("p,dt,cs", [(1, F32, 70000), (2, F32, 40000), (3, F32, 3072), (4, F16, 8192),
                                     (8, BF16, 20000), (16, F32, 4096)])
def test_op_matches_reference(bc, oracle_c, p, dt, cs):
    _run_op_steps(bc, oracle_c, p, dt, cs, 0, 1)


@pytest.mark.parametrize("pieces", [1, 3, 0])
@pytest.mark.parametrize("p,dt,cs", [(2, F32, 40000), (8, BF16, 20000)])
def test_op_piece_counts(bc, oracle_c, p, dt, cs, pieces):
    _run_op_steps(bc, oracle_c, p, dt, cs, pieces, 1)


def test_op_sum(bc, oracle_c):
    _run_op_steps(bc, oracle_c, 4, F32, 5000, 2, 0)


def test_op_more_ranks_than_the_fused_middle_step(bc, oracle_c):
    """17 chunks: the middle step composed from decode + reduce + the worker encode"""
    _run_op_steps(bc, oracle_c, 17, F32, 1536, 0, 1, steps=2)


def test_op_misaligned_gradient_on_one_rank(bc, oracle_c):
    """rank 1's gradient is offset by one element (the aligned-copy route) and the piece
    count is automatic: both ranks build the same piece ranges"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    p, cs, dt = 2, 40000, F32
    n = p * cs
    rng = np.random.default_rng(4242)
    comms = loopback_communicators(p, 0)
    states = [bc.OneBitErrorFeedbackState(n, p, 0) for _ in range(p)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    for step in range(2):
        xs = [grads(rng, n, dt, r) for r in range(p)]
        want, _ = REF.centralized_step(oracle_c, xs, dt, refs, True)
        ts = [dev(xs[0], dt), dev(np.concatenate([xs[1][:1], xs[1]]), dt)[1:]]
        assert ts[1].data_ptr() % 16
        torch.cuda.synchronize()

        def rank(r):
            raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
            sr = _state_raws(N, states[r])
            N.check(N.C.bagua_centralized_onebit_error_feedback(comms[r].handle, ctypes.byref(raw), 1,
                                                                *[ctypes.byref(s) for s in sr], 0), f"rank {r}")

        run_ranks(rank, p)
        for r in range(p):
            assert bits_equal(host(ts[r], dt), want[r]), (step, r)
            assert bits_equal(f32_host(states[r].worker_carry), refs[r].wc), (step, r)


# ---- bucket path -----------------------------------------------------------------
def test_bucket_path_scattered(bc, oracle_c):
    from bagua_core.bucket import CentralizedOneBitErrorFeedback
    from bagua_core.communicator import loopback_communicators
    p, dt = 2, F32
    sizes = [3000, 5192]
    n = sum(sizes)
    cs = n // p
    rng = np.random.default_rng(606)
    comms = loopback_communicators(p, 0)
    steps_x = [[grads(rng, n, dt, r) for r in range(p)] for _ in range(2)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    wants = [REF.centralized_step(oracle_c, xs, dt, refs, True)[0] for xs in steps_x]
    parts, gaps, states, buckets = [], [], [], []
    for r in range(p):
        a = torch.zeros(sizes[0], device="cuda")
        gaps.append(torch.empty(4096, device="cuda"))  # keeps the two tensors apart
        b = torch.zeros(sizes[1], device="cuda")
        parts.append([a, b])
        bk = bc.BaguaBucketPy(f"ef{r}", [bc.BaguaTensorPy(a, f"r{r}.a"), bc.BaguaTensorPy(b, f"r{r}.b")])
        st = bc.OneBitErrorFeedbackState(n, p, 0)
        bk.append_centralized_synchronous_op(comms[r], None, hierarchical=False, average=True,
                                             compression="OneBitSignScale", error_feedback=st)
        ops = bk.ops()
        assert len(ops) == 1 and isinstance(ops[0], CentralizedOneBitErrorFeedback) and ops[0].state is st
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
            assert bits_equal(outs[r], wants[step][r]), (step, r)
    for r in range(p):
        assert bits_equal(f32_host(states[r].worker_carry), refs[r].wc) and bits_equal(f32_host(states[r].server_carry),
                                                                                      refs[r].sc)
        states[r].zero_()
    again = run_step(steps_x[0])
    for r in range(p):
        assert bits_equal(again[r], first[r]), f"rank {r}: zeroed state must reproduce step 1"


# ---- refusals: nothing is launched ----------------------------------------------------
def test_python_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    comm = loopback_communicators(1, 0)[0]
    g = torch.ones(4096, device="cuda")
    bk = bc.BaguaBucketPy("refuse", [bc.BaguaTensorPy(g, "refuse.g")])
    st = bc.OneBitErrorFeedbackState(4096, 1, 0)
    with pytest.raises(NotImplementedError, match="OneBitSignScale"):
        bk.append_centralized_synchronous_op(comm, None, compression="MinMaxUInt8", error_feedback=st)
    with pytest.raises(NotImplementedError, match="OneBitSignScale"):
        bk.append_centralized_synchronous_op(comm, None, compression=None, error_feedback=st)
    with pytest.raises(NotImplementedError, match="hierarchical"):
        bk.append_centralized_synchronous_op(comm, comm, hierarchical=True, compression="OneBitSignScale",
                                             error_feedback=st)
    with pytest.raises(RuntimeError, match="does not fit"):
        bk.append_centralized_synchronous_op(comm, None, compression="OneBitSignScale",
                                             error_feedback=bc.OneBitErrorFeedbackState(2048, 1, 0))
    assert bk.ops() == []
    bk.append_centralized_synchronous_op(comm, None, compression="OneBitSignScale", error_feedback=st)
    other = bc.BaguaBucketPy("refuse2", [bc.BaguaTensorPy(torch.ones(4096, device="cuda"), "refuse2.g")])
    with pytest.raises(RuntimeError, match="one state, one op"):
        other.append_centralized_synchronous_op(comm, None, compression="OneBitSignScale", error_feedback=st)
    assert len(bk.ops()) == 1 and other.ops() == []
    torch.cuda.synchronize()
    assert float(g.sum()) == 4096.0 and all(float(t.abs().sum()) == 0.0 for t in st.tensors())


def test_native_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comm = loopback_communicators(1, 0)[0]
    n = 4096
    g = torch.ones(n, device="cuda")
    st = bc.OneBitErrorFeedbackState(n, 1, 0)
    op = N.C.bagua_centralized_onebit_error_feedback

    def call(raw, sr, pieces=0):
        return op(comm.handle, ctypes.byref(raw), 1, *[ctypes.byref(s) for s in sr], pieces)

    raw = bc.BaguaTensorPy(g, "g").raw()
    good = _state_raws(N, st)
    small = _state_raws(N, bc.OneBitErrorFeedbackState(n // 2, 1, 0))
    for i in range(4):  # each state tensor in turn: wrong size, wrong dtype, wrong device, misaligned
        for field, value in (("num_elem", None), ("dtype", N.DTYPE_F16), ("device_id", 1)):
            sr = _state_raws(N, st)
            if value is None:
                # a state built for half the elements; the scales of one rank have no smaller size: two
                sr[i] = small[i] if i in (0, 2) else N.bagua_tensor_t(good[i].ptr, 2, 2, N.DTYPE_F32, 0)
            else:
                setattr(sr[i], field, value)
            assert call(raw, sr) == ERR_INVALID_ARG, (i, field)
        sr = _state_raws(N, st)
        sr[i].ptr += 4
        assert call(raw, sr) == ERR_INVALID_ARG, (i, "alignment")
    partly = N.bagua_tensor_t(raw.ptr, n - 8, n, raw.dtype, raw.device_id)
    assert call(partly, good) == ERR_UNSUPPORTED
    ints = N.bagua_tensor_t(raw.ptr, n, n, N.DTYPE_I64, raw.device_id)
    assert call(ints, good) == ERR_UNSUPPORTED
    assert call(raw, good, pieces=1 << 21) == ERR_INVALID_ARG  # unknown schedule bit
    torch.cuda.synchronize()
    assert float(g.sum()) == float(n) and all(float(t.abs().sum()) == 0.0 for t in st.tensors())
    # the native bucket refuses the op in hierarchical mode and with another codec
    bk = bc.BaguaBucketPy("native_refuse", [bc.BaguaTensorPy(g, "native_refuse.g")])
    nop = N.bagua_bucket_op_t(kind=N.BUCKET_OP_CENTRALIZED_ONEBIT_ERROR_FEEDBACK, average=1,
                              compression=N.COMPRESSION_ONEBIT, fused=1, comm=comm.handle.value,
                              intranode=comm.handle.value, ef_worker_carry=good[0], ef_worker_scales=good[1],
                              ef_server_carry=good[2], ef_server_scale=good[3])
    assert N.C.bagua_bucket_append_op(bk.handle, ctypes.byref(nop)) == ERR_UNSUPPORTED
    nop.intranode = None
    nop.compression = N.COMPRESSION_MINMAX_UINT8
    assert N.C.bagua_bucket_append_op(bk.handle, ctypes.byref(nop)) == ERR_UNSUPPORTED
    nop.compression = N.COMPRESSION_ONEBIT
    nop.ef_server_scale = N.bagua_tensor_t()
    assert N.C.bagua_bucket_append_op(bk.handle, ctypes.byref(nop)) == ERR_INVALID_ARG
    assert N.C.bagua_bucket_num_ops(bk.handle) == 0


def test_ranks_disagreeing_on_error_feedback(bc, monkeypatch):
    """rank 0 runs the op with error feedback, rank 1 the plain 1-bit op: with the schedule
    check on, both get BAGUA_ERR_INVALID_ARG before any byte is exchanged"""
    monkeypatch.setenv("BAGUA_CHECK_SCHEDULE", "1")
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    p, cs = 2, 40000
    n = p * cs
    rng = np.random.default_rng(8)
    xs = [grads(rng, n, F32, r) for r in range(p)]
    comms = loopback_communicators(p, 0)
    ts = [dev(x, F32) for x in xs]
    st = bc.OneBitErrorFeedbackState(n, p, 0)
    torch.cuda.synchronize()
    rcs = [None] * p

    def rank(r):
        raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
        if r == 0:
            rcs[r] = N.C.bagua_centralized_onebit_error_feedback(comms[r].handle, ctypes.byref(raw), 1,
                                                                 *[ctypes.byref(s) for s in _state_raws(N, st)], 0)
        else:
            rcs[r] = N.C.bagua_centralized_low_precision_pipelined(comms[r].handle, ctypes.byref(raw), 1,
                                                                   N.COMPRESSION_ONEBIT, 0)

    run_ranks(rank, p)
    assert rcs == [ERR_INVALID_ARG] * p, rcs
    for r in range(p):
        assert bits_equal(host(ts[r], F32), xs[r]), f"rank {r} changed"
    assert all(float(t.abs().sum()) == 0.0 for t in st.tensors())
