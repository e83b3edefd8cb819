"""GPU tests of the MXFP4 codec's stochastic rounding (MXFP4.md, "Stochastic rounding"): the
stochastic forms of mxfp4_encode_kernel and mxfp4_reduce_encode_kernel, their C entries, the
runtime op on the loopback transport and over RCCL, the bucket op and the Python surface, byte
for byte against the numpy statement of the rule (tests/mxfp4_sr_reference.py).

Sizes follow the launch geometry described in tests/test_gpu_mxfp4.py: an encode wave covers
2048 f32 / 4096 16-bit elements, a piece boundary lies on a multiple of 128 blocks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mxfp4_boundary_cases as B
import mxfp4_reference as R
import mxfp4_sr_reference as SR
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_mxfp4 import (BF16, DTYPES, F16, F32, INVALID_ARG, OK, TORCH, UNSUPPORTED, dev_at, grads, received,
                            same_bytes, u8)
from test_gpu_op_edges import KernelNames

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
KEY = SR.key(0xB0A7, 3, 1, 0)
KERNELS = ("mxfp4_encode_kernel", "mxfp4_reduce_encode_kernel", "mxfp4_decode_kernel")
CS = [1, 31, 33, 3 * 2048 + 17, 8192, 128 * 32 * 2 + 163]


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("BAGUA_MXFP4_HWCVT", "BAGUA_TUNE_MX_ENCODE_BLOCKS", "BAGUA_TUNE_MX_MIDDLE_BLOCKS", "BAGUA_PIPELINE_TAPER",
              "BAGUA_PIPELINE_PIECES", "BAGUA_PIPELINE_MIN_PIECE", "BAGUA_CHECK_SCHEDULE"):
        monkeypatch.delenv(k, raising=False)


def encode(bc, xt, dtype, n, cs, p, key, target=-1, fill=None, num_elem=None):
    """bagua_mxfp4_compress_sr into a fresh buffer (prefilled with `fill` when given)"""
    S = R.compressed_bytes(cs, p)
    out = torch.full((S,), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
    rc = bc._native.K.bagua_mxfp4_compress_sr(dtype, xt.data_ptr(), n if num_elem is None else num_elem, cs, p,
                                              out.data_ptr(), S, target, key, None)
    assert rc == OK, rc
    return u8(out)


# ------------------------------------------------------------------ encode ----
@pytest.mark.parametrize("one_workgroup", [False, True])
@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_against_the_reference(bc, dtype, n_chunks, one_workgroup, monkeypatch):
    """every chunk; with three chunks of an odd size the chunks' bases are odd and misaligned
    (guarded loads, a pair of the hash straddling the lanes' vectors)"""
    if one_workgroup:
        monkeypatch.setenv("BAGUA_TUNE_MX_ENCODE_BLOCKS", "1")  # the grid-stride loop
    rng = np.random.default_rng(1000 * dtype + 10 * n_chunks + one_workgroup)
    for cs in CS:
        x = grads(rng, n_chunks * cs, dtype)
        got = encode(bc, dev(x, dtype), dtype, x.size, cs, n_chunks, KEY)
        same_bytes(got, SR.compress_sr(x, dtype, n_chunks, KEY), f"cs={cs} p={n_chunks}")
    plain = R.compress(x, dtype, n_chunks)
    nb, sb = R.blocks(cs), R.scale_bytes(cs)
    assert np.array_equal(got[:nb], plain[:nb]) and not np.array_equal(got[sb:], plain[sb:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_target_chunk_partly_valid_and_misaligned(bc, dtype):
    rng = np.random.default_rng(5 + dtype)
    for p, cs in ((4, 1000), (3, 1001)):
        x = grads(rng, p * cs, dtype)
        xt = dev(x, dtype)
        S = R.compressed_bytes(cs, p)
        for target in (0, p - 2, p - 1):  # the others' segments stay as they were
            got = encode(bc, xt, dtype, x.size, cs, p, KEY, target=target, fill=0xAB)
            same_bytes(got, SR.compress_sr(x, dtype, p, KEY, target, out=np.full(S, 0xAB, np.uint8)),
                       f"p={p} cs={cs} target {target}")
        huge = NP.from_f32(np.full(p * cs, 6e4, np.float32), dtype)
        for num_elem in (cs + 517, 2 * cs + 31, 5, 0):  # elements at or past num_elem count as +0
            y = x.copy()
            y[num_elem:num_elem + 40] = huge[num_elem:num_elem + 40]
            got = encode(bc, dev(y, dtype), dtype, y.size, cs, p, KEY, num_elem=num_elem)
            same_bytes(got, SR.compress_sr(y, dtype, p, KEY, num_elem=num_elem), f"p={p} cs={cs} num_elem={num_elem}")
    for cs, p in ((33, 1), (8193, 1), (1000, 3)):  # the tensor one element into its allocation
        x = grads(rng, p * cs, dtype)
        got = encode(bc, dev_at(x, dtype, 1), dtype, x.size, cs, p, KEY)
        same_bytes(got, SR.compress_sr(x, dtype, p, KEY), f"base[1:] cs={cs} p={p}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_surface(bc, dtype):
    rng = np.random.default_rng(21 + dtype)
    p, cs = 3, 2 * 4096 + 40
    x = grads(rng, p * cs, dtype)
    t = bc.BaguaTensorPy(dev(x, dtype), "x")
    rounding = bc.MXFP4StochasticRounding(0xFACE)
    comps = [t.compress_with_stochastic_rounding(p, rounding, step) for step in (0, 1, 0)]
    got = [c.to_numpy_u8() for c in comps]
    for step, g in zip((0, 1, 0), got):
        same_bytes(g, SR.compress_sr(x, dtype, p, SR.key(0xFACE, step, 0, 0)), f"step {step}")
    assert not np.array_equal(got[0], got[1])
    out = torch.zeros(p * cs, dtype=TORCH[dtype], device="cuda")
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP4", p, comps[1])  # the plain decoder
    same_bytes(host(out, dtype), R.decompress(got[1], p, np.zeros_like(x), dtype), "decoded")
    with pytest.raises(TypeError):
        t.compress_with_stochastic_rounding(p, 0xFACE, 0)
    with pytest.raises(RuntimeError):
        t.compress_with_stochastic_rounding(5, rounding, 0)


def piece_ranges(bc, cs, schedule):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & 0xFFFF):
        assert bc._native.K.bagua_mxfp4_piece_range(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == 0
        out.append((b.value, e.value))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_index_invariance_and_ranges(bc, dtype):
    """one tensor as 1 chunk, as 4 chunks and as range pieces: the same payload bytes; a range
    writes its own scale bytes and payload and nothing else"""
    K = bc._native.K
    rng = np.random.default_rng(77 + dtype)
    n, p = 4 * 3 * 4096, 4
    cs = n // p
    x = grads(rng, n, dtype)
    xt = dev(x, dtype)
    one = encode(bc, xt, dtype, n, n, 1, KEY)
    four = encode(bc, xt, dtype, n, cs, p, KEY)
    sb1, sb4, seg4 = R.scale_bytes(n), R.scale_bytes(cs), R.segment_bytes(cs)
    pay4 = np.concatenate([four[c * seg4 + sb4:(c + 1) * seg4] for c in range(p)])
    same_bytes(one[sb1:], pay4, "payload of 1 chunk against 4 chunks")
    same_bytes(one, SR.compress_sr(x, dtype, 1, KEY), "1 chunk")
    S = R.compressed_bytes(cs, p)
    for schedule in (3, 4 | TAPERED, 8):
        buf = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
        want = np.full(S, 0xAB, np.uint8)
        for b, e in piece_ranges(bc, cs, schedule):
            assert K.bagua_mxfp4_compress_sr_range(dtype, xt.data_ptr(), n, cs, p, buf.data_ptr(), S, b, e, KEY,
                                                   None) == OK
            for c in range(p):  # what this range owns of every segment, and nothing else
                want[c * seg4 + b:c * seg4 + e] = four[c * seg4 + b:c * seg4 + e]
                want[c * seg4 + sb4 + 16 * b:c * seg4 + sb4 + 16 * e] = four[c * seg4 + sb4 + 16 * b:
                                                                             c * seg4 + sb4 + 16 * e]
                if e == R.blocks(cs):
                    want[c * seg4 + e:c * seg4 + sb4] = 0
            same_bytes(u8(buf), want, f"schedule {schedule:#x} after range [{b}, {e})")
        same_bytes(u8(buf), four, f"schedule {schedule:#x} reassembled")


# ------------------------------------------------------------ middle step ----
def middle(bc, recv, dtype, cs, p, target, average, key, rng=None, fill=0xCD):
    K = bc._native.K
    S = recv.size
    rt = torch.from_numpy(recv).cuda()
    out = torch.full((S,), fill, dtype=torch.uint8, device="cuda")
    if rng is None:
        rc = K.bagua_mxfp4_reduce_requantize_sr(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(), S, target, key,
                                                None)
    else:
        rc = K.bagua_mxfp4_reduce_requantize_sr_range(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(), S,
                                                      target, rng[0], rng[1], key, None)
    assert rc == OK, rc
    return u8(out)


@pytest.mark.parametrize("p", list(range(1, 17)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step_fused_equals_composed(bc, dtype, p, monkeypatch):
    monkeypatch.setenv("BAGUA_TUNE_MX_MIDDLE_BLOCKS", "2")  # the larger cs spans two grid-stride iterations
    rng = np.random.default_rng(100 * dtype + p)
    for cs in (1001, 2 * 8192 + 33) if p in (1, 2, 8, 16) else (1001,):
        recv = received(rng, p, cs, dtype)
        target = p // 2  # odd cs: an odd target's chunk starts at an odd index
        for average in (0, 1):
            want, _ = SR.reduce_requantize_sr(recv, p, cs, dtype, target, bool(average), KEY,
                                              out=np.full(recv.size, 0xCD, np.uint8))
            same_bytes(middle(bc, recv, dtype, cs, p, target, average, KEY), want, f"p={p} cs={cs} average={average}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step_ranges(bc, dtype):
    rng = np.random.default_rng(300 + dtype)
    p, cs, target = 3, 3 * 4096 + 1192, 2
    recv = received(rng, p, cs, dtype)
    whole, _ = SR.reduce_requantize_sr(recv, p, cs, dtype, target, True, KEY, out=np.full(recv.size, 0xCD, np.uint8))
    seg, sb, nb = R.segment_bytes(cs), R.scale_bytes(cs), R.blocks(cs)
    for b, e in ((0, 128), (128, 384), (384, nb), (256, 256)):
        want = np.full(recv.size, 0xCD, np.uint8)
        o = target * seg
        want[o + b:o + e] = whole[o + b:o + e]
        want[o + sb + 16 * b:o + sb + 16 * e] = whole[o + sb + 16 * b:o + sb + 16 * e]
        if e == nb:
            want[o + e:o + seg] = whole[o + e:o + seg]
            want[o + sb:o + sb + 16 * b] = 0xCD
        same_bytes(middle(bc, recv, dtype, cs, p, target, 1, KEY, rng=(b, e)), want, f"range [{b}, {e})")


def test_middle_step_refuses_17_segments(bc):
    K = bc._native.K
    p, cs = 17, 64
    S = R.compressed_bytes(cs, p)
    buf = torch.zeros(S, dtype=torch.uint8, device="cuda")
    out = torch.zeros(S, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp4_reduce_requantize_sr(F32, buf.data_ptr(), S, cs, p, 1, out.data_ptr(), S, 0, KEY,
                                              None) == UNSUPPORTED
    assert K.bagua_mxfp4_reduce_requantize_sr_range(F32, buf.data_ptr(), S, cs, p, 1, out.data_ptr(), S, 0, 0, 2, KEY,
                                                    None) == UNSUPPORTED


# --------------------------------------------------------- boundary table ----
def boundary_cases(bc):
    """the boundary table through the stochastic encode and the middle-step tables through the
    stochastic middle step, each checked against the reference; name -> bytes"""
    out = {}
    for dtype in DTYPES:
        t = B.table(dtype)
        for p in (1, 3):
            for k in (KEY, 0, (1 << 64) - 1):
                got = encode(bc, dev_at(t.x, dtype), dtype, t.x.size, t.x.size // p, p, k)
                same_bytes(got, SR.compress_sr(t.x, dtype, p, k), f"table dtype={dtype} p={p} key={k:#x}")
                out[f"enc_{dtype}_{p}_{k:x}"] = got
        for kind, m in (("exact", B.middle_exact(dtype)),) + ((("near", B.middle_neighbours()),) if dtype == F32 else ()):
            for average in (0, 1):
                want, _ = SR.reduce_requantize_sr(m.recv, m.p, m.cs, dtype, 1, bool(average), KEY,
                                                  out=np.full(m.recv.size, 0xCD, np.uint8))
                got = middle(bc, m.recv, dtype, m.cs, m.p, 1, average, KEY)
                same_bytes(got, want, f"middle {kind} dtype={dtype} average={average}")
                out[f"mid_{kind}_{dtype}_{average}"] = got
    return out


def test_boundary_table_on_both_decode_paths(bc, tmp_path):
    """here with the hardware conversions decoding the received segments, and in a child process
    started with BAGUA_MXFP4_HWCVT=0 (the stochastic encode itself is arithmetic on both)"""
    path = str(tmp_path / "sw.npz")
    env = dict(os.environ, BAGUA_MXFP4_HWCVT="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "mxfp4_sr_child.py"), path], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.environ.get("BAGUA_MXFP4_HWCVT", "1") != "0"
    here = boundary_cases(bc)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(here)
        for k in here:
            same_bytes(z[k], here[k], k)


# -------------------------------------------------------------------- ops ----
def run_op(bc, comms, xs, dtype, average, pieces, seeds, steps, timed=False, num_elem=None, offsets=None):
    """bagua_centralized_mxfp4_stochastic on fresh device copies of xs; returns (every rank's result,
    rank 0's kernel names when timed)"""
    N = bc._native
    ts = [dev_at(x, dtype, offsets[r] if offsets else 0) for r, x in enumerate(xs)]
    names = []

    def rank(r):
        raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
        if num_elem is not None:
            raw.num_elem = num_elem
        call = lambda: N.C.bagua_centralized_mxfp4_stochastic(comms[r].handle, ctypes.byref(raw), average,  # noqa: E731
                                                              seeds[r], steps[r], pieces)
        if timed and r == 0:
            with KernelNames(N, comms[0]) as k:
                rc = call()
            names.extend(k.names)
        else:
            rc = call()
        N.check(rc, f"rank {r}")

    torch.cuda.synchronize()
    run_ranks(rank, len(ts))
    return [host(t, dtype).copy() for t in ts], names


def counts(names):
    return [names.count(k) for k in KERNELS]


@pytest.mark.parametrize("p", [1, 2, 3, 8, 17])
def test_op_on_loopback(bc, p):
    """pieces 1, 4 and 8 tapered: the same bytes, those of the CPU simulation; seeds and steps
    differ from rank to rank; the path from rank 0's kernel names"""
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    cs = 3 * 4096 + 1192 if p < 17 else 2 * 4096
    seeds, steps = [1000 + 7 * r for r in range(p)], [r % 3 for r in range(p)]
    rng = np.random.default_rng(40 + p)
    for dtype, average in ((F32, 1), (BF16, 0)):  # mean, and sum mode
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        want = SR.centralized_sr(xs, dtype, bool(average), seeds, steps)
        plain = R.centralized(xs, dtype, bool(average))
        assert not np.array_equal(want[0].view(np.uint8), plain[0].view(np.uint8))
        for pieces in (1, 4, 8 | TAPERED):
            got, names = run_op(bc, comms, xs, dtype, average, pieces, seeds, steps, timed=True)
            for r in range(p):
                same_bytes(got[r], want[r], f"p={p} dtype={dtype} average={average} pieces={pieces:#x} rank {r}")
            k = sum(e > b for b, e in piece_ranges(bc, cs, pieces)) if 1 < p <= 16 and pieces > 1 else 1
            if p <= 16:  # pieced with the fused middle step; one rank and one piece run unpieced
                assert counts(names) == [k, k, k] and "reduce_chunks_kernel" not in names, (pieces, names)
            else:        # composed: encode of all chunks and of the own one, decode of the received and of the gathered
                assert counts(names) == [2, 0, 2] and "reduce_chunks_kernel" in names, (pieces, names)


def test_op_misaligned_rank_and_partly_valid(bc):
    from bagua_core.communicator import loopback_communicators
    p, cs = 3, 3 * 4096 + 1192
    comms = loopback_communicators(p, 0)
    seeds, steps = [5] * p, [9] * p
    rng = np.random.default_rng(808)
    xs = [grads(rng, p * cs, F16) for _ in range(p)]
    got, names = run_op(bc, comms, xs, F16, 1, 3, seeds, steps, timed=True, offsets=[0, 1, 0])
    k = sum(e > b for b, e in piece_ranges(bc, cs, 3))
    assert k > 1 and counts(names) == [k, k, k], names  # rank 0's launches: the pieced schedule
    want = SR.centralized_sr(xs, F16, True, seeds, steps)
    for r in range(p):
        same_bytes(got[r], want[r], f"misaligned rank 1: rank {r}")
    # a partly valid tensor (huge values past the last valid element): the composed steps
    num_elem = p * cs - cs // 2 - 3
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    for x in xs:
        x[num_elem:] = 3e38
    got, names = run_op(bc, comms, xs, F32, 1, 3, seeds, steps, timed=True, num_elem=num_elem)
    assert counts(names) == [2, 0, 2] and "reduce_chunks_kernel" in names, names
    want = SR.centralized_sr(xs, F32, True, seeds, steps, num_elem=num_elem)
    for r in range(p):
        same_bytes(got[r], want[r], f"partly valid rank {r}")


def test_bucket_through_the_scheduler(bc):
    """two executions use steps 0 and 1 and differ; a fresh op with the same seed reproduces both"""
    from bagua_core.communicator import loopback_communicators
    comm = loopback_communicators(1, 0)[0]
    n = 3 * 5000 + 8
    rng = np.random.default_rng(3)
    x = grads(rng, n, F32)
    want = [SR.centralized_sr([x], F32, True, 0xABCD, step)[0] for step in (0, 1)]
    assert not np.array_equal(want[0], want[1])
    seen = []
    for run in range(2):
        backend = bc.BaguaCommBackendPy(4, 0)
        t = torch.zeros(n, device="cuda")
        bt = bc.BaguaTensorPy(t, f"g{run}")
        bk = bc.BaguaBucketPy(f"mxfp4_sr_bucket{run}", [bt])
        bk.append_centralized_synchronous_op(comm, None, hierarchical=False, average=True, compression="MXFP4",
                                             stochastic_rounding=bc.MXFP4StochasticRounding(0xABCD))
        assert type(bk.ops()[0]).__name__ == "CentralizedMXFP4Stochastic"
        backend.register_ordered_buckets([bk])
        for step in (0, 1):
            t.copy_(torch.from_numpy(x))
            ev = torch.cuda.Event()
            ev.record()
            backend.mark_communication_ready(bt, ev.cuda_event)
            assert backend.wait_pending_comm_ops() == 1
            same_bytes(host(t, F32), want[step], f"op {run}, execution {step}")
            seen.append(host(t, F32).copy())
    assert np.array_equal(seen[0], seen[2]) and np.array_equal(seen[1], seen[3])


def test_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comm = loopback_communicators(1, 0)[0]
    n = 4096
    g = torch.ones(n, device="cuda")
    bt = bc.BaguaTensorPy(g, "sr_refuse.g")
    bk = bc.BaguaBucketPy("sr_refuse", [bt])
    rounding = bc.MXFP4StochasticRounding(1)
    for compression in ("MinMaxUInt8", "OneBitSignScale", None):
        with pytest.raises(NotImplementedError):
            bk.append_centralized_synchronous_op(comm, None, compression=compression, stochastic_rounding=rounding)
    with pytest.raises(NotImplementedError):
        bk.append_centralized_synchronous_op(comm, comm, hierarchical=True, compression="MXFP4",
                                             stochastic_rounding=rounding)
    with pytest.raises(NotImplementedError):
        bk.append_centralized_synchronous_op(comm, None, compression="MXFP4", stochastic_rounding=rounding,
                                             error_feedback=bc.MXFP4ErrorFeedbackState(n, 1, 0))
    with pytest.raises(TypeError):
        bk.append_centralized_synchronous_op(comm, None, compression="MXFP4", stochastic_rounding=1)
    assert N.C.bagua_bucket_num_ops(bk.handle) == 0
    # the native op
    op = N.C.bagua_centralized_mxfp4_stochastic
    raw = bt.raw()
    ints = N.bagua_tensor_t(raw.ptr, n, n, N.DTYPE_I64, raw.device_id)
    assert op(comm.handle, ctypes.byref(ints), 1, 1, 0, 1) == UNSUPPORTED
    assert op(comm.handle, ctypes.byref(raw), 1, 1, 0, -1) == INVALID_ARG
    assert op(None, ctypes.byref(raw), 1, 1, 0, 1) == INVALID_ARG
    assert op(comm.handle, None, 1, 1, 0, 1) == INVALID_ARG
    out = N.bagua_tensor_t()
    assert N.C.bagua_tensor_compress_mxfp4_stochastic(ctypes.byref(ints), 1, 0, 1, 0, ctypes.byref(out)) == UNSUPPORTED
    assert N.C.bagua_tensor_compress_mxfp4_stochastic(ctypes.byref(raw), 3, 0, 1, 0, ctypes.byref(out)) == INVALID_ARG
    torch.cuda.synchronize()
    assert float(g.sum()) == float(n)
    # the native bucket: hierarchical mode, another codec, error-feedback state beside the seed
    state = bc.MXFP4ErrorFeedbackState(n, 1, 0)

    def nop(**kw):
        args = dict(kind=N.BUCKET_OP_CENTRALIZED_MXFP4_STOCHASTIC, average=1, compression=N.COMPRESSION_MXFP4, fused=1,
                    comm=comm.handle.value, sr_seed=7)
        args.update(kw)
        return N.bagua_bucket_op_sr_t(**args)

    def append(o):
        return N.C.bagua_bucket_append_op(bk.handle, ctypes.byref(o))

    assert append(nop(intranode=comm.handle.value)) == UNSUPPORTED
    assert append(nop(compression=N.COMPRESSION_ONEBIT)) == UNSUPPORTED
    assert append(nop(compression=N.COMPRESSION_MINMAX_UINT8)) == UNSUPPORTED
    assert append(nop(ef_worker_carry=state._raw(state.worker_residual))) == INVALID_ARG
    assert append(nop(kind=8)) == UNSUPPORTED
    assert N.C.bagua_bucket_num_ops(bk.handle) == 0
    assert append(nop()) == OK and N.C.bagua_bucket_num_ops(bk.handle) == 1


# ------------------------------------------------------------------- RCCL ----
def test_op_over_rccl(tmp_path):
    """two processes, each its own communicator over RCCL's socket transport on the one GPU
    (set up as tests/test_gpu_mxfp4_pipelined_rccl.py): 3 pieces and one, against the simulation"""
    world, cs = 2, 5 * 4096
    rng = np.random.default_rng(1300)
    xs = [grads(rng, world * cs, F32) for _ in range(world)]
    seeds, steps = [0x51, 0x52], [4, 4]
    want = SR.centralized_sr(xs, F32, True, seeds, steps)
    np.savez(tmp_path / "inputs.npz", **{f"x{r}": x for r, x in enumerate(xs)})
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"NCCL_HOSTID": f"bagua-test-rank-{r}", "NCCL_SOCKET_IFNAME": "lo", "NCCL_IB_DISABLE": "1",
                    "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        log = open(tmp_path / f"rank{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "mxfp4_sr_rccl_worker.py"), str(r),
                                        str(world), str(tmp_path), "3,1", str(seeds[r]), str(steps[r])],
                                       stdout=log, stderr=subprocess.STDOUT, env=env, cwd=ROOT), log))
    failed = []
    for r, (p, log) in enumerate(procs):
        try:
            rc = p.wait(timeout=90)
        except subprocess.TimeoutExpired:
            for q, _ in procs:
                q.kill()
            rc = "timeout"
        log.close()
        if rc != 0:
            failed.append(r)
    if failed:
        tails = "\n".join(f"--- rank {r}:\n" + (tmp_path / f"rank{r}.log").read_text()[-1500:] for r in failed)
        pytest.fail(f"ranks {failed} failed:\n{tails}")
    for r in range(world):
        with np.load(tmp_path / f"out{r}.npz", allow_pickle=False) as z:
            for i, pieces in enumerate((3, 1)):
                assert np.array_equal(z[f"t{i}"], want[r].view(np.uint8)), f"rank {r}, pieces={pieces}"


# ------------------------------------------------------------- statistics ----
def test_mean_decode_is_unbiased(bc):
    """2^16 f32 elements, 256 steps of one seed: every element's mean decode is within
    5 * step / (2 sqrt(256)) of x, the bound of tests/test_mxfp4_sr_cpu.py::test_unbiased"""
    K = bc._native.K
    n, steps = 1 << 16, 256
    rng = np.random.default_rng(2025)
    x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    xt = dev(x, F32)
    S = R.compressed_bytes(n, 1)
    buf = torch.zeros(S, dtype=torch.uint8, device="cuda")
    dec = torch.zeros(n, device="cuda")
    acc = torch.zeros(n, dtype=torch.float64, device="cuda")
    for step in range(steps):
        assert K.bagua_mxfp4_compress_sr(F32, xt.data_ptr(), n, n, 1, buf.data_ptr(), S, -1, SR.key(77, step), None) == OK
        assert K.bagua_mxfp4_decompress(F32, buf.data_ptr(), S, n, 1, dec.data_ptr(), None) == OK
        acc += dec.double()
    torch.cuda.synchronize()
    mean = (acc / steps).cpu().numpy()
    x64 = x.astype(np.float64).reshape(-1, 32)
    scale, _ = R.encode_blocks(x64, F32)
    e = scale.astype(np.int64) - 127
    step_of = SR.floor_code_and_fraction(np.ldexp(np.abs(x64), -e[:, None]))[2] * np.ldexp(1.0, e)[:, None]
    bound = (5.0 * step_of / (2.0 * np.sqrt(steps))).ravel()
    err = np.abs(mean - x.astype(np.float64))
    print(f"worst element {(err / bound).max() * 5:.2f} step / (2 sqrt(K)), bound 5")
    assert (err <= bound).all()
    rne = R.decompress(R.compress(x, F32, 1), 1, np.zeros_like(x), F32).astype(np.float64)
    assert (np.abs(rne - x) > bound).mean() > 0.5  # round-to-nearest fails it
