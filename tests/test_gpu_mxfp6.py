"""GPU tests of the MXFP6 codec (MXFP6.md): kernels, C ABI, runtime dispatch, the fused middle
step, the block-range entries, the ops and the Python surface, byte for byte against the numpy
reference (tests/mxfp6_reference.py).  Compressed bytes, slack included, and decoded tensors are
compared exactly; a reduced tensor that may hold NaN as the project's other tests do.

Launch geometry of csrc/kernels/mxfp6.hip, from which the sizes below follow: an encode and a
decode lane own 16-B vectors of T (4 f32 / 8 16-bit elements) and work in groups of four lanes
(16 / 32 elements, 12 / 24 payload bytes); an encode wave covers 8 KiB of input per iteration
(2048 / 4096 elements) and a workgroup of four waves 8192 / 16384; a decode workgroup covers
4096 / 8192 elements per iteration; a middle-step lane owns one block of 32 and its workgroup
8192 elements.  BAGUA_TUNE_MX6_*_BLOCKS=2 caps the grid at two workgroups, which puts the start
of the second grid-stride iteration at twice what one workgroup covers.  One, two, three and four
blocks leave 8, 16, 24 and 0 bytes of payload slack."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp6_reference as R
from oracle import oracle_np as NP
from test_gpu_codec import assert_float_bits_equal
from test_gpu_multirank import dev, host
from test_gpu_mxfp8 import (BF16, DTYPES, F16, F32, FILL, TORCH, bc, dev_at, grads, hostile_inputs,  # noqa: F401
                            run_centralized, same_bytes, u8)
from test_gpu_mxfp8_op import default_schedule_env  # noqa: F401  (autouse: no schedule knob inherited)
from test_mxfp6_cpu import code_table, tie_table

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
GRID_KNOBS = ("BAGUA_TUNE_MX6_ENCODE_BLOCKS", "BAGUA_TUNE_MX6_DECODE_BLOCKS", "BAGUA_TUNE_MX6_MIDDLE_BLOCKS")
# 1; one below, at and one above every edge of the geometry above, for both element sizes
SIZES = [1] + [s + d for s in (4, 8, 32, 64, 96, 128, 2048, 4096, 8192, 16384, 32768) for d in (-1, 0, 1)]


@pytest.fixture
def composed(monkeypatch):
    """mxfp8_reference's middle step and composed ops (decompress + reduce + compress) over this codec's reference"""
    import mxfp8_reference as M8
    monkeypatch.setattr(M8, "compress", R.compress)
    monkeypatch.setattr(M8, "decompress", R.decompress)
    return M8


def roundtrip(bc, x, dtype, p, what, offset=0):
    """compress + decompress_from through BaguaTensorPy against the reference; returns the reference's bytes"""
    comp = bc.BaguaTensorPy(dev_at(x, dtype, offset), "x").compress("MXFP6", p, -1)
    want = R.compress(x, dtype, p)
    assert comp.num_elements() == R.compressed_bytes(x.size // p, p)
    same_bytes(comp.to_numpy_u8(), want, f"{what}: compressed")
    out = dev_at(np.zeros_like(x), dtype, offset)
    out.fill_(7.0)
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP6", p, comp)
    same_bytes(host(out, dtype), R.decompress(want, p, np.zeros_like(x), dtype), f"{what}: decoded")
    return want


def middle(bc, M, recv, p, cs, dtype, target, average, what, store=True, offset=0):
    """bagua_mxfp6_reduce_requantize against the reference's decompress + reduce + compress"""
    S = recv.size
    want_buf, want_t = M.reduce_requantize(recv, p, cs, dtype, target, bool(average), out=np.full(S, FILL, np.uint8))
    rt = torch.from_numpy(recv).cuda()
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    tensor = dev_at(NP.from_f32(np.full(p * cs, 5.0, np.float32), dtype), dtype, offset)
    rc = bc._native.K.bagua_mxfp6_reduce_requantize(dtype, rt.data_ptr(), S, cs, p, tensor.data_ptr() if store else None,
                                                    average, out.data_ptr(), S, target, None)
    assert rc == OK, what
    same_bytes(u8(out), want_buf, what)
    got = host(tensor, dtype)
    keep = np.ones(p * cs, bool)
    if store:
        keep[target * cs:(target + 1) * cs] = False
        assert_float_bits_equal(got[~keep], want_t[~keep], dtype, what)
    assert (NP.to_f32(got, dtype)[keep] == 5.0).all(), f"{what}: written outside the own chunk"


@pytest.mark.parametrize("two_workgroups", [False, True])
@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_codec_sizes(bc, dtype, n_chunks, two_workgroups, monkeypatch):
    if two_workgroups:
        for k in GRID_KNOBS:
            monkeypatch.setenv(k, str(2 * n_chunks))  # the cap is shared by the chunks: two workgroups each
    rng = np.random.default_rng(1000 * dtype + 10 * n_chunks + two_workgroups)
    for cs in SIZES:
        roundtrip(bc, grads(rng, n_chunks * cs, dtype), dtype, n_chunks, f"cs={cs} p={n_chunks}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_both_tables(bc, composed, dtype, offset):
    """every code at every position and every tie, through the encode, the decode and the middle step at
    p = 1, on the vector path and on the guarded one (a view one element into its allocation)"""
    x1, scale, codes = code_table(dtype)
    x = NP.from_f32(np.concatenate([x1, tie_table(dtype)[0]]).astype(np.float32).ravel(), dtype)
    comp = roundtrip(bc, x, dtype, 1, f"tables offset={offset}", offset)
    sb = R.scale_bytes(x.size)
    assert np.array_equal(comp[:64], scale) and np.array_equal(R.unpack(comp[sb:sb + 24 * 64]), codes)
    middle(bc, composed, comp, 1, x.size, dtype, 0, 0, f"tables middle step offset={offset}", offset=offset)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_of_every_scale_byte_and_code(bc, dtype):
    """block 2 b + h holds scale byte b and the codes (b + j + 32 h) mod 64: all 256 x 64 pairs, 0xFF included"""
    scales = np.repeat(np.arange(256, dtype=np.uint8), 2)
    codes = (scales[:, None] + np.arange(32)[None, :] + 32 * (np.arange(512) % 2)[:, None]) % 64
    cs = 32 * 512 - 5  # ragged: the last block decodes 27 elements
    buf = np.zeros(R.compressed_bytes(cs, 1), np.uint8)
    buf[:512] = scales
    buf[R.scale_bytes(cs):R.scale_bytes(cs) + 24 * 512] = R.pack(codes).ravel()
    out = torch.zeros(cs, dtype=TORCH[dtype], device="cuda")
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP6", 1, bc.BaguaTensorPy(torch.from_numpy(buf).cuda(), "bytes"))
    want = R.decompress(buf, 1, np.zeros(cs, R.STORAGE[dtype]), dtype)
    same_bytes(host(out, dtype), want, "decode")
    wf = NP.to_f32(want, dtype)
    assert np.isnan(wf[-59:]).all() and not np.isnan(wf[:-59]).any() and np.nanmax(np.abs(wf)) == R.MAX_FINITE[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_inputs_partial_tensor_and_single_target(bc, dtype):
    N, K = bc._native, bc._native.K
    cases, p = hostile_inputs(dtype)  # NaN, +-Inf, largest finite, -0, denormal, all zero, one element 2^40 above
    for name, x in cases.items():
        roundtrip(bc, x, dtype, p, name)
    # a partly valid tensor: elements at or past num_elem count as +0, however large they are
    rng = np.random.default_rng(9 + dtype)
    p, cs = 3, 1000
    for num_elem in (cs + 517, 2 * cs + 31, 5, 0):
        x = grads(rng, p * cs, dtype)
        x[num_elem:num_elem + 40] = NP.from_f32(np.full(40, 6e4, np.float32), dtype)[:x[num_elem:num_elem + 40].size]
        xt = dev(x, dtype)
        raw = bc.BaguaTensorPy(xt, "x").raw()
        raw.num_elem = num_elem
        out = N.bagua_tensor_t()
        N.check(N.C.bagua_tensor_compress(ctypes.byref(raw), N.COMPRESSION_MXFP6, p, 0, -1, ctypes.byref(out)), "compress")
        got = bc.BaguaTensorPy._from_raw(out, "c", owned=True).to_numpy_u8()
        same_bytes(got, R.compress(x, dtype, p, num_elem=num_elem), f"num_elem={num_elem}")
    # target_chunk >= 0 leaves the other segments' bytes untouched
    x = grads(rng, 4 * cs, dtype)
    xt, S = dev(x, dtype), R.compressed_bytes(cs, 4)
    for target in (0, 3):
        out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        assert K.bagua_mxfp6_compress(dtype, xt.data_ptr(), x.size, cs, 4, out.data_ptr(), S, target, None) == OK
        same_bytes(u8(out), R.compress(x, dtype, 4, target, out=np.full(S, FILL, np.uint8)), f"target {target}")


def received(rng, p, cs, dtype):
    """p segments as the alltoall delivers them; segment 0 holds a NaN block, and on f16 the sum overflows"""
    x = NP.to_f32(grads(rng, p * cs, dtype, scale=3e4 if dtype == F16 else 1e-3), dtype).copy()
    if dtype == F16:
        for c in range(p):
            x[c * cs + cs // 2:c * cs + cs // 2 + 8] = 60000.0
    x[37] = np.nan
    with np.errstate(over="ignore", invalid="ignore"):
        return R.compress(NP.from_f32(x, dtype), dtype, p)


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 9, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_requantize(bc, composed, dtype, p, monkeypatch):
    """every BY (2 up to p = 4, 4 up to 8, 8 up to 16) on both sides of each boundary, with a full and a
    partly filled second round of the summation tree; sum and average; storing the reduced chunk and not"""
    monkeypatch.setenv("BAGUA_TUNE_MX6_MIDDLE_BLOCKS", "2")  # the larger cs spans two grid-stride iterations
    rng = np.random.default_rng(100 * dtype + p)
    for cs in (1000, 2 * 8192 + 33) if p in (2, 5, 9) else (1000,):
        recv = received(rng, p, cs, dtype)
        for average in (0, 1):
            for store in (False, True):
                middle(bc, composed, recv, p, cs, dtype, p // 2, average,
                       f"p={p} cs={cs} average={average} store={store}", store)


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_entries_reproduce_the_whole_chunk_bytes(bc, composed, dtype):
    """1, 2, 3 and 8 pieces of a chunk of more than two granules with a ragged last block: encode, decode and
    middle step range by range (last piece first) give the whole-chunk entries' bytes"""
    K = bc._native.K
    p, cs = 2, 3 * 4096 + 33
    rng = np.random.default_rng(8000 + dtype)
    x = grads(rng, p * cs, dtype)
    xt = dev(x, dtype)
    comp = R.compress(x, dtype, p)
    S = comp.size
    dec = R.decompress(comp, p, np.zeros(p * cs, R.STORAGE[dtype]), dtype)
    recv = received(rng, p, cs, dtype)
    rt, ct = torch.from_numpy(recv).cuda(), torch.from_numpy(comp).cuda()
    mid, _ = composed.reduce_requantize(recv, p, cs, dtype, 1, True, out=np.full(S, FILL, np.uint8))
    for pieces in (1, 2, 3, 8):
        enc = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        out = torch.full((p * cs,), 7.0, dtype=TORCH[dtype], device="cuda")
        mo = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        b, e = ctypes.c_int(), ctypes.c_int()
        for q in reversed(range(pieces)):
            assert K.bagua_mxfp6_piece_range(cs, pieces, q, ctypes.byref(b), ctypes.byref(e)) == OK
            bb, be = b.value, e.value
            assert (bb, be) == R.piece_range(cs, pieces, q)
            if bb == be:
                continue  # the op skips empty pieces
            assert K.bagua_mxfp6_compress_range(dtype, xt.data_ptr(), x.size, cs, p, enc.data_ptr(), S, bb, be, None) == OK
            assert K.bagua_mxfp6_decompress_range(dtype, ct.data_ptr(), S, cs, p, out.data_ptr(), bb, be, None) == OK
            assert K.bagua_mxfp6_reduce_requantize_range(dtype, rt.data_ptr(), S, cs, p, 1, mo.data_ptr(), S, 1, bb, be,
                                                         None) == OK
        same_bytes(u8(enc), comp, f"pieces={pieces}: encode")
        same_bytes(host(out, dtype), dec, f"pieces={pieces}: decode")
        same_bytes(u8(mo), mid, f"pieces={pieces}: middle step")


@pytest.mark.parametrize("pieces", [0, 1, 3])
@pytest.mark.parametrize("p", [1, 2])
def test_centralized_op(bc, composed, p, pieces):
    """the pipelined entry (0: the op's own piece count) equals the reference's composed op; the kernel names
    of rank 0 show the fused middle step, once per filled piece"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comms = loopback_communicators(p, 0)
    cs = 4 * 4096 + 80   # four granules and a ragged block, whole 16-B vectors: the op can run pieced
    rng = np.random.default_rng(40 + p)
    op = N.C.bagua_centralized_low_precision_pipelined
    for dt in (F32, BF16):
        xs = [grads(rng, p * cs, dt) for _ in range(p)]
        ts = [dev(x, dt) for x in xs]
        names = run_centralized(bc, comms, lambda c, raw, av, _m: op(c, raw, av, N.COMPRESSION_MXFP6, pieces), ts, 1,
                                timed=True)  # rank 0's kernel names, through KernelNames
        k = names.count("mxfp6_reduce_encode_kernel")
        assert k >= 1 and "reduce_chunks_kernel" not in names, names
        assert names.count("mxfp6_encode_kernel") == k == names.count("mxfp6_decode_kernel"), names
        if pieces == 3 and p == 2:
            assert k == 3, names
        want = composed.centralized(xs, dt, True)
        for r in range(p):
            same_bytes(host(ts[r], dt), want[r], f"p={p} dtype={dt} pieces={pieces} rank {r}")


@pytest.mark.parametrize("dtype", [F32, F16])
def test_ring_op_and_bucket_ops_by_name(bc, composed, dtype):
    """the decentralized op at one rank runs the composed elementwise sequence with this codec; the
    centralized bucket op takes the name; error feedback and stochastic rounding do not exist for it"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comm = loopback_communicators(1, 0)[0]
    n = 3000 + 17
    rng = np.random.default_rng(60 + dtype)
    data = [grads(rng, n, dtype) for _ in range(4)]  # t, weight, left, right
    devs = [dev(a, dtype) for a in data]
    ts = [bc.BaguaTensorPy(d, f"t{k}") for k, d in enumerate(devs)]
    bk = bc.BaguaBucketPy("ring", [ts[0]])
    bk.append_low_precision_decentralized_synchronous_op(comm, None, hierarchical=False, peer_selection_mode="ring",
                                                         compression="MXFP6", weight=ts[1], left_peer_weight=ts[2],
                                                         right_peer_weight=ts[3])
    raws = [t.raw() for t in ts]
    torch.cuda.synchronize()
    N.check(N.C.bagua_decentralized_low_precision_synchronous(comm.handle, *[ctypes.byref(x) for x in raws],
                                                              N.COMPRESSION_MXFP6), "ring op")
    for k, want in enumerate(composed.decentralized(*[[a] for a in data], dtype)):
        same_bytes(host(devs[k], dtype), want[0], f"ring op tensor {k}")
    bk2 = bc.BaguaBucketPy("central", [ts[0]])
    bk2.append_centralized_synchronous_op(comm, None, hierarchical=False, average=True, compression="MXFP6")
    with pytest.raises(NotImplementedError):
        bk2.append_centralized_synchronous_op(comm, None, compression="MXFP6",
                                              error_feedback=bc.MXFP8ErrorFeedbackState(n, 1, 0))
    with pytest.raises(NotImplementedError):
        bk2.append_centralized_synchronous_op(comm, None, compression="MXFP6",
                                              stochastic_rounding=bc.MXFP8StochasticRounding(7))
    assert len(bk2.ops()) == 1 and bc.METHODS["MXFP6"] == N.COMPRESSION_MXFP6 == 5


def test_refusals(bc):
    K = bc._native.K
    cs, p = 128 * 32 * 3 + 40, 2   # nb = 386
    S, S17 = R.compressed_bytes(cs, p), R.compressed_bytes(64, 17)
    x = torch.zeros(cs * p, device="cuda")
    buf, out = (torch.full((max(S, S17) + 16,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
    xp, bp, op = x.data_ptr(), buf.data_ptr(), out.data_ptr()
    # short and misaligned buffers, a target past the chunks, a dtype that is no codec dtype
    for o, size, target in ((op, S - 1, -1), (op + 4, S, -1), (op, S, p)):
        assert K.bagua_mxfp6_compress(F32, xp, cs * p, cs, p, o, size, target, None) == INVALID_ARG
    assert K.bagua_mxfp6_compress(3, xp, cs * p, cs, p, op, S, -1, None) == UNSUPPORTED
    for b, size in ((bp, S - 1), (bp + 4, S)):
        assert K.bagua_mxfp6_decompress(F32, b, size, cs, p, xp, None) == INVALID_ARG
    for b, o, size in ((bp, op, S - 1), (bp + 8, op, S), (bp, op + 8, S)):
        assert K.bagua_mxfp6_reduce_requantize(F32, b, S, cs, p, None, 1, o, size, 0, None) == INVALID_ARG
    # ranges: begin not on the granule, end past nb, end before begin, negative begin, past the chunk
    for bb, be in ((64, 128), (0, 387), (256, 128), (-1, 128), (0, 100), (-1, -1), (386, 386 + 128), (512, 512)):
        assert K.bagua_mxfp6_compress_range(F32, xp, cs * p, cs, p, op, S, bb, be, None) == INVALID_ARG
        assert K.bagua_mxfp6_decompress_range(F32, bp, S, cs, p, xp, bb, be, None) == INVALID_ARG
        assert K.bagua_mxfp6_reduce_requantize_range(F32, bp, S, cs, p, 1, op, S, 0, bb, be, None) == INVALID_ARG
    # more segments than the fused middle step takes
    assert K.bagua_mxfp6_reduce_requantize(F32, bp, S17, 64, 17, None, 1, op, S17, 0, None) == UNSUPPORTED
    assert (u8(out) == FILL).all() and not x.any()
