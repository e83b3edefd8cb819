"""GPU tests of the MXFP8 codec (MXFP8.md): kernels, C ABI, runtime dispatch, the fused
middle step of the centralized op, the block-range entries and the Python surface, byte for
byte against the numpy reference (tests/mxfp8_reference.py).  Compressed bytes and decoded
tensors are compared exactly; a reduced tensor that may hold NaN is compared as the project's
other tests do, NaN at the same positions and every other value bit for bit.

Launch geometry of csrc/kernels/mxfp8.hip, from which the sizes below follow: an encode
and a decode lane own 16-B vectors of T (4 f32 / 8 16-bit elements); an encode wave covers
8 KiB of input per iteration (2048 / 4096 elements) and a workgroup of four waves 8192 /
16384; a decode workgroup covers 4096 / 8192 elements per iteration; a middle-step lane
owns one block of 32 and its workgroup 8192 elements.  BAGUA_TUNE_MX8_*_BLOCKS=2 caps the
grid at two workgroups, which puts the start of the second grid-stride iteration at twice
what one workgroup covers."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp8_reference as R
from oracle import oracle_np as NP
from test_gpu_codec import assert_float_bits_equal
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_op_edges import KernelNames

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
GRID_KNOBS = ("BAGUA_TUNE_MX8_ENCODE_BLOCKS", "BAGUA_TUNE_MX8_DECODE_BLOCKS", "BAGUA_TUNE_MX8_MIDDLE_BLOCKS")

# one below, at and one above: a block (32); what a lane covers (4 / 8); what an encode wave covers
# (2048 / 4096); what a workgroup covers (encode 8192 / 16384, decode 4096 / 8192); the second
# grid-stride iteration under a two-workgroup grid (encode 16384 / 32768, decode 8192 / 16384); and 1
SIZES = [1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193,
         16383, 16384, 16385, 32767, 32768, 32769]


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


def grads(rng, n, dtype, scale=1e-3):
    """gradient-like values whose magnitude changes from block to block"""
    mag = np.repeat(10.0 ** rng.uniform(-3, 2, (n + 31) // 32), 32)[:n]
    return NP.from_f32((rng.standard_normal(n) * mag * scale).astype(np.float32), dtype)


def dev_at(x, dtype, offset=0):
    """x on the device, `offset` elements into a fresh allocation (offset 1: not 16-B aligned)"""
    base = torch.zeros(x.size + offset, dtype=TORCH[dtype], device="cuda")
    view = base[offset:]
    view.copy_(dev(x, dtype))
    return view


def u8(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"


def roundtrip(bc, x, dtype, p, what, offset=0):
    """compress + decompress_from through BaguaTensorPy against the reference"""
    xt = dev_at(x, dtype, offset)
    comp = bc.BaguaTensorPy(xt, "x").compress("MXFP8", p, -1)
    want = R.compress(x, dtype, p)
    assert comp.num_elements() == R.compressed_bytes(x.size // p, p)
    same_bytes(comp.to_numpy_u8(), want, f"{what}: compressed")
    out = dev_at(np.zeros_like(x), dtype, offset)
    out.fill_(7.0)
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP8", p, comp)
    dec = R.decompress(want, p, np.zeros_like(x), dtype)
    same_bytes(host(out, dtype), dec, f"{what}: decoded")


# ------------------------------------------------------------------ codec ----
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_view(bc, dtype):
    rng = np.random.default_rng(77 + dtype)
    for cs, p in [(33, 1), (8193, 1), (1000, 3), (1001, 2)]:
        roundtrip(bc, grads(rng, p * cs, dtype), dtype, p, f"base[1:] cs={cs} p={p}", offset=1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_target_chunk_leaves_the_rest(bc, dtype):
    K = bc._native.K
    rng = np.random.default_rng(5 + dtype)
    p, cs = 4, 1000
    x = grads(rng, p * cs, dtype)
    xt = dev(x, dtype)
    S = R.compressed_bytes(cs, p)
    assert K.bagua_mxfp8_compressed_bytes(cs, p) == S
    for target in (0, 2, 3):
        out = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
        assert K.bagua_mxfp8_compress(dtype, xt.data_ptr(), x.size, cs, p, out.data_ptr(), S, target, None) == OK
        want = R.compress(x, dtype, p, target, out=np.full(S, 0xAB, np.uint8))
        same_bytes(u8(out), want, f"target {target}")
        # through BaguaTensorPy the buffer is fresh from the pool: only the target's segment is defined
        seg = S // p
        got = bc.BaguaTensorPy(xt, "x").compress("MXFP8", p, target).to_numpy_u8()
        same_bytes(got[target * seg:(target + 1) * seg], want[target * seg:(target + 1) * seg], f"target {target}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_partially_valid_tensor(bc, dtype):
    """elements at or past num_elem count as +0, however large they are"""
    N = bc._native
    rng = np.random.default_rng(9 + dtype)
    p, cs = 3, 1000
    huge = NP.from_f32(np.full(p * cs, 6e4, np.float32), dtype)
    for num_elem in (cs + 517, 2 * cs, 2 * cs + 31, 5, 0):
        x = grads(rng, p * cs, dtype)
        x[num_elem:num_elem + 40] = huge[num_elem:num_elem + 40]
        xt = dev(x, dtype)
        raw = bc.BaguaTensorPy(xt, "x").raw()
        raw.num_elem = num_elem
        out = N.bagua_tensor_t()
        N.check(N.C.bagua_tensor_compress(ctypes.byref(raw), N.COMPRESSION_MXFP8, p, 0, -1, ctypes.byref(out)), "compress")
        comp = bc.BaguaTensorPy._from_raw(out, "c", owned=True)
        same_bytes(comp.to_numpy_u8(), R.compress(x, dtype, p, num_elem=num_elem), f"num_elem={num_elem}")


# --------------------------------------------------------- hostile inputs ----
def hostile_inputs(dtype):
    """name -> tensor of 2 chunks of 1000 elements (31 blocks and a ragged one of 8)"""
    rng = np.random.default_rng(31 + dtype)
    p, cs = 2, 1000
    mx = np.float32(R.MAX_FINITE[dtype])
    tiny = {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}[dtype]

    def base():
        return NP.to_f32(grads(rng, p * cs, dtype), dtype).copy()

    out = {}
    for name, pos in (("nan first block", 3), ("nan middle block", 500), ("nan last ragged block", cs - 2)):
        x = base()
        x[pos] = np.nan
        x[cs + pos] = np.nan
        out[name] = x
    x = base()
    x[[5, 700, cs - 1]] = np.inf
    x[[6, 701, cs + 40]] = -np.inf
    out["inf"] = x
    x = base()
    x[[1, 640, cs - 1]] = mx
    x[[2, 641]] = -mx
    out["largest finite"] = x
    out["minus zero only"] = np.full(p * cs, -0.0, np.float32)
    x = (rng.integers(-3, 4, p * cs) * tiny).astype(np.float32)
    out["denormal only"] = x
    x = base()
    x[:cs] = 0.0
    out["all-zero chunk"] = x
    x = base() * np.float32(1e-3 if dtype != F16 else 1.0)
    # f16 spans 2^40 from its smallest denormal to its largest finite value
    big, small = (np.float32(2.0 ** 40), np.float32(1.0)) if dtype != F16 else (np.float32(65504.0), np.float32(2.0 ** -24))
    x[64:96] = small
    x[70] = big
    out["one element 2^40 above the rest"] = x
    with np.errstate(over="ignore", invalid="ignore"):
        return {k: NP.from_f32(v, dtype) for k, v in out.items()}, p


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_inputs(bc, dtype):
    cases, p = hostile_inputs(dtype)
    for name, x in cases.items():
        roundtrip(bc, x, dtype, p, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_of_hostile_bytes(bc, dtype):
    """scale bytes 0, 254 and 255 (and 1, 127, 247, 248) under every element byte, magnitude 0x7F included"""
    scales = np.repeat(np.array([0, 254, 255, 1, 127, 247, 248], np.uint8), 8)
    cs = 32 * scales.size - 5  # ragged: the last block decodes 27 elements
    nb, sb = R.blocks(cs), R.scale_bytes(cs)
    buf = np.zeros(R.compressed_bytes(cs, 1), np.uint8)
    buf[:nb] = scales
    buf[sb:sb + 32 * nb] = np.tile(np.arange(256, dtype=np.uint8), scales.size // 8)
    comp = bc.BaguaTensorPy(torch.from_numpy(buf).cuda(), "hostile bytes")
    out = torch.zeros(cs, dtype=TORCH[dtype], device="cuda")
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP8", 1, comp)
    want = R.decompress(buf, 1, np.zeros(cs, R.STORAGE[dtype]), dtype)
    same_bytes(host(out, dtype), want, "decode")
    mx = R.MAX_FINITE[dtype]
    wf = NP.to_f32(want, dtype)
    assert np.isnan(wf[512:768]).all() and np.isnan(wf[127]) and np.isnan(wf[255]) and np.nanmax(np.abs(wf)) == mx


# ------------------------------------------------------------ middle step ----
def received(rng, p, cs, dtype):
    """p segments as the alltoall delivers them: segment j is rank j's encode of the own chunk.
    Rank 0's holds a NaN block; on f16 the values are large enough for the sum to overflow."""
    scale = 3e4 if dtype == F16 else 1e-3
    x = NP.to_f32(grads(rng, p * cs, dtype, scale=scale), dtype).copy()
    if dtype == F16:
        x[cs // 2:cs // 2 + 8] = 60000.0  # in every segment: the sum leaves the f16 range
        for c in range(p):
            x[c * cs + cs // 2:c * cs + cs // 2 + 8] = 60000.0
    x[37] = np.nan
    with np.errstate(over="ignore", invalid="ignore"):
        return R.compress(NP.from_f32(x, dtype), dtype, p)


@pytest.mark.parametrize("p", list(range(1, 17)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_requantize(bc, dtype, p, monkeypatch):
    """every p the fused middle step takes: for p = 5 to 7 and 9 to 15 the summation tree's second round
    is partly filled (the kernel breaks out of it at p and clamps the index it loads from)"""
    K = bc._native.K
    monkeypatch.setenv("BAGUA_TUNE_MX8_MIDDLE_BLOCKS", "2")  # cs below spans two grid-stride iterations
    rng = np.random.default_rng(100 * dtype + p)
    # the larger size for one p of each kind as well: a partly filled second round under BY = 4 (5) and BY = 8 (12)
    for cs in (1000, 2 * 8192 + 33) if p in (1, 2, 3, 4, 5, 8, 12, 16) else (1000,):
        recv = received(rng, p, cs, dtype)
        S = recv.size
        rt = torch.from_numpy(recv).cuda()
        target = p // 2
        for average in (0, 1):
            want_buf, want_t = R.reduce_requantize(recv, p, cs, dtype, target, bool(average),
                                                   out=np.full(S, 0xCD, np.uint8))
            for store in (False, True):
                what = f"p={p} cs={cs} average={average} store={store}"
                out = torch.full((S,), 0xCD, dtype=torch.uint8, device="cuda")
                tensor = torch.full((p * cs,), 5.0, dtype=TORCH[dtype], device="cuda")
                rc = K.bagua_mxfp8_reduce_requantize(dtype, rt.data_ptr(), S, cs, p, tensor.data_ptr() if store else None,
                                                     average, out.data_ptr(), S, target, None)
                assert rc == OK, what
                same_bytes(u8(out), want_buf, what)
                got_t = host(tensor, dtype)
                if store:
                    assert_float_bits_equal(got_t[target * cs:(target + 1) * cs], want_t[target * cs:(target + 1) * cs],
                                            dtype, what)
                else:
                    assert (NP.to_f32(got_t, dtype) == 5.0).all(), f"{what}: the tensor must not be written"


def test_reduce_requantize_refuses_17_segments(bc):
    K = bc._native.K
    p, cs = 17, 64
    S = R.compressed_bytes(cs, p)
    buf = torch.zeros(S, dtype=torch.uint8, device="cuda")
    out = torch.zeros(S, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp8_reduce_requantize(F32, buf.data_ptr(), S, cs, p, None, 1, out.data_ptr(), S, 0, None) == UNSUPPORTED


# -------------------------------------------------------------------- ops ----
def run_centralized(bc, comms, fn, ts, average, num_elem=None, timed=False):
    N = bc._native
    names = []

    def rank(r):
        raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
        if num_elem is not None:
            raw.num_elem = num_elem
        if timed and r == 0:
            with KernelNames(N, comms[0]) as k:
                rc = fn(comms[r].handle, ctypes.byref(raw), average, N.COMPRESSION_MXFP8)
            names.extend(k.names)
        else:
            rc = fn(comms[r].handle, ctypes.byref(raw), average, N.COMPRESSION_MXFP8)
        N.check(rc, f"rank {r}")

    torch.cuda.synchronize()
    run_ranks(rank, len(ts))
    return names


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 17])
def test_centralized_op(bc, p, fused):
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    fn = (N.C.bagua_centralized_low_precision_synchronous if fused
          else N.C.bagua_centralized_low_precision_synchronous_unfused)
    comms = loopback_communicators(p, 0)
    cs, dt = 1000, F32
    rng = np.random.default_rng(40 + p)
    first = True
    for dt in (F32, BF16):
        for average in (1, 0):
            xs = [grads(rng, p * cs, dt) for _ in range(p)]
            ts = [dev(x, dt) for x in xs]
            names = run_centralized(bc, comms, fn, ts, average, timed=first)
            if first:  # the path: the fused kernel up to 16 ranks, the composed steps otherwise
                assert "mxfp8_encode_kernel" in names and "mxfp8_decode_kernel" in names, names
                if fused and p <= 16:
                    assert "mxfp8_reduce_encode_kernel" in names and "reduce_chunks_kernel" not in names, names
                else:
                    assert "reduce_chunks_kernel" in names and "mxfp8_reduce_encode_kernel" not in names, names
                first = False
            want = R.centralized(xs, dt, bool(average))
            for r in range(p):
                same_bytes(host(ts[r], dt), want[r], f"p={p} dtype={dt} average={average} rank {r}")
    # a partially valid tensor (huge values past the last valid element): the composed steps
    num_elem = p * cs - cs // 2 - 3
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    for x in xs:
        x[num_elem:] = 3e38
    ts = [dev(x, F32) for x in xs]
    names = run_centralized(bc, comms, fn, ts, 1, num_elem=num_elem, timed=True)
    assert "mxfp8_reduce_encode_kernel" not in names and "reduce_chunks_kernel" in names, names
    want = R.centralized(xs, F32, True, num_elem=num_elem)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"p={p} partially valid rank {r}")


# (the ring op and the bucket op by name: tests/test_gpu_mxfp8_op.py)
def test_hierarchical_centralized_op(bc):
    from test_gpu_hierarchical import _node_reduce, _run, _topology
    N = bc._native
    nodes, per_node = 2, 2
    p = nodes * per_node
    n = 1000 * nodes
    rng = np.random.default_rng(8)
    xs = [(rng.standard_normal(n) * 1e-3).astype(np.float32) for _ in range(p)]
    comms = _topology(bc, nodes, per_node)
    ts = [torch.from_numpy(x.copy()).cuda() for x in xs]
    torch.cuda.synchronize()

    def rank(g):
        intra, inter = comms[g]
        raw = bc.BaguaTensorPy(ts[g], "g").raw()
        N.check(N.C.bagua_centralized_low_precision_hierarchical(
            intra.handle, inter.handle if inter is not None else None, ctypes.byref(raw), 1, N.COMPRESSION_MXFP8),
            "hierarchical op")

    _run(p, rank)
    want = R.centralized([_node_reduce(xs[k * per_node:(k + 1) * per_node], True) for k in range(nodes)], F32, True)
    for g in range(p):
        same_bytes(host(ts[g], F32), want[g // per_node], f"rank {g}")


# -------------------------------------------------------- argument errors ----
def test_argument_errors(bc):
    K = bc._native.K
    cs, p = 100, 2
    S = R.compressed_bytes(cs, p)
    x = torch.zeros(cs * p, device="cuda")
    out = torch.zeros(S, dtype=torch.uint8, device="cuda")
    xp, op = x.data_ptr(), out.data_ptr()
    assert K.bagua_mxfp8_compress(F32, xp, cs * p, cs, p, op, S, -1, None) == OK
    assert K.bagua_mxfp8_compress(F32, xp, cs * p, cs, p, op, S - 1, -1, None) == INVALID_ARG   # short output
    assert K.bagua_mxfp8_compress(3, xp, cs * p, cs, p, op, S, -1, None) == UNSUPPORTED          # U8 is no codec dtype
    assert K.bagua_mxfp8_compress(F32, xp, cs * p, cs, p, op, S, p, None) == INVALID_ARG        # target out of range
    assert K.bagua_mxfp8_compress(F32, xp, cs * p, cs, p, op, S, -2, None) == INVALID_ARG
    assert K.bagua_mxfp8_compress(F32, xp, cs * p, cs, p, op + 4, S, -1, None) == INVALID_ARG   # misaligned output
    assert K.bagua_mxfp8_compress(F32, None, cs * p, cs, p, op, S, -1, None) == INVALID_ARG
    assert K.bagua_mxfp8_decompress(F32, op, S - 1, cs, p, xp, None) == INVALID_ARG
    assert K.bagua_mxfp8_decompress(7, op, S, cs, p, xp, None) == UNSUPPORTED
    assert K.bagua_mxfp8_reduce_requantize(F32, op, S, cs, p, None, 1, op, S - 1, 0, None) == INVALID_ARG
    assert K.bagua_mxfp8_reduce_requantize(F32, op, S, cs, p, None, 1, op, S, p, None) == INVALID_ARG
    assert K.bagua_mxfp8_reduce_requantize(9, op, S, cs, p, None, 1, op, S, 0, None) == UNSUPPORTED
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        bc.BaguaTensorPy(x, "x").compress("MXFP8", 3, -1)  # 200 % 3 != 0


# ------------------------------------------------------------ block ranges ----
TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
FILL = 0xA5


def piece_ranges(K, cs, schedule):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & 0xFFFF):
        assert K.bagua_mxfp8_piece_range(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == OK
        assert (b.value, e.value) == R.piece_range(cs, schedule, q)
        out.append((b.value, e.value))
    assert out[0][0] == 0 and out[-1][1] == R.blocks(cs)
    return out


@pytest.mark.parametrize("cs", [3 * 4096 + 33, 128 * 32 * 5, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_range_entries_reproduce_the_whole_chunk_bytes(bc, dtype, cs):
    """pieces 1, 3, 4 and 4 | TAPERED: encode, decode and middle step range by range (last piece
    first) give the whole-chunk entries' bytes; at cs = 1000 the trailing pieces are empty"""
    K = bc._native.K
    p = 3
    rng = np.random.default_rng(8000 + 10 * dtype + cs % 97)
    x = grads(rng, p * cs, dtype)
    xt = dev(x, dtype)
    comp = R.compress(x, dtype, p)
    S = comp.size
    dec = R.decompress(comp, p, np.zeros(p * cs, R.STORAGE[dtype]), dtype)
    recv = received(rng, p, cs, dtype)
    rt = torch.from_numpy(recv).cuda()
    ct = torch.from_numpy(comp).cuda()
    mid, _ = R.reduce_requantize(recv, p, cs, dtype, 1, True, out=np.full(S, FILL, np.uint8))
    for schedule in (1, 3, 4, 4 | TAPERED):
        what = f"cs={cs} schedule={schedule:#x}"
        rs = piece_ranges(K, cs, schedule)
        if cs == 1000:
            assert rs[0] == (0, 32) and all(b == e == 32 for b, e in rs[1:])
        enc = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        out = torch.full((p * cs,), 7.0, dtype=TORCH[dtype], device="cuda")
        mo = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        for bb, be in reversed(rs):
            if bb == be:
                continue  # the op skips empty pieces
            assert K.bagua_mxfp8_compress_range(dtype, xt.data_ptr(), x.size, cs, p, enc.data_ptr(), S, bb, be, None) == OK
            assert K.bagua_mxfp8_decompress_range(dtype, ct.data_ptr(), S, cs, p, out.data_ptr(), bb, be, None) == OK
            assert K.bagua_mxfp8_reduce_requantize_range(dtype, rt.data_ptr(), S, cs, p, 1, mo.data_ptr(), S, 1, bb, be,
                                                         None) == OK
        same_bytes(u8(enc), comp, f"{what}: encode")
        same_bytes(host(out, dtype), dec, f"{what}: decode")
        same_bytes(u8(mo), mid, f"{what}: middle step")
    # one piece alone touches nothing outside its ranges
    bb, be = piece_ranges(K, cs, 3)[0]
    enc = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp8_compress_range(dtype, xt.data_ptr(), x.size, cs, p, enc.data_ptr(), S, bb, be, None) == OK
    nb, sb, seg = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    m = np.zeros(seg, bool)
    m[bb:sb if be == nb else be] = True
    m[sb + 32 * bb:seg if be == nb else sb + 32 * be] = True
    same_bytes(u8(enc), np.where(np.tile(m, p), comp, FILL).astype(np.uint8), "piece 0 alone")


def test_bad_block_ranges_are_refused(bc):
    K = bc._native.K
    cs, p = 128 * 32 * 3 + 40, 2   # nb = 386
    S = R.compressed_bytes(cs, p)
    x = torch.zeros(cs * p, device="cuda")
    buf = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    for bb, be in ((64, 128), (0, 387), (256, 128), (-1, 128), (0, 100), (-1, -1), (386, 386 + 128), (512, 512)):
        assert K.bagua_mxfp8_compress_range(F32, x.data_ptr(), cs * p, cs, p, out.data_ptr(), S, bb, be, None) == INVALID_ARG
        assert K.bagua_mxfp8_decompress_range(F32, buf.data_ptr(), S, cs, p, x.data_ptr(), bb, be, None) == INVALID_ARG
        assert K.bagua_mxfp8_reduce_requantize_range(F32, buf.data_ptr(), S, cs, p, 1, out.data_ptr(), S, 0, bb, be,
                                                     None) == INVALID_ARG
    assert (u8(out) == FILL).all() and not x.any()
    p17 = 17
    S17 = R.compressed_bytes(4096 + 64, p17)
    b17 = torch.zeros(S17, dtype=torch.uint8, device="cuda")
    o17 = torch.full((S17,), FILL, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp8_reduce_requantize_range(F32, b17.data_ptr(), S17, 4096 + 64, p17, 1, o17.data_ptr(), S17, 0, 0,
                                                 128, None) == UNSUPPORTED
    assert (u8(o17) == FILL).all()
