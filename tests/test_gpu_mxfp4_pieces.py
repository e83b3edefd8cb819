"""GPU tests of the MXFP4 block-range kernels (MXFP4.md, "Pipelined op"): the encode, the
decode and the fused middle step on the block ranges of a piece schedule, byte for byte
against the whole-chunk entries and the numpy reference, with every byte outside a piece's
ranges checked untouched.

Shapes: cs = 3 * 4096 + 37 * 32 + 5 has three granule boundaries (128 blocks = 4096
elements), a ragged last tile of 38 blocks and a ragged last block of 5 elements; with three
chunks the chunks after the first are not 16-B aligned and take the guarded loads.  cs =
5 * 4096 is all-vector; cs = 1000 lies inside one granule, so piece 0 holds everything."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp4_boundary_cases as B
import mxfp4_reference as R
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host
from test_gpu_mxfp4 import BF16, DTYPES, F16, F32, OK, TORCH, UNSUPPORTED, grads, received, same_bytes, u8

pytestmark = pytest.mark.gpu

TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
SCHEDULES = [2, 3, 4 | TAPERED, 6, 9]
RAGGED = 3 * 4096 + 37 * 32 + 5
SHAPES = [(RAGGED, 1), (RAGGED, 3), (5 * 4096, 1), (1000, 1)]
FILL = 0xA5
SENTINEL = {F32: 0x5A5A5A5A, F16: 0x5A5A, BF16: 0x5A5A}  # a finite pattern no decode of the inputs gives


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


def ranges(K, cs, schedule):
    """the non-empty pieces of the schedule (the empty ones at the tail launch nothing: the op
    skips them, and the range entries refuse a block_begin at nb that is no multiple of 128)"""
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & 0xFFFF):
        assert K.bagua_mxfp4_piece_range(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == OK
        out.append((b.value, e.value))
    assert out[0][0] == 0 and out[-1][1] == R.blocks(cs)
    return [(b, e) for b, e in out if e > b]


def segment_mask(cs, bb, be):
    """the bytes of one segment that the range [bb, be) may write"""
    nb, sb, seg = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    m = np.zeros(seg, bool)
    if bb < be:
        last = be == nb
        m[bb:sb if last else be] = True
        m[sb + 16 * bb:seg if last else sb + 16 * be] = True
    return m


def sentinel(n, dtype):
    bits = torch.full((n,), SENTINEL[dtype], dtype=torch.int32 if dtype == F32 else torch.int16, device="cuda")
    return bits.view(TORCH[dtype])


def bits_of(t, dtype):
    return np.ascontiguousarray(host(t, dtype)).view(np.uint32 if dtype == F32 else np.uint16)


def whole_encode(K, xt, n, cs, p, dtype):
    S = R.compressed_bytes(cs, p)
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp4_compress(dtype, xt.data_ptr(), n, cs, p, out.data_ptr(), S, -1, None) == OK
    return u8(out)


def check_encode_pieces(K, xt, n, cs, p, dtype, schedule, want, what):
    S = want.size
    rs = ranges(K, cs, schedule)
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    for bb, be in reversed(rs):
        assert K.bagua_mxfp4_compress_range(dtype, xt.data_ptr(), n, cs, p, out.data_ptr(), S, bb, be, None) == OK
    same_bytes(u8(out), want, f"{what}: all pieces")
    for q, (bb, be) in enumerate(rs):
        out.fill_(FILL)
        assert K.bagua_mxfp4_compress_range(dtype, xt.data_ptr(), n, cs, p, out.data_ptr(), S, bb, be, None) == OK
        mask = np.tile(segment_mask(cs, bb, be), p)
        same_bytes(u8(out), np.where(mask, want, FILL).astype(np.uint8), f"{what}: piece {q} alone")


def check_decode_pieces(K, comp, cs, p, dtype, schedule, what):
    S = comp.size
    ct = torch.from_numpy(comp).cuda()
    whole = sentinel(p * cs, dtype)
    assert K.bagua_mxfp4_decompress(dtype, ct.data_ptr(), S, cs, p, whole.data_ptr(), None) == OK
    want = bits_of(whole, dtype)
    rs = ranges(K, cs, schedule)
    out = sentinel(p * cs, dtype)
    for bb, be in reversed(rs):
        assert K.bagua_mxfp4_decompress_range(dtype, ct.data_ptr(), S, cs, p, out.data_ptr(), bb, be, None) == OK
    same_bytes(bits_of(out, dtype), want, f"{what}: all pieces")
    for q, (bb, be) in enumerate(rs):
        out = sentinel(p * cs, dtype)
        assert K.bagua_mxfp4_decompress_range(dtype, ct.data_ptr(), S, cs, p, out.data_ptr(), bb, be, None) == OK
        mask = np.zeros(cs, bool)
        mask[32 * bb:min(32 * be, cs)] = True
        expect = np.where(np.tile(mask, p), want, want.dtype.type(SENTINEL[dtype]))
        same_bytes(bits_of(out, dtype), expect, f"{what}: piece {q} alone")
    return want


@pytest.mark.parametrize("cs,p", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_ranges(bc, dtype, cs, p):
    K = bc._native.K
    rng = np.random.default_rng(7000 + 10 * dtype + p)
    x = grads(rng, p * cs, dtype)
    xt = dev(x, dtype)
    want = R.compress(x, dtype, p)
    same_bytes(whole_encode(K, xt, x.size, cs, p, dtype), want, "whole-chunk entry against the reference")
    for schedule in SCHEDULES:
        check_encode_pieces(K, xt, x.size, cs, p, dtype, schedule, want, f"cs={cs} p={p} schedule={schedule:#x}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_range_of_a_partly_valid_tensor(bc, dtype):
    """elements at or past input_num_element count as +0 in every piece, as in the whole-chunk entry"""
    K = bc._native.K
    cs, p = RAGGED, 3
    rng = np.random.default_rng(7100 + dtype)
    x = grads(rng, p * cs, dtype)
    xt = dev(x, dtype)
    num_elem = cs + 2 * 4096 + 77
    want = R.compress(x, dtype, p, num_elem=num_elem)
    S = want.size
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    for bb, be in reversed(ranges(K, cs, 3)):
        assert K.bagua_mxfp4_compress_range(dtype, xt.data_ptr(), num_elem, cs, p, out.data_ptr(), S, bb, be, None) == OK
    same_bytes(u8(out), want, "partly valid")


@pytest.mark.parametrize("nt", [None, "1"])
@pytest.mark.parametrize("cs,p", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_ranges(bc, dtype, cs, p, nt, monkeypatch):
    K = bc._native.K
    if nt is not None:
        monkeypatch.setenv("BAGUA_MX_DECODE_NT", nt)  # the non-temporal stores: the same bytes
    rng = np.random.default_rng(7200 + 10 * dtype + p)
    x = grads(rng, p * cs, dtype)
    x[5] = NP.from_f32(np.array([np.nan], np.float32), dtype)[0]  # a NaN block decodes to the canonical NaN
    with np.errstate(invalid="ignore"):
        comp = R.compress(x, dtype, p)
    first = True
    for schedule in SCHEDULES if nt is None else (3, 4 | TAPERED):
        got = check_decode_pieces(K, comp, cs, p, dtype, schedule, f"cs={cs} p={p} schedule={schedule:#x} nt={nt}")
        if first:
            want = R.decompress(comp, p, np.zeros(p * cs, R.STORAGE[dtype]), dtype)
            same_bytes(got, want, "whole-chunk entry against the reference")
            first = False


@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step_ranges(bc, dtype, p, average):
    K = bc._native.K
    rng = np.random.default_rng(7300 + 100 * dtype + p)
    for cs in (RAGGED, 5 * 4096, 1000) if p in (2, 16) else (RAGGED,):
        recv = received(rng, p, cs, dtype)
        S = recv.size
        rt = torch.from_numpy(recv).cuda()
        target = p // 2
        whole = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        assert K.bagua_mxfp4_reduce_requantize(dtype, rt.data_ptr(), S, cs, p, None, average, whole.data_ptr(), S,
                                               target, None) == OK
        want = u8(whole)
        ref, _ = R.reduce_requantize(recv, p, cs, dtype, target, bool(average), out=np.full(S, FILL, np.uint8))
        same_bytes(want, ref, "whole-chunk entry against the reference")
        seg = S // p
        for schedule in SCHEDULES:
            what = f"p={p} cs={cs} average={average} schedule={schedule:#x}"
            rs = ranges(K, cs, schedule)
            out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
            for bb, be in reversed(rs):
                assert K.bagua_mxfp4_reduce_requantize_range(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(), S,
                                                             target, bb, be, None) == OK
            same_bytes(u8(out), want, f"{what}: all pieces")
            for q, (bb, be) in enumerate(rs):
                out.fill_(FILL)
                assert K.bagua_mxfp4_reduce_requantize_range(dtype, rt.data_ptr(), S, cs, p, average, out.data_ptr(), S,
                                                             target, bb, be, None) == OK
                mask = np.zeros(S, bool)
                mask[target * seg:(target + 1) * seg] = segment_mask(cs, bb, be)
                same_bytes(u8(out), np.where(mask, want, FILL).astype(np.uint8), f"{what}: piece {q} alone")


def test_middle_step_range_refuses_17_segments(bc):
    K = bc._native.K
    p, cs = 17, 4096 + 64
    S = R.compressed_bytes(cs, p)
    buf = torch.zeros(S, dtype=torch.uint8, device="cuda")
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp4_reduce_requantize_range(F32, buf.data_ptr(), S, cs, p, 1, out.data_ptr(), S, 0, 0, 128,
                                                 None) == UNSUPPORTED
    assert (u8(out) == FILL).all()


@pytest.mark.parametrize("hw", ["0", "1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_table_through_ranges(bc, dtype, hw, monkeypatch):
    """every tie of the grid under every scale byte (tests/mxfp4_boundary_cases.py) as one chunk
    through the encode and decode ranges of 3 and 5 tapered pieces, with the hardware
    conversions and with the arithmetic: the bytes of the whole-chunk entries"""
    K = bc._native.K
    monkeypatch.setenv("BAGUA_MXFP4_HWCVT", hw)
    x = B.table(dtype).x
    cs = x.size
    xt = dev(x, dtype)
    want = R.compress(x, dtype, 1)
    same_bytes(whole_encode(K, xt, cs, cs, 1, dtype), want, "whole-chunk entry against the reference")
    for schedule in (3 | TAPERED, 5 | TAPERED):
        what = f"boundary table, {cs} elements, schedule={schedule:#x} hw={hw}"
        S = want.size
        out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        for bb, be in reversed(ranges(K, cs, schedule)):
            assert K.bagua_mxfp4_compress_range(dtype, xt.data_ptr(), cs, cs, 1, out.data_ptr(), S, bb, be, None) == OK
        same_bytes(u8(out), want, f"{what}: encode")
        check_decode_pieces(K, want, cs, 1, dtype, schedule, f"{what}: decode")
