"""CPU tests of the MXFP8 codec's rules (MXFP8.md) on the numpy reference
(tests/mxfp8_reference.py), of the kernels' block arithmetic
(csrc/kernels/mxfp8_common.hpp, compiled for the host) against that reference, and of the
host-only entries (sizes, piece ranges, argument refusals)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import mxfp8_reference as R
from oracle import oracle_np as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
# decades a random block's magnitude is drawn from: the whole normal range of the type
DECADES = {F32: (-30, 30), F16: (-4, 3), BF16: (-30, 30)}
TAPERED = 0x10000


def random_blocks(dtype, nblocks, seed):
    """(nblocks, 32) float64 values of T: normal draws, one magnitude per block, some exact zeros"""
    rng = np.random.default_rng(seed)
    lo, hi = DECADES[dtype]
    mag = 10.0 ** rng.uniform(lo, hi, (nblocks, 1))
    x = rng.standard_normal((nblocks, 32)) * mag
    x[rng.random((nblocks, 32)) < 0.05] = 0.0
    with np.errstate(over="ignore"):
        t = NP.from_f32(x.astype(np.float32).ravel(), dtype)
    return NP.to_f32(t, dtype).astype(np.float64).reshape(nblocks, 32)


def stored64(v, dtype):
    return NP.to_f32(v.ravel(), dtype).astype(np.float64).reshape(v.shape)


def as_t(x, dtype):
    """float64 values rounded to T, as float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return stored64(NP.from_f32(x.astype(np.float32).ravel(), dtype).reshape(x.shape), dtype)


def bits(v, dtype):
    return v.view(np.uint32 if dtype == F32 else np.uint16)


def edge_blocks(dtype):
    """amax planted on both sides of every 1.75 * 2^j the type holds: 1.75 * 2^j itself and
    the next T value above it"""
    ulp = {F32: 2.0 ** -23, F16: 2.0 ** -10, BF16: 2.0 ** -7}[dtype]
    js = range(-14, 15) if dtype == F16 else range(-125, 127)
    rows = []
    for j in js:
        for a in (1.75 * 2.0 ** j, (1.75 + ulp) * 2.0 ** j):
            r = np.zeros(32)
            r[j % 32] = a
            r[(j + 5) % 32] = -a / 3
            rows.append(r)
    return as_t(np.array(rows), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_error_bound_scaled_maximum_and_idempotence(dtype):
    x = np.concatenate([random_blocks(dtype, 2048, 11 + dtype), edge_blocks(dtype)])
    x = x[np.isfinite(x).all(axis=1)]
    assert x.size >= 2 ** 16
    scale, payload = R.encode_blocks(x, dtype)
    assert ((payload & 0x7F) != 0x7F).all()       # the encoder never writes magnitude 0x7F
    d1 = R.decode_blocks(scale, payload, dtype)
    e = scale.astype(np.int64) - 127
    amax = np.abs(x).max(axis=1)
    ok = (e > -127) & (amax < R.MAX_FINITE[dtype] / 2) & (amax > 0)
    assert ok.sum() > 1000
    # |x^ - x| <= max(|x| 2^-4, 2^(e - 10)), up to the rounding of the decode to T (half an ulp of T)
    ulp_t = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dtype]
    err = np.abs(stored64(d1, dtype) - x)
    bound = np.maximum(np.abs(x) * 2.0 ** -4, np.ldexp(1.0, e - 10)[:, None])
    if dtype == F16:  # below 2^-14 f16's own step (2^-24) may exceed the codec's
        bound = np.maximum(bound, 2.0 ** -25)
    assert (err[ok] <= (bound + np.abs(x) * ulp_t)[ok]).all()
    # no element saturates: the largest scaled magnitude is within the grid, and above half of it
    y = np.ldexp(amax[ok], -e[ok])
    assert (y <= 448.0).all() and (y > 224.0).all()
    # decode(encode(decode(encode x))) == decode(encode x), bit for bit
    s2, p2 = R.encode_blocks(stored64(d1, dtype), dtype)
    d2 = R.decode_blocks(s2, p2, dtype)
    assert np.array_equal(bits(d1, dtype), bits(d2, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_agrees_with_torch_float8_e4m3fn(dtype):
    """a second, independent statement of the element rounding: torch's CPU conversion of the
    scaled values (exact in f32: a T value times a power of two, at most 448)"""
    x = np.concatenate([random_blocks(dtype, 2048, 31 + dtype), edge_blocks(dtype)])
    x = x[np.isfinite(x).all(axis=1)]
    scale, payload = R.encode_blocks(x, dtype)
    e, y = R.scaled(x, dtype)
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    want = torch.from_numpy(np.copysign(y32, x.astype(np.float32))).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert ((want & 0x7F) != 0x7F).all()          # torch never overflows to its NaN either
    assert np.array_equal(payload, want)
    # and back: torch's value of every code, times the scale, is the reference's decode
    codes = np.arange(256, dtype=np.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    vals = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    assert np.array_equal(np.abs(vals), R.GRID[codes & 0x7F])
    assert np.array_equal(np.signbit(vals), (codes & 0x80) != 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_table(dtype):
    # a 448 in the block pins e = 0 (448 = 0.875 * 2^9: e = 9 - 9), so the values are their own scaled form
    ties = [2.0 ** -10, 3 * 2.0 ** -10, 15 * 2.0 ** -10, 17 * 2.0 ** -10, 1.0625, 1.1875, 400.0]
    want = [0x00, 0x02, 0x08, 0x08, 0x38, 0x3A, 0x7C]
    x = np.zeros((1, 32))
    x[0, 0] = 448.0
    x[0, 1:8] = ties
    x[0, 8:15] = [-t for t in ties]
    x = as_t(x, dtype)
    assert np.array_equal(np.abs(x[0, 1:8]), ties)   # every T holds them
    scale, payload = R.encode_blocks(x, dtype)
    assert scale[0] == 127 and payload[0, 0] == 0x7E
    assert list(payload[0, 1:8]) == want
    assert list(payload[0, 8:15]) == [0x80 | c for c in want]
    assert list(payload[0, 15:]) == [0] * 17


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_inf_largest_finite_and_signed_zero(dtype):
    mx = R.MAX_FINITE[dtype]
    x = np.zeros((5, 32))
    x[0, 7] = np.nan                      # NaN block
    x[0, 8] = 1.0
    x[1, 0], x[1, 1], x[1, 2] = np.inf, -np.inf, 1.0
    x[2, 0], x[2, 1] = mx, -mx
    x[3, :] = -0.0                        # -0 only
    x[4, 0], x[4, 1], x[4, 2] = 1.0, -0.0, -1e-6   # a value rounding to zero keeps its sign
    scale, payload = R.encode_blocks(x, dtype)
    assert scale[0] == 0xFF and not payload[0].any()
    d = R.decode_blocks(scale, payload, dtype)
    assert (bits(d, dtype)[0] == R.NAN_BITS[dtype]).all()
    v = stored64(d, dtype)
    assert v[1, 0] == mx and v[1, 1] == -mx and v[2, 0] == mx and v[2, 1] == -mx
    assert scale[1] == scale[2] == {F32: 247, F16: 135, BF16: 247}[dtype]
    assert scale[3] == 0 and (payload[3] == 0x80).all()
    assert (v[3] == 0).all() and np.signbit(v[3]).all()
    assert payload[4, 0] == 0x78 and payload[4, 1] == 0x80 and payload[4, 2] == 0x80   # 1 = 256 * 2^-8
    assert np.signbit(v[4, 1]) and np.signbit(v[4, 2]) and v[4, 2] == 0
    # magnitude 0x7F from a hostile sender: the canonical NaN for that element alone
    hs, hp = np.array([127], np.uint8), np.zeros((1, 32), np.uint8)
    hp[0, :4] = [0x7F, 0xFF, 0x7E, 0x38]
    hd = R.decode_blocks(hs, hp, dtype)
    assert (bits(hd, dtype)[0, :2] == R.NAN_BITS[dtype]).all()
    assert list(stored64(hd, dtype)[0, 2:5]) == [448.0, 1.0, 0.0]


def test_exponent_clamp_on_f32_denormals():
    tiny = 2.0 ** -149
    x = np.zeros((2, 32))
    x[0, :4] = [tiny, -3 * tiny, 2.0 ** -127, 1.5 * 2.0 ** -127]   # denormal-only block
    x[1, :3] = [2.0 ** -126, 2.0 ** -136, -(2.0 ** -138)]          # smallest normal: e would be -134
    scale, payload = R.encode_blocks(x, F32)
    assert list(scale) == [0, 0]
    v = stored64(R.decode_blocks(scale, payload, F32), F32)
    # under e = -127 the grid's smallest step is 2^-136
    assert list(v[0, :4]) == [0.0, -0.0, 2.0 ** -127, 1.5 * 2.0 ** -127]
    assert list(v[1, :3]) == [2.0 ** -126, 2.0 ** -136, -0.0]   # 2^-138 is below the tie 2^-137: code 0, sign kept
    assert np.signbit(v[1, 2])


@pytest.mark.parametrize("cs", [1, 31, 32, 33, 63, 64, 1025])
def test_layout_and_sizes(cs):
    nb = (cs + 31) // 32
    assert R.blocks(cs) == nb
    assert R.scale_bytes(cs) % 32 == 0 and 0 <= R.scale_bytes(cs) - nb < 32
    assert R.payload_bytes(cs) == 32 * nb
    seg = R.segment_bytes(cs)
    for p in (1, 2, 3, 7, 16, 17):
        assert R.compressed_bytes(cs, p) == p * seg and R.compressed_bytes(cs, p) % p == 0
    # element j of a block is payload byte j; slack is zero
    p = 3
    x = np.zeros(p * cs, np.float32)
    x[cs:2 * cs] = 1.0       # chunk 1: 1 = 0.5 * 2^1, so e = -8 and every valid element is 256 = code 0x78
    buf = R.compress(x, F32, p)
    s = buf[seg:2 * seg]
    assert (s[:nb] == 127 - 8).all() and not s[nb:R.scale_bytes(cs)].any()
    pay = s[R.scale_bytes(cs):]
    assert (pay[:cs] == 0x78).all() and not pay[cs:].any()
    assert not buf[:seg].any()
    out = np.full(p * cs, 7.0, np.float32)
    R.decompress(buf, p, out, F32)
    assert np.array_equal(out, x)
    # a partially valid tensor: elements at or past num_elem count as +0
    big = x.copy()
    big[cs + cs // 2:] = 3e38
    assert np.array_equal(R.compress(big, F32, p, num_elem=cs + cs // 2),
                          R.compress(np.where(np.arange(p * cs) < cs + cs // 2, x, 0).astype(np.float32), F32, p))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_of_decoded_segments_is_finite(dtype):
    rng = np.random.default_rng(3)
    for p in (2, 3, 5, 9, 16, 17):
        cs = 96
        xs = [NP.from_f32((rng.standard_normal(p * cs) * 10.0 ** rng.uniform(-6, 2)).astype(np.float32), dtype)
              for _ in range(p)]
        for average in (False, True):
            outs = R.centralized(xs, dtype, average)
            for o in outs:
                assert np.isfinite(NP.to_f32(o, dtype)).all()
            assert all(np.array_equal(bits(o, dtype), bits(outs[0], dtype)) for o in outs)


# ---- the kernels' arithmetic, compiled for the host ---------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mxfp8") / "mxfp8_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp8_host_check.cpp"), "-o", exe], check=True)
    return exe


def hostile_blocks(dtype):
    mx = R.MAX_FINITE[dtype]
    tiny = 2.0 ** -149 if dtype == F32 else (2.0 ** -24 if dtype == F16 else 2.0 ** -133)
    mids = (R.GRID[:-1] + R.GRID[1:]) / 2      # all 126 ties between neighbouring codes
    rows = []
    for amax in (448.0, 256.0, 224.0, 1.0, mx, mx / 2, tiny, 3 * tiny, 2.0 ** -126 if dtype != F16 else 2.0 ** -14,
                 2.0 ** -119 if dtype != F16 else 2.0 ** -20):
        for k in range(0, 126, 15):
            r = np.zeros(32)
            r[0] = amax
            m = mids[k:k + 15]
            r[1:1 + m.size] = amax * m / 448.0
            r[16:16 + m.size] = -r[1:1 + m.size]
            r[31] = -0.0
            rows.append(r)
    rows.append(np.full(32, -0.0))
    rows.append(np.array([np.inf, -np.inf] + [1.0] * 30))
    rows.append(np.array([np.nan] + [1.0] * 31))
    rows.append(np.array([2.0 ** 40] + [1.0] * 31) * (1.0 if dtype != F16 else 2.0 ** -30))
    return as_t(np.array(rows), dtype)


def run_host(exe, args, raw):
    return subprocess.run([exe] + args, input=raw, capture_output=True, check=True).stdout


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_arithmetic_matches_the_reference(host_check, dtype):
    x = np.concatenate([random_blocks(dtype, 6000, 23 + dtype), hostile_blocks(dtype), edge_blocks(dtype)])
    # every tie of the grid, exactly, under many exponents
    mids = (R.GRID[:-1] + R.GRID[1:]) / 2
    exps = range(-20, 7) if dtype == F16 else range(-126, 118, 7)
    rows = []
    for k in exps:
        for q in range(0, 126, 31):
            m = mids[q:q + 31]
            rows.append(np.concatenate([[448.0], m if k % 2 else -m, np.zeros(31 - m.size)]) * 2.0 ** k)
    x = np.concatenate([x, as_t(np.array(rows), dtype)])
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    scale, payload = R.encode_blocks(x, dtype)
    got = np.frombuffer(run_host(host_check, ["encode", maxf], x.astype(np.float32).tobytes()), np.uint8).reshape(-1, 33)
    assert np.array_equal(got[:, 0], scale)
    assert np.array_equal(got[:, 1:], payload)
    # decode: the reference's bytes, plus every element byte under scale bytes 0, 1, 2, 127, 246 .. 255
    hs = np.repeat(np.array([0, 1, 2, 8, 9, 127, 246, 247, 248, 253, 254, 255], np.uint8), 8)
    hp = np.tile(np.arange(256, dtype=np.uint8).reshape(8, 32), (12, 1))
    s_all, p_all = np.concatenate([scale, hs]), np.concatenate([payload, hp])
    raw = np.concatenate([s_all[:, None], p_all], axis=1).astype(np.uint8).tobytes()
    dec = run_host(host_check, ["decode", maxf, str(dtype)], raw)
    got_t = np.frombuffer(dec, np.uint32 if dtype == F32 else np.uint16).reshape(-1, 32)
    want = R.decode_blocks(s_all, p_all, dtype)
    assert np.array_equal(got_t, bits(want, dtype))


def test_host_check_is_clean_under_the_host_sanitizers(tmp_path):
    """the stand-alone program (its own main, no GPU) built with the address and
    undefined-behaviour sanitizers and run over hostile blocks"""
    exe = str(tmp_path / "mxfp8_host_check_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp8_host_check.cpp"), "-o", exe], check=True)
    x = np.concatenate([hostile_blocks(F32), random_blocks(F32, 500, 1)])
    out = subprocess.run([exe, "encode", "7f7fffff"], input=x.astype(np.float32).tobytes(), capture_output=True)
    assert out.returncode == 0 and not out.stderr, out.stderr.decode()
    assert len(out.stdout) == 33 * x.shape[0]
    allb = np.concatenate([np.repeat(np.arange(256, dtype=np.uint8), 8)[:, None],
                           np.tile(np.arange(256, dtype=np.uint8).reshape(8, 32), (256, 1))], axis=1)
    for dtype in DTYPES:
        maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
        out = subprocess.run([exe, "decode", maxf, str(dtype)], input=allb.tobytes(), capture_output=True)
        assert out.returncode == 0 and not out.stderr, out.stderr.decode()
        got = np.frombuffer(out.stdout, np.uint32 if dtype == F32 else np.uint16).reshape(-1, 32)
        # all 256 scale bytes x all 256 element bytes
        assert np.array_equal(got, bits(R.decode_blocks(allb[:, 0], allb[:, 1:], dtype), dtype))


# ---- host-only entries of the library --------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from bagua_core import _native as N
    return N.K


def test_sizes_and_piece_ranges_match_the_reference(lib):
    for cs in (0, 1, 31, 32, 33, 1000, 4096, 4097, 3 * 4096 + 33, 128 * 32 * 5, 1 << 20, (1 << 20) + 77):
        for p in (1, 2, 3, 16, 17):
            assert lib.bagua_mxfp8_compressed_bytes(cs, p) == R.compressed_bytes(cs, p)
        for pieces in (1, 2, 3, 4, 8, 3 | TAPERED, 4 | TAPERED, 8 | TAPERED, 2 | TAPERED):
            prev = 0
            for q in range(pieces & 0xFFFF):
                b, e = ctypes.c_int(-1), ctypes.c_int(-1)
                assert lib.bagua_mxfp8_piece_range(cs, pieces, q, ctypes.byref(b), ctypes.byref(e)) == 0
                assert (b.value, e.value) == R.piece_range(cs, pieces, q), (cs, pieces, q)
                assert b.value == prev and e.value >= b.value
                assert b.value % 128 == 0 or b.value == R.blocks(cs)
                prev = e.value
            assert prev == R.blocks(cs)
    assert lib.bagua_mxfp8_compressed_bytes(-1, 1) == 0 and lib.bagua_mxfp8_compressed_bytes(1, -1) == 0


def test_host_side_refusals(lib):
    b, e = ctypes.c_int(), ctypes.c_int()
    INVALID, UNSUPPORTED = 1, 4     # BAGUA_ERR_INVALID_ARG, BAGUA_ERR_UNSUPPORTED
    assert lib.bagua_mxfp8_piece_range(-1, 1, 0, ctypes.byref(b), ctypes.byref(e)) == INVALID
    assert lib.bagua_mxfp8_piece_range(100, 0, 0, ctypes.byref(b), ctypes.byref(e)) == INVALID
    assert lib.bagua_mxfp8_piece_range(100, 2, 2, ctypes.byref(b), ctypes.byref(e)) == INVALID
    assert lib.bagua_mxfp8_piece_range(100, 2, -1, ctypes.byref(b), ctypes.byref(e)) == INVALID
    assert lib.bagua_mxfp8_piece_range(100, 2, 0, None, ctypes.byref(e)) == INVALID
    assert lib.bagua_mxfp8_piece_range(100, 2 | 0x100000, 0, ctypes.byref(b), ctypes.byref(e)) == INVALID
    # refused before anything is launched: null buffers, bad counts, bad dtype, short or misaligned buffers
    buf = np.zeros(4096, np.uint8)
    off = (-buf.ctypes.data) % 16
    al = buf.ctypes.data + off               # a 16-B aligned host address: never dereferenced
    S = R.compressed_bytes(64, 2)
    assert lib.bagua_mxfp8_compress(F32, None, 128, 64, 2, al, S, -1, None) == INVALID
    assert lib.bagua_mxfp8_compress(F32, al, 128, 64, 2, None, S, -1, None) == INVALID
    assert lib.bagua_mxfp8_compress(F32, al, 128, 64, 0, al, S, -1, None) == INVALID
    assert lib.bagua_mxfp8_compress(F32, al, -1, 64, 2, al, S, -1, None) == INVALID
    assert lib.bagua_mxfp8_compress(F32, al, 128, 64, 2, al, S, 2, None) == INVALID
    assert lib.bagua_mxfp8_compress(F32, al, 128, 64, 2, al, S - 1, -1, None) == INVALID
    assert lib.bagua_mxfp8_compress(F32, al, 128, 64, 2, al + 4, S, -1, None) == INVALID
    assert lib.bagua_mxfp8_compress(3, al, 128, 64, 2, al, S, -1, None) == UNSUPPORTED
    assert lib.bagua_mxfp8_decompress(F32, None, S, 64, 2, al, None) == INVALID
    assert lib.bagua_mxfp8_decompress(F32, al, S - 1, 64, 2, al, None) == INVALID
    assert lib.bagua_mxfp8_decompress(F32, al + 4, S, 64, 2, al, None) == INVALID
    assert lib.bagua_mxfp8_reduce_requantize(F32, al, S, 64, 2, None, 1, al, S, 2, None) == INVALID
    assert lib.bagua_mxfp8_reduce_requantize(F32, al, S, 64, 2, None, 1, al, S - 1, 0, None) == INVALID
    S17 = R.compressed_bytes(64, 17)
    assert lib.bagua_mxfp8_reduce_requantize(F32, al, S17, 64, 17, None, 1, al, S17, 0, None) == UNSUPPORTED
    # ranges: begin not on the granule, end past nb, end before begin, negative begin
    cs = 128 * 32 * 3
    Sb = R.compressed_bytes(cs, 1)
    for bb, be in ((64, 128), (0, 385), (256, 128), (-1, 128), (0, 100), (-1, -1)):
        assert lib.bagua_mxfp8_compress_range(F32, al, cs, cs, 1, al, Sb, bb, be, None) == INVALID, (bb, be)
        assert lib.bagua_mxfp8_decompress_range(F32, al, Sb, cs, 1, al, bb, be, None) == INVALID, (bb, be)
        assert lib.bagua_mxfp8_reduce_requantize_range(F32, al, Sb, cs, 1, 1, al, Sb, 0, bb, be, None) == INVALID, (bb, be)
    # an empty range launches nothing
    assert lib.bagua_mxfp8_compress_range(F32, al, cs, cs, 1, al, Sb, 384, 384, None) == 0
    assert lib.bagua_mxfp8_decompress_range(F32, al, Sb, cs, 1, al, 128, 128, None) == 0


def test_method_is_registered():
    import bagua_core
    from bagua_core import _native as N
    assert bagua_core.METHODS["MXFP8"] == N.COMPRESSION_MXFP8 == 4
