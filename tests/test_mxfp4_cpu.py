"""CPU tests of the MXFP4 codec's rules (MXFP4.md) on the numpy reference
(tests/mxfp4_reference.py), and of the kernels' block arithmetic
(csrc/kernels/mxfp4_common.hpp, compiled for the host) against that reference."""
import os
import subprocess

import numpy as np
import pytest

import mxfp4_reference as R
from oracle import oracle_np as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
# decades a random block's magnitude is drawn from: the whole normal range of the type
DECADES = {F32: (-30, 30), F16: (-4, 3), BF16: (-30, 30)}


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


def bits(v, dtype):
    return v.view(np.uint32 if dtype == F32 else np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_error_bound_and_idempotence(dtype):
    x = random_blocks(dtype, 4000, 11 + dtype)
    x = x[np.isfinite(x).all(axis=1)]
    scale, payload = R.encode_blocks(x, dtype)
    d1 = R.decode_blocks(scale, payload, dtype)
    e = scale.astype(np.int64) - 127
    amax = np.abs(x).max(axis=1)
    ok = (e > -127) & (amax < R.MAX_FINITE[dtype] / 2)
    assert ok.sum() > 1000
    err = np.abs(stored64(d1, dtype) - x)
    assert (err[ok] <= np.ldexp(1.0, e[ok])[:, None]).all()
    # no element saturates: the largest scaled magnitude is within the grid, and above half of it
    y = np.ldexp(amax[ok], -e[ok])
    assert (y <= 6.0).all() and (y > 3.0).all()
    # decode(encode(decode(encode x))) == decode(encode x), bit for bit
    s2, p2 = R.encode_blocks(stored64(d1, dtype), dtype)
    d2 = R.decode_blocks(s2, p2, dtype)
    assert np.array_equal(bits(d1, dtype), bits(d2, dtype))


def test_f16_decode_is_exact_in_the_normal_range():
    x = random_blocks(F16, 3000, 5)
    amax = np.abs(x).max(axis=1)
    x = x[(amax >= 2.0 ** -14) & (amax < 32768.0)]
    scale, payload = R.encode_blocks(x, F16)
    d16 = stored64(R.decode_blocks(scale, payload, F16), F16)
    d32 = stored64(R.decode_blocks(scale, payload, F32), F32)
    keep = np.abs(d32) >= 2.0 ** -24  # what f16 can hold at all
    assert np.array_equal(d16[keep], d32[keep])


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_table(dtype):
    # a 6 in the block pins e = 0 (6 = 0.75 * 2^3: e = 3 - 3), so the values are their own scaled form
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]
    x = np.zeros((1, 32))
    x[0, 0] = 6.0
    x[0, 1:8] = ties
    x[0, 8:15] = [-t for t in ties]
    scale, payload = R.encode_blocks(x, dtype)
    assert scale[0] == 127
    nib = np.empty(32, np.uint8)
    nib[0::2], nib[1::2] = payload[0] & 15, payload[0] >> 4
    assert nib[0] == 7
    assert list(nib[1:8]) == want
    assert list(nib[8:15]) == [8 | c for c in want]
    assert list(nib[15:]) == [0] * 17


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
    assert scale[3] == 0 and (payload[3] == 0x88).all()
    assert (v[3] == 0).all() and np.signbit(v[3]).all()
    assert payload[4, 0] == 0x86 and payload[4, 1] == 0x08
    assert np.signbit(v[4, 1]) and np.signbit(v[4, 2]) and v[4, 2] == 0


def test_exponent_clamp_on_f32_denormals():
    tiny = 2.0 ** -149
    x = np.zeros((2, 32))
    x[0, :4] = [tiny, -3 * tiny, 2.0 ** -127, 1.5 * 2.0 ** -127]   # denormal-only block
    x[1, :3] = [2.0 ** -126, 2.0 ** -128, -(2.0 ** -129)]          # smallest normal: e would be -128
    scale, payload = R.encode_blocks(x, F32)
    assert list(scale) == [0, 0]
    v = stored64(R.decode_blocks(scale, payload, F32), F32)
    # under e = -127 the grid is 0, 2^-128, 2^-127, 1.5 * 2^-127, ...
    assert list(v[0, :4]) == [0.0, -0.0, 2.0 ** -127, 1.5 * 2.0 ** -127]
    assert list(v[1, :3]) == [2.0 ** -126, 2.0 ** -128, -0.0]   # 2^-129 is the tie 0.25: code 0, sign kept
    assert np.signbit(v[1, 2])


@pytest.mark.parametrize("cs", [1, 31, 32, 33, 63, 64, 1025])
def test_layout_and_sizes(cs):
    nb = (cs + 31) // 32
    assert R.blocks(cs) == nb
    assert R.scale_bytes(cs) % 32 == 0 and 0 <= R.scale_bytes(cs) - nb < 32
    assert R.payload_bytes(cs) % 32 == 0 and 0 <= R.payload_bytes(cs) - 16 * nb < 32
    seg = R.segment_bytes(cs)
    for p in (1, 2, 3, 7, 16, 17):
        assert R.compressed_bytes(cs, p) == p * seg and R.compressed_bytes(cs, p) % p == 0
    # element 2j is the low nibble of payload byte j, element 2j + 1 the high one; slack is zero
    p = 3
    x = np.zeros(p * cs, np.float32)
    x[cs:2 * cs] = 1.0       # chunk 1: 1 = 0.5 * 2^1, so e = -2 and every valid element is 4 = code 6
    buf = R.compress(x, F32, p)
    s = buf[seg:2 * seg]
    assert (s[:nb] == 127 - 2).all() and not s[nb:R.scale_bytes(cs)].any()
    pay = s[R.scale_bytes(cs):]
    nib = np.empty(2 * pay.size, np.uint8)
    nib[0::2], nib[1::2] = pay & 15, pay >> 4
    assert (nib[:cs] == 6).all() and not nib[cs:].any()
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
    for p in range(2, 17):
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
    exe = str(tmp_path_factory.mktemp("mxfp4") / "mxfp4_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp4_host_check.cpp"), "-o", exe], check=True)
    return exe


def hostile_blocks(dtype):
    mx = R.MAX_FINITE[dtype]
    tiny = 2.0 ** -149 if dtype == F32 else (2.0 ** -24 if dtype == F16 else 2.0 ** -133)
    rows = []
    for amax in (6.0, 4.0, 3.0, 1.0, mx, mx / 2, tiny, 3 * tiny, 2.0 ** -126 if dtype != F16 else 2.0 ** -14):
        r = np.zeros(32)
        r[0] = amax
        r[1:8] = [amax * t / 6.0 for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)]
        r[8:15] = -r[1:8]
        r[15], r[16] = -0.0, amax * 2.0 ** -40
        rows.append(r)
    rows.append(np.full(32, -0.0))
    rows.append(np.array([np.inf, -np.inf] + [1.0] * 30))
    rows.append(np.array([np.nan] + [1.0] * 31))
    rows.append(np.array([2.0 ** 40] + [1.0] * 31) * (1.0 if dtype != F16 else 2.0 ** -30))
    x = np.array(rows)
    with np.errstate(over="ignore", invalid="ignore"):
        return stored64(NP.from_f32(x.astype(np.float32).ravel(), dtype).reshape(x.shape), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_arithmetic_matches_the_reference(host_check, dtype):
    x = np.concatenate([random_blocks(dtype, 6000, 23 + dtype), hostile_blocks(dtype)])
    # every tie of the grid, exactly, under many exponents
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0])
    exps = range(-20, 10) if dtype == F16 else range(-126, 124, 7)
    t = np.array([np.concatenate([[6.0], ties, -ties, np.zeros(15)]) * 2.0 ** k for k in exps])
    x = np.concatenate([x, stored64(NP.from_f32(t.astype(np.float32).ravel(), dtype).reshape(t.shape), dtype)])
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    scale, payload = R.encode_blocks(x, dtype)
    got = subprocess.run([host_check, "encode", maxf], input=x.astype(np.float32).tobytes(), capture_output=True,
                         check=True).stdout
    got = np.frombuffer(got, np.uint8).reshape(-1, 17)
    assert np.array_equal(got[:, 0], scale)
    assert np.array_equal(got[:, 1:], payload)
    # decode: the reference's bytes, plus every nibble under scale bytes 0, 1, 2, 127, 253, 254 and 255
    hs = np.array([0, 1, 2, 127, 253, 254, 255], np.uint8)
    hp = np.tile((np.arange(16, dtype=np.uint8) * 0x11)[None, :], (hs.size, 1))
    hp[:, 8:] = ((np.arange(8) * 0x21 + 0x80) % 256).astype(np.uint8)[None, :]
    s_all, p_all = np.concatenate([scale, hs]), np.concatenate([payload, hp])
    raw = np.concatenate([s_all[:, None], p_all], axis=1).astype(np.uint8).tobytes()
    dec = subprocess.run([host_check, "decode", maxf], input=raw, capture_output=True, check=True).stdout
    dec = np.frombuffer(dec, np.float32).reshape(-1, 32)
    # the host program returns the clamped f32 value; the kernels then round it to T
    got_t = NP.from_f32(dec.ravel(), dtype).reshape(-1, 32)
    want = R.decode_blocks(s_all, p_all, dtype)
    nan = s_all == 0xFF
    assert np.isnan(dec[nan]).all()
    assert np.array_equal(bits(np.ascontiguousarray(got_t[~nan]), dtype), bits(np.ascontiguousarray(want[~nan]), dtype))
