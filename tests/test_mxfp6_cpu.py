"""CPU tests of the MXFP6 codec (MXFP6.md): the kernels' block arithmetic
(csrc/kernels/mxfp6_common.hpp, compiled for the host as tools/mxfp6_host_check.cpp) against
the numpy reference (tests/mxfp6_reference.py) byte for byte and against the error bound, and
the piece table.  The two tables below are also what tests/test_gpu_mxfp6.py feeds the kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mxfp6_reference as R
from oracle import oracle_np as NP
from test_mxfp8_cpu import (BF16, DTYPES, F16, F32, ROOT, as_t, bits, hostile_blocks, random_blocks, run_host,
                            stored64)

# the scale bytes a finite T can produce: f16 from its smallest subnormal 2^-24 (byte 101) to 65504 (byte 141)
SCALE_BYTES = {F32: range(0, 254), F16: range(101, 142), BF16: range(0, 254)}
# triples of the tie table T cannot hold, a property of T and the grid alone: the 7 midpoints above 4 under
# the top scale byte (past the largest finite T), and for f16 the midpoints finer than its subnormal step 2^-24
LEFT_OUT = {F32: 7, F16: 172, BF16: 7}
VALUE = np.array([(-1.0 if c & 0x20 else 1.0) * R.code_value(c) for c in range(64)])   # code 0x20 is -0


def code_table(dtype):
    """every code at every position: element j of block i is the value of code (i + j) mod 64
    times 2^k; 32 consecutive codes hold exactly one of +-7.5, so block i's scale byte is 127 + k
    and its codes are the ones planted.  Returns (x, scale bytes, codes)."""
    codes = (np.arange(64)[:, None] + np.arange(32)[None, :]) % 64
    k = (np.arange(64) * 5) % (13 if dtype == F16 else 100) - (6 if dtype == F16 else 50)
    return VALUE[codes] * np.ldexp(1.0, k)[:, None], (127 + k).astype(np.uint8), codes.astype(np.uint8)


def step_t(v, dtype, d):
    """the T value d ulps from v (v != 0, a value of T), as float64"""
    t = NP.from_f32(v.astype(np.float32).ravel(), dtype)
    u = t.view(np.uint32 if dtype == F32 else np.uint16)
    return stored64((u.astype(np.int64) + d).astype(u.dtype).view(t.dtype), dtype).reshape(v.shape)


def tie_table(dtype):
    """per scale byte three blocks: a pin (the largest T value within the top binade of the scaled
    grid, 7.5 where T holds it) and the 31 midpoints between neighbouring magnitudes with
    alternating sign; the T values one ulp below; one ulp above.  A triple whose midpoint T cannot
    hold, or that is not below the pin, is zeroed in all three and counted.  Returns (x, count)."""
    mids = (R.GRID[:-1] + R.GRID[1:]) / 2 * np.where(np.arange(31) % 2, -1.0, 1.0)
    rows, left = [], 0
    for b in SCALE_BYTES[dtype]:
        s = 2.0 ** (b - 127)
        pins = [v for v in (7.5 * s, 7 * s, 6 * s, 4 * s, R.MAX_FINITE[dtype])
                if 3.75 * s < v <= 7.5 * s and v <= R.MAX_FINITE[dtype] and as_t(np.array([v]), dtype)[0] == v]
        m = mids * s
        ok = (as_t(m, dtype) == m) & (np.abs(m) < pins[0])
        ok &= np.abs(step_t(np.where(ok, m, 1.0), dtype, 1)) < pins[0]
        left += int((~ok).sum())
        safe = np.where(ok, m, 1.0)
        for d in (0, -1, 1):
            rows.append(np.concatenate([[pins[0]], np.where(ok, step_t(safe, dtype, d) if d else m, 0.0)]))
    return np.array(rows), left


@pytest.fixture(scope="module", params=[(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "sanitizers"])
def host_check(request, tmp_path_factory):
    """the stand-alone program (its own main, no GPU), plain and under the host address and
    undefined-behaviour sanitizers, under which a finding ends the program with a failure status"""
    exe = str(tmp_path_factory.mktemp("mxfp6") / "mxfp6_host_check")
    subprocess.run(["g++", "-O1", *request.param, "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp6_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_matches_the_reference(host_check, dtype):
    x1, want_scale, want_codes = code_table(dtype)
    assert np.array_equal(as_t(x1, dtype), x1)
    x2, left = tie_table(dtype)
    total = 31 * len(SCALE_BYTES[dtype])
    print(f"tie table dtype {dtype}: {left} of {total} triples not representable")
    assert left == LEFT_OUT[dtype] and np.array_equal(as_t(x2, dtype), x2)
    # (mxfp8's hostile blocks: NaN, +-Inf, -0, denormal, largest finite, 2^40 above the rest; and an all-zero block)
    x = np.concatenate([x1, x2, random_blocks(dtype, 3000, 61 + dtype), hostile_blocks(dtype), np.zeros((1, 32))])
    scale, codes = R.encode_blocks(x, dtype)
    # the program's encode of x, and its decode of those bytes and of 256 raw blocks: scale byte b, element j
    # of code (b + j) mod 64 -- every byte, every code at every position
    hs, hc = np.arange(256, dtype=np.uint8), ((np.arange(256)[:, None] + np.arange(32)[None, :]) % 64).astype(np.uint8)
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    got = np.frombuffer(run_host(host_check, ["encode", maxf], x.astype(np.float32).tobytes()), np.uint8).reshape(-1, 25)
    raw = np.concatenate([got, np.concatenate([hs[:, None], R.pack(hc)], axis=1)]).tobytes()
    got_dec = np.frombuffer(run_host(host_check, ["decode", maxf, str(dtype)], raw),
                            np.uint32 if dtype == F32 else np.uint16).reshape(-1, 32)
    got_scale, got_pay = got[:, 0], got[:, 1:]
    assert np.array_equal(got_scale, scale) and np.array_equal(got_pay, R.pack(codes))
    assert np.array_equal(got_scale[:64], want_scale) and np.array_equal(got_pay[:64], R.pack(want_codes))  # as planted
    want = R.decode_blocks(np.concatenate([scale, hs]), np.concatenate([codes, hc]), dtype)
    assert np.array_equal(got_dec, bits(want, dtype))
    # the program's decode(encode(x)), every element of every block with e > -127 and no clamp:
    # |x^ - x| <= max(|x| 2^-4, 2^(e - 4)), plus T's rounding of the decode
    e = got_scale.astype(np.int64) - 127
    ok = np.isfinite(x).all(axis=1) & (e > -127) & (np.abs(x).max(axis=1) < R.MAX_FINITE[dtype] / 2)
    assert ok.sum() > 3000
    err = np.abs(stored64(got_dec[:x.shape[0]].view(R.STORAGE[dtype]), dtype) - x)
    ulp_t = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dtype]
    bound = np.maximum(np.abs(x) * 2.0 ** -4, np.ldexp(1.0, e - 4)[:, None]) + np.abs(x) * ulp_t
    if dtype == F16:  # below 2^-14 f16's own step (2^-24) may exceed the codec's
        bound = np.maximum(bound, 2.0 ** -25)
    assert (err[ok] <= bound[ok]).all()


@pytest.mark.parametrize("pieces", range(1, 9))
def test_pieces_tile_both_regions_once(pieces):
    """mxfp6_pieces through bagua_centralized_piece_plan: the pieces' scale-byte ranges tile
    [0, sbytes) and their payload ranges [sbytes, segment) in order, at 24 bytes per block"""
    from bagua_core import _native as N
    assert N.COMPRESSION_MXFP6 == 5
    for cs, p in ((128 * 32 * 5 + 33, 2), (4096 * 9, 3), (100, 1)):
        sb, seg = R.scale_bytes(cs), R.segment_bytes(cs)
        for phase in (0, 1):
            at, prev = [0, sb], 0
            for q in range(pieces):
                b, e, r = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_size_t * 4)()
                n = N.C.bagua_centralized_piece_plan(5, F32, p, cs, pieces, q, phase, ctypes.byref(b), ctypes.byref(e), r)
                assert n == pieces and b.value == prev and (b.value, e.value) == R.piece_range(cs, pieces, q)
                prev = e.value
                if b.value == e.value:
                    continue
                assert [r[0], r[2]] == at and r[0] == b.value and r[2] == sb + 24 * b.value
                at = [r[1], r[3]]
                if e.value < R.blocks(cs):
                    assert at == [e.value, sb + 24 * e.value] and r[3] % 32 == 0
            assert prev == R.blocks(cs) and at == [sb, seg]
        assert N.K.bagua_mxfp6_compressed_bytes(cs, p) == p * seg == R.compressed_bytes(cs, p)
