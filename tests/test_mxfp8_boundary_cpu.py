"""CPU tests of the MXFP8 boundary table (tests/mxfp8_boundary_cases.py): the table is what it
says it is, the numpy reference gives every block its byte and every tie and neighbour its
code, and the kernels' host arithmetic (tools/mxfp8_host_check.cpp) agrees byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import mxfp8_boundary_cases as B
import mxfp8_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [B.F32, B.F16, B.BF16]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mxfp8b") / "mxfp8_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp8_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("dtype", DTYPES)
def test_table_shape_and_coverage(dtype):
    t = B.table(dtype)
    assert t.x.size == t.nb * 32 and t.nb % 3 == 0 and t.nb % 128 != 0
    assert t.x.size <= 260_000
    # every scale byte a finite T can produce is pinned, and all 126 ties stand under the two
    # lowest bytes that hold them all, the two highest and at least a dozen between
    pinned = t.cls == B.PINNED
    assert set(t.byte[pinned]) == set(B.BYTES[dtype])
    full = []
    for byte in B.BYTES[dtype]:
        blk = pinned & (t.byte == byte)
        ties = t.tie[blk][(t.kind[blk] == B.TIE) & (t.side[blk] == 0)]
        signs = t.code[blk][(t.kind[blk] == B.TIE) & (t.side[blk] == 0)] >> 7
        if set(zip(ties, signs)) == {(i, s) for i in range(126) for s in (0, 1)}:
            full.append(byte)
    # (where T is coarse -- f16's denormal range, the lowest bytes of f32 and bf16 -- some ties are no T values)
    assert len(full) >= 16 and full[-1] == B.BYTES[dtype][-1] - 1 and full[-2] == B.BYTES[dtype][-1] - 2, full
    # the pin and the planted maximum visit all 32 positions
    assert set(t.pin_pos[pinned]) == set(range(32))
    assert set(t.pin_pos[t.cls == B.PLANTED]) == set(range(32))
    assert (t.cls == B.EDGE).sum() >= 24
    print(f"dtype {dtype}: {t.nb} blocks, {t.x.size} elements, {t.left_out} (byte, tie, side, sign) "
          f"triples T cannot represent under their pin; all ties under bytes {full[0]}..{full[-1]}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_on_the_table(dtype):
    t = B.table(dtype)
    v = t.values()
    scale, payload = R.encode_blocks(v, dtype)
    # every block gets its byte
    assert np.array_equal(scale, t.byte)
    # the pin decides it
    s0, _ = R.encode_blocks(t.without_pins(), dtype)
    assert (s0[t.pin_decides] < t.byte[t.pin_decides]).all()
    assert t.pin_decides[t.cls == B.PLANTED].all() and (s0[t.cls == B.PLANTED] == t.byte[t.cls == B.PLANTED] - 2).all()
    assert t.pin_decides.sum() > t.nb // 3
    pins = np.abs(v[np.arange(t.nb), t.pin_pos])
    assert (pins == np.abs(v).max(axis=1)).all()
    # every tie and neighbour gets its code
    m = t.kind == B.TIE
    assert np.array_equal(payload[m], t.code[m].astype(np.uint8))
    assert m.sum() > 0.8 * t.x.size * 31 / 32 * (t.cls == B.PINNED).mean()
    # edge blocks: 1.75 * 2^j and the next T value above it lie one scale byte apart
    e = np.nonzero(t.cls == B.EDGE)[0]
    assert (np.diff(t.byte[e][:-2].reshape(-1, 2), axis=1) >= 0).all()
    # and the decode of the encode is idempotent on the table
    d = R.decode_blocks(scale, payload, dtype)
    s2, p2 = R.encode_blocks(B.NP.to_f32(d.ravel(), dtype).astype(np.float64).reshape(-1, 32), dtype)
    bits = np.uint32 if dtype == B.F32 else np.uint16
    assert np.array_equal(R.decode_blocks(s2, p2, dtype).view(bits), d.view(bits))


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_on_the_table(host_check, dtype):
    t = B.table(dtype)
    v = t.values()
    scale, payload = R.encode_blocks(v, dtype)
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    got = subprocess.run([host_check, "encode", maxf], input=v.astype(np.float32).tobytes(), capture_output=True,
                         check=True).stdout
    got = np.frombuffer(got, np.uint8).reshape(-1, 33)
    assert np.array_equal(got[:, 0], scale)
    assert np.array_equal(got[:, 1:], payload)
    raw = np.concatenate([scale[:, None], payload], axis=1).astype(np.uint8).tobytes()
    dec = subprocess.run([host_check, "decode", maxf, str(dtype)], input=raw, capture_output=True, check=True).stdout
    bits = np.uint32 if dtype == B.F32 else np.uint16
    assert np.array_equal(np.frombuffer(dec, bits).reshape(-1, 32), R.decode_blocks(scale, payload, dtype).view(bits))
