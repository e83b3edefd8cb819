"""CPU tests of the MXFP4 boundary table (tests/mxfp4_boundary_cases.py): the table does what
it claims, on the numpy reference (tests/mxfp4_reference.py) and on the kernels' block
arithmetic compiled for the host (tools/mxfp4_host_check.cpp).  No GPU.

Two things the table cannot do, both by the scale rule itself (MXFP4.md): any |x| in
(3, 6] * 2^e gives the scale byte e + 127, so in the HIGH blocks, which hold the 3.5 and 5.0
triples, the byte is held by those elements as well as by the pin; and every amax below
2^-124 gives byte 0, so at byte 0 no element can move it.  `test_the_pin_decides_the_scale_byte`
checks every other block."""
import math
import os
import subprocess

import numpy as np
import pytest

import mxfp4_boundary_cases as B
import mxfp4_ef_reference as REF
import mxfp4_reference as R
from oracle import oracle_np as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]


def nibbles(payload):
    nib = np.empty((payload.shape[0], 32), np.uint8)
    nib[:, 0::2], nib[:, 1::2] = payload & 15, payload >> 4
    return nib


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mxfp4_boundary") / "mxfp4_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp4_host_check.cpp"), "-o", exe], check=True)
    return exe


# ---------------------------------------------------------------- the table ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_shape_and_classes(dtype):
    t = B.table(dtype)
    assert t.x.size == 32 * t.nb and t.x.dtype == B.STORAGE[dtype]
    # three chunks of whole blocks; a ragged last wave tile (64 / 128 blocks); past the start of the
    # second grid-stride iteration of a two-workgroup encode (8 wave tiles)
    assert t.nb % 3 == 0 and t.nb % 128 != 0 and t.nb % 64 != 0
    assert t.nb > 8 * (64 if dtype == F32 else 128)
    assert t.nb * 32 <= 38000
    v = t.values()
    assert np.isfinite(v).all() and not (np.signbit(v) & (v == 0)).any(), "no -0, no inf, no NaN"
    pinned = np.isin(t.cls, (B.LOW, B.HIGH))
    assert sorted(set(t.byte[pinned])) == list(B.BYTES[dtype])
    assert (t.cls == B.EDGE).sum() >= 24 and (t.cls == B.PLANTED).sum() >= 96
    # the pin visits all 32 positions in each class, and is the block's amax
    for cls in (B.LOW, B.HIGH, B.PLANTED):
        assert set(t.pin_pos[t.cls == cls]) == set(range(32))
    rows = np.arange(t.nb)
    assert (np.abs(v[rows, t.pin_pos]) == np.abs(v).max(axis=1)).all()
    assert (t.kind[rows, t.pin_pos] == B.PIN).all()
    # every class of element reaches every position of a 16-byte vector and every nibble of a payload word
    for i in range(len(B.BOUNDARIES)):
        for side in B.SIDES:
            for neg in (False, True):
                at = np.nonzero((t.kind == B.BOUNDARY) & (t.bnd == i) & (t.side == side) & (np.signbit(v) == neg)
                                & (v != 0))[1]
                assert set(at % 8) == set(range(8)), (i, side, neg)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_bytes_are_the_ones_built_for(dtype):
    t = B.table(dtype)
    scale, _ = R.encode_blocks(t.values(), dtype)
    bad = np.nonzero(scale != t.byte)[0]
    assert bad.size == 0, (bad[:8], scale[bad[:8]], t.byte[bad[:8]])
    # the edge class: the two pins of an exponent lie one scale byte apart unless both clamp to 0
    pins = B.edge_pins(dtype)
    for (a, ba), (b, bb) in zip(pins[0:-2:2], pins[1:-2:2]):
        assert b > a and (bb == ba + 1 or (ba == 0 and bb <= 1))
        assert math.frexp(a)[0] == 0.75 and b == t_neighbours(a, dtype)[1] and t_value(a, dtype) and t_value(b, dtype)
    assert len(pins) >= 26 and {ba for _, ba in pins} >= ({102, 125, 126, 140, 141} if dtype == F16 else {0, 125, 126, 252, 253})
    assert pins[-2][0] == math.ldexp(1.0, B.EMIN[dtype]) and pins[-1][0] < pins[-2][0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pin_decides_the_scale_byte(dtype):
    """without its pin a block gets another scale byte: in every LOW, edge and planted block above
    byte 0 (module docstring: not the HIGH blocks, not byte 0); in the planted blocks it moves by 2"""
    t = B.table(dtype)
    scale, _ = R.encode_blocks(t.without_pins(), dtype)
    must = np.isin(t.cls, (B.LOW, B.EDGE, B.PLANTED)) & (t.byte > 0)
    assert must.sum() > 0.45 * t.nb
    same = np.nonzero(must & (scale == t.byte))[0]
    assert same.size == 0, (same[:8], t.byte[same[:8]], t.cls[same[:8]])
    planted = t.cls == B.PLANTED
    assert (t.byte[planted].astype(np.int64) - scale[planted] == 2).all()
    # and in the HIGH blocks the elements beside the pin all lie at or below it
    assert (scale <= t.byte).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoding_and_encoding_again(dtype):
    """MXFP4.md: the same values bit for bit; the same bytes unless the block's amax rounded down to
    3 * 2^e, which the scale rule puts one byte lower (the edge class's upper pins are such blocks)"""
    t = B.table(dtype)
    s1, p1 = R.encode_blocks(t.values(), dtype)
    d1 = R.decode_blocks(s1, p1, dtype)
    s2, p2 = R.encode_blocks(NP.to_f32(d1.ravel(), dtype).astype(np.float64).reshape(-1, 32), dtype)
    d2 = R.decode_blocks(s2, p2, dtype)
    assert np.array_equal(d1.view(B.BITS[dtype]), d2.view(B.BITS[dtype]))
    top = (nibbles(p1) & 7).max(axis=1)
    moved = s1 != s2
    assert moved.any() and (top[moved] <= 5).all() and (s1[moved] - s2[moved] >= 1).all()
    assert np.array_equal(p1[top == 7], p2[top == 7]) and not moved[top >= 6].any()


def t_neighbours(v, dtype):
    """the next T values below and above v > 0, from T's exponent range and significand width"""
    m, k = math.frexp(v)
    up = math.ldexp(1.0, max(k - 1, B.EMIN[dtype]) - B.MANT[dtype])
    down = math.ldexp(1.0, max(k - 1 if m > 0.5 else k - 2, B.EMIN[dtype]) - B.MANT[dtype])
    return v - down, v + up


def t_value(v, dtype):
    with np.errstate(over="ignore"):
        back = float(NP.to_f32(NP.from_f32(np.array([v], np.float32), dtype), dtype)[0])
    return math.isfinite(back) and back == v


def expected_left_out(dtype):
    """not a finite T value, or above the pin -- the pin restated: 6 * 2^e, else 4 * 2^e, else the largest finite T"""
    out = set()
    for byte in B.BYTES[dtype]:
        e = byte - 127
        pin = next((c * 2.0 ** e for c in (6.0, 4.0) if t_value(c * 2.0 ** e, dtype)), R.MAX_FINITE[dtype])
        for i, c in enumerate(B.BOUNDARIES):
            v = c * 2.0 ** e
            if not t_value(v, dtype) or v > pin:
                out |= {(byte, i, s) for s in B.SIDES}
                continue
            lo, hi = t_neighbours(v, dtype)
            assert t_value(lo, dtype) and lo < v
            if not t_value(hi, dtype) or hi > pin:
                out.add((byte, i, 1))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_left_out_set(dtype):
    t = B.table(dtype)
    assert set(t.left_out) == expected_left_out(dtype)
    # the cap: nothing is left out for f32 and bf16 at bytes 0 to 252, nothing for f16 at bytes 105 to 140
    lo, hi = (105, 140) if dtype == F16 else (0, 252)
    assert not [x for x in t.left_out if lo <= x[0] <= hi]
    whole = {(byte, i) for byte, i, _ in t.left_out}
    if dtype == F16:  # 25 of the 287 (byte, boundary) pairs
        assert len(whole) == 25 and len(t.left_out) == 75
    else:             # boundary 5.0 under byte 253
        assert whole == {(253, 6)} and len(t.left_out) == 3
    # every triple that is not left out is in the table, for both signs
    v = t.values()
    have = set()
    for b, j in zip(*np.nonzero(t.kind == B.BOUNDARY)):
        have.add((int(t.byte[b]), int(t.bnd[b, j]), int(t.side[b, j]), bool(v[b, j] < 0)))
    for byte in B.BYTES[dtype]:
        for i in range(len(B.BOUNDARIES)):
            for s in B.SIDES:
                if (byte, i, s) in t.left_out:
                    continue
                zero = dtype == F16 and byte == 105 and i == 0 and s == -1  # below the smallest f16: +0
                assert (byte, i, s, False) in have and (zero or (byte, i, s, True) in have), (byte, i, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_elements_and_their_nibbles(dtype):
    """every boundary element is what it is described as, and the reference gives the lower code below
    the boundary, the upper code above it and the even code at it: a kernel that rounds ties away
    from zero, or truncates, differs from the reference on this table"""
    t = B.table(dtype)
    v = t.values()
    scale, payload = R.encode_blocks(v, dtype)
    nib = nibbles(payload)
    lower, upper, even = np.array(B.LOWER_CODE), np.array(B.UPPER_CODE), np.array(B.EVEN_CODE)
    bs, js = np.nonzero(t.kind == B.BOUNDARY)
    assert bs.size > 15 * t.nb
    i, s = t.bnd[bs, js].astype(np.int64), t.side[bs, js]
    a = np.abs(v[bs, js])
    exact = np.ldexp(np.array(B.BOUNDARIES)[i], t.byte[bs] - 127)
    for k in range(bs.size):
        lo, hi = t_neighbours(exact[k], dtype)
        assert a[k] == (lo, exact[k], hi)[s[k] + 1], (t.byte[bs[k]], i[k], s[k])
    want = np.where(s < 0, lower[i], np.where(s > 0, upper[i], even[i]))
    sign = np.where(np.signbit(v[bs, js]), 8, 0)
    assert np.array_equal(nib[bs, js], want | sign)
    # the two wrong roundings a kernel could have differ on the table
    away = np.where(s < 0, lower[i], upper[i])
    trunc = np.where(s > 0, upper[i], lower[i])
    assert (away != want).sum() > 1000 // (8 if dtype == F16 else 1) and (trunc != want).sum() > 1000 // (8 if dtype == F16 else 1)
    # every code and both signs are produced at the lowest two bytes
    for byte in list(B.BYTES[dtype])[:2] if dtype != F16 else [105, 106]:
        at = nib[t.byte == byte]
        assert set(at.ravel()) >= set(range(1, 8)) | set(range(9, 16)), byte


# ------------------------------------------------------- the host arithmetic ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_on_the_table(host_check, dtype):
    """the `encode` and `ef` modes of mxfp4_host_check give the reference's bytes and residuals"""
    t = B.table(dtype)
    x32 = t.values().astype(np.float32)
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    scale, payload = R.encode_blocks(t.values(), dtype)
    got = subprocess.run([host_check, "encode", maxf], input=x32.tobytes(), capture_output=True, check=True).stdout
    got = np.frombuffer(got, np.uint8).reshape(-1, 17)
    assert np.array_equal(got[:, 0], scale) and np.array_equal(got[:, 1:], payload)
    e32 = np.zeros_like(x32)
    for step in range(2):  # the second step's residual is the first's
        s_ref, p_ref, e_ref = REF.ef_blocks(x32, e32, dtype)
        raw = np.concatenate([x32, e32], axis=1).astype(np.float32).tobytes()
        out = subprocess.run([host_check, "ef", maxf, str(dtype)], input=raw, capture_output=True, check=True).stdout
        rec = np.frombuffer(out, np.uint8).reshape(-1, 17 + 128)
        assert np.array_equal(rec[:, 0], s_ref) and np.array_equal(rec[:, 1:17], p_ref), step
        e_got = np.ascontiguousarray(rec[:, 17:]).view(np.uint32).reshape(-1, 32)
        assert np.array_equal(e_got, e_ref.view(np.uint32)), step
        if step == 0:
            assert np.array_equal(s_ref, scale) and np.array_equal(p_ref, payload), "zero state: the plain codec's bytes"
            assert e_ref.any()
        e32 = e_ref


# ----------------------------------------------------- middle-step inputs ----
def reduced(m):
    """the reference's reduce (sum mode) of the decoded segments, as float64, and each decoded part"""
    t = np.zeros(m.p * m.cs, R.STORAGE[m.dtype])
    R.decompress(m.recv, m.p, t, m.dtype)
    parts = NP.to_f32(t, m.dtype).astype(np.float64).reshape(m.p, -1, 32)
    NP.reduce_chunks(t, m.dtype, m.p, 0, False)
    return NP.to_f32(t[:m.cs], m.dtype).astype(np.float64).reshape(-1, 32), parts


def check_middle_nibbles(m, got):
    scale, payload = R.encode_blocks(got, m.dtype)
    assert np.array_equal(scale, m.byte)
    nib = nibbles(payload)
    bs, js = np.nonzero(m.bnd >= 0)
    i, s = m.bnd[bs, js].astype(np.int64), m.side[bs, js]
    want = np.where(s < 0, np.array(B.LOWER_CODE)[i], np.where(s > 0, np.array(B.UPPER_CODE)[i], np.array(B.EVEN_CODE)[i]))
    assert np.array_equal(nib[bs, js] & 7, want)
    assert np.array_equal(nib[bs, js] >> 3, np.signbit(got[bs, js]).astype(np.uint8))
    return bs, js, i, s


@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_exact_inputs(dtype):
    m = B.middle_exact(dtype)
    assert m.p == 2 and m.recv.size == 2 * R.segment_bytes(m.cs)
    got, parts = reduced(m)
    assert np.array_equal(parts, m.parts), "every part decodes, as T stores it, to the value meant"
    assert np.array_equal(got, m.want)
    bs, js, i, s = check_middle_nibbles(m, got)
    assert (s == 0).all()
    assert np.array_equal(np.abs(got[bs, js]), np.ldexp(np.array(B.BOUNDARIES)[i], m.byte[bs] - 127))
    # every boundary with both signs at every output byte, the lowest and the highest reachable under a
    # pin of 6 included (a block of byte 0 has no lower byte for the odd quarters: form B only)
    bytes_ = sorted(set(m.byte))
    assert bytes_ == list(B.MIDDLE_EXACT_BYTES[dtype]) and len(bytes_) >= 12
    assert bytes_[-1] == (140 if dtype == F16 else 252) and bytes_[0] == (104 if dtype == F16 else 0)
    for byte in bytes_:
        seen = {(int(a), bool(n)) for a, n in zip(i[m.byte[bs] == byte], got[bs, js][m.byte[bs] == byte] < 0)}
        need = (4, 5, 6) if byte == bytes_[0] else range(7)
        assert seen >= {(a, n) for a in need for n in (False, True)}, byte
    for word in range(4):  # the one-lane encode's four payload words each see a tie
        assert ((js // 8) == word).any()


def test_middle_neighbour_inputs():
    """p = 3, f32: (segment 0 + segment 2) + segment 1 is exact at both adds and is the boundary's
    one-ulp neighbour"""
    m = B.middle_neighbours()
    assert m.p == 3 and m.dtype == F32
    got, parts = reduced(m)
    assert np.array_equal(parts, m.parts)
    first = parts[0] + parts[2]  # float64: exact
    assert np.array_equal(first.astype(np.float32).astype(np.float64), first), "the tree's intermediate sum is exact"
    assert np.array_equal(got, first + parts[1]) and np.array_equal(got, m.want)
    bs, js, i, s = check_middle_nibbles(m, got)
    exact = np.ldexp(np.array(B.BOUNDARIES)[i], m.byte[bs] - 127).astype(np.float32)
    toward = np.where(s < 0, np.float32(0), np.float32(np.inf)).astype(np.float32)
    want = np.where(s == 0, exact, np.nextafter(exact, toward))
    assert np.array_equal(np.abs(got[bs, js]), want.astype(np.float64))
    for byte in set(m.byte):
        seen = {(int(a), int(b)) for a, b in zip(i[m.byte[bs] == byte], s[m.byte[bs] == byte])}
        assert seen >= {(a, b) for a in range(7) for b in (-1, 1)}, byte
    assert min(m.byte) == 26 and max(m.byte) == 252 and {126, 127, 128} <= set(m.byte)
