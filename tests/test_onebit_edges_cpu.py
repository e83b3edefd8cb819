"""CPU cross-check of the crafted 1-bit receive buffers (tests/onebit_segment_cases.py): the C
oracle and the numpy oracle, written independently, must give identical bytes for
decompress_onebit, reduce_chunks and compress_onebit(target) on every class x dtype x p x
average x position, and each class must produce what it is named for -- so that
test_gpu_onebit_recv_edges.py compares the kernels with values two restatements of the
format agree on, and a mis-built case cannot pass as a trivial one.

Where a class cannot do what its name says for some dtype, check_class asserts what it does
instead: denormal_f32 decodes to +-0 in f16 (1e-40 is below half of f16's smallest denormal)
and to the denormal 2^-133 in bf16; denormal_16 is a denormal in f16 only; overflow_16 decodes
to a finite value in f32, where every segment carries it and the sum overflows instead;
inf_cancel at p = 1 has no second segment and stays +-inf."""
import numpy as np
import pytest

import onebit_segment_cases as OS
from onebit_segment_cases import BF16, F16, F32

PS = [2, 5, 9]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_floats(a, b, dtype, cls):
    """Byte for byte -- except in every_segment_nan, where NaN is added to NaN: IEEE 754 leaves
    open which operand's sign and payload the sum takes (the C loop and numpy's vector loop
    differ), so there the values must agree in NaN-ness and, where not NaN, in every bit."""
    if cls != "every_segment_nan":
        return np.array_equal(bits(a), bits(b))
    fa, fb = OS.to_f32(a, dtype), OS.to_f32(b, dtype)
    na, nb = np.isnan(fa), np.isnan(fb)
    return np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("cls", ["benign"] + OS.CLASSES)
def test_oracles_agree_and_classes_are_what_they_say(oracle_c, cls, dtype):
    from oracle import oracle_np
    cs = OS.CS
    for p in PS:
        for k in OS.positions(p):
            recv = OS.crafted(cls, dtype, p, cs, k)
            assert recv.size == oracle_c.onebit_compressed_size(p, cs) and recv.size % p == 0
            target = (k + 1) % p
            for average in (0, 1):
                with np.errstate(all="ignore"):
                    dc, rc, sc = OS.middle_step(oracle_c, recv, dtype, p, cs, target, average)
                    dn, rn, sn = OS.middle_step(oracle_np, recv, dtype, p, cs, target, average)
                what = f"{cls} {OS.NAMES[dtype]} p={p} k={k} average={average}"
                assert np.array_equal(bits(dc), bits(dn)), f"decompress differs: {what}"
                assert same_floats(rc, rn, dtype, cls), f"reduce differs: {what}"
                assert np.array_equal(sc, sn), f"compress(target) differs: {what}"
                check_class(oracle_c, cls, dtype, p, cs, k, average, recv, dc, rc, sc, what)


def test_p1_and_inf_cancel_alone(oracle_c):
    """p = 1 (used by the GPU decode and middle-step tests): both oracles agree, and inf_cancel
    without a second segment decodes to +-inf"""
    from oracle import oracle_np
    for dtype in (F32, F16, BF16):
        for cls in OS.CLASSES:
            recv = OS.crafted(cls, dtype, 1, OS.CS, 0)
            for average in (0, 1):
                with np.errstate(all="ignore"):
                    a = OS.middle_step(oracle_c, recv, dtype, 1, OS.CS, 0, average)
                    b = OS.middle_step(oracle_np, recv, dtype, 1, OS.CS, 0, average)
                assert np.array_equal(bits(a[0]), bits(b[0])) and same_floats(a[1], b[1], dtype, cls) and \
                    np.array_equal(a[2], b[2]), (cls, dtype, average)
            if cls == "inf_cancel":
                assert np.isinf(OS.to_f32(a[1], dtype)).all()


def check_class(backend, cls, dtype, p, cs, k, average, recv, dec, red, seg, what):
    """The class produces what it is named for (read off the oracle's output)."""
    d = OS.to_f32(dec, dtype).reshape(p, cs)
    r = OS.to_f32(red, dtype)
    b = OS.bits_of(recv, p, cs)          # [p][tiles * 1024], padding included
    bk = b[k][:cs]
    nb = OS.tiles_of(cs) * OS.TILE_BYTES
    out_bits = OS.unpack_bits(seg[32:32 + nb])
    out_scale = seg[:4].view(np.float32)[0]
    tiny_normal = {F32: 2.0 ** -126, F16: 2.0 ** -14, BF16: 2.0 ** -126}[dtype]
    assert bk.any() and not bk.all() or cls in ("bits_all_0", "bits_all_1"), what
    # in every class: the re-encoded bit is "reduced value < 0", padding bits are 0, bytes 8..31 too
    assert np.array_equal(out_bits[:cs], r < 0) and not out_bits[cs:].any() and not seg[8:32].any(), what
    assert seg[4:8].view(np.uint32)[0] == cs and not seg[32 + nb:].any(), what
    if cls in ("benign", "neg_scale", "bits_all_0", "bits_all_1", "bits_marker", "padding_bits_set",
               "garbage_header", "equal_cancel", "denormal_f32", "denormal_16", "zero_scale", "neg_zero_scale"):
        assert np.isfinite(d).all() and np.isfinite(r).all() and np.isfinite(out_scale) and out_scale > 0, what
    if cls == "nan_scale":
        assert np.isnan(d[k]).all() and np.isnan(r).all() and np.isnan(out_scale) and not out_bits.any(), what
    elif cls == "neg_scale":
        assert np.all(d[k][~bk] < 0) and np.all(d[k][bk] > 0), what
    elif cls in ("neg_zero_scale", "zero_scale"):
        assert np.all(d[k] == 0), what
        assert np.array_equal(np.signbit(d[k]), ~bk if cls == "neg_zero_scale" else bk), what
    elif cls in ("pos_inf", "neg_inf"):
        s = np.inf if cls == "pos_inf" else -np.inf
        assert np.all(d[k][~bk] == s) and np.all(d[k][bk] == -s), what
        assert np.all(np.isinf(r)) and (r > 0).any() and (r < 0).any() and np.isinf(out_scale), what
    elif cls == "inf_cancel":
        k2 = (k + 1) % p
        agree = bk == b[k2][:cs]
        assert np.all(d[k][~bk] == np.inf) and np.all(d[k2][~b[k2][:cs]] == -np.inf), what
        assert agree.any() and (~agree).any() and np.array_equal(np.isnan(r), agree), what
        assert np.isnan(out_scale), what
    elif cls == "denormal_f32":
        if dtype == F16:  # 1e-40 < 2^-25: rounds to zero, the sign kept
            assert np.all(d[k] == 0) and np.array_equal(np.signbit(d[k]), bk), what
        else:
            assert np.all(d[k] != 0) and np.all(np.abs(d[k]) < tiny_normal), what
            if dtype == BF16:
                assert np.all(np.abs(d[k]) == 2.0 ** -133), what
    elif cls == "denormal_16":
        if dtype == F16:
            assert np.all(np.abs(d[k]) == 2.0 ** -24), what
        else:
            assert np.all(np.abs(d[k]) >= tiny_normal) and np.all(np.abs(d[k]) < 4e-8), what
    elif cls == "overflow_16":
        if dtype == F32:  # finite in f32; every segment carries it and the sum overflows
            assert np.isfinite(d).all() and np.all(np.abs(d) > 3.3e38), what
            assert np.isinf(r).any() and (r == np.inf).any() and (r == -np.inf).any(), what
        else:
            assert np.all(d[k][~bk] == np.inf) and np.all(d[k][bk] == -np.inf), what
            assert np.isinf(r).all(), what
    elif cls == "equal_cancel":
        assert np.all(np.abs(d) == np.abs(d[0][0])) and d[0][0] != 0, what
        if p % 2 == 0:
            z = r == 0
            assert z.sum() > cs // 8 and not np.signbit(r[z]).any() and not out_bits[:cs][z].any(), what
    elif cls == "every_segment_nan":
        assert np.isnan(d).all() and np.isnan(r).all() and np.isnan(out_scale) and not out_bits.any(), what
    elif cls == "bits_all_0":
        assert not bk.any() and np.all(d[k] == d[k][0]) and d[k][0] > 0, what
    elif cls == "bits_all_1":
        assert bk.all() and np.all(d[k] == d[k][0]) and d[k][0] < 0, what
    elif cls == "bits_marker":
        co = recv.size // p
        tiles = OS.tiles_of(cs)
        for c in range(p):
            f = recv[c * co + 32:c * co + 32 + nb].view("<u2").reshape(tiles, 64)
            lane, t = 5, tiles - 1
            assert f[t][lane] == (lane * 73 + t * 11 + c * 4099) & 0xffff and f[0][0] == (c * 4099) & 0xffff, what
        # element 0 of tile 0 is bit 0 of lane 0's field: negative where c * 4099 is odd
        assert np.array_equal(d[:, 0] < 0, np.arange(p) % 2 == 1), what
        assert len({b[c][:cs].tobytes() for c in range(p)}) == p, what
    elif cls == "padding_bits_set":
        assert cs % OS.TILE and b[:, cs:].all(), what
        # the scale is the mean over cs elements of |reduced|: padding contributes nothing
        assert out_scale == np.float32(backend.onebit_tree_sum(np.abs(r))) / np.float32(cs), what
    elif cls == "garbage_header":
        co = recv.size // p
        clean = recv.copy()
        for c in range(p):
            assert recv[c * co + 4:c * co + 8].view(np.uint32)[0] == 0xFFFFFFFF and recv[c * co + 8:c * co + 32].all()
            clean[c * co + 4:c * co + 32] = 0
        assert np.array_equal(bits(OS.decode(backend, clean, dtype, p, cs)), bits(dec)), what
