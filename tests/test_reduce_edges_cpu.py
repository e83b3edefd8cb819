"""CPU cross-check of the crafted receive buffers (tests/segment_cases.py): the C oracle and
the numpy oracle, written independently, must give identical bytes for decompress,
reduce_chunks and compress(target) on every class x dtype x p x average x position, and
each class must produce what it is named for -- so that the GPU tests
(test_gpu_reduce_edges.py, test_gpu_ring_apply_edges.py) compare the kernels with values
two restatements of the reference agree on, and a mis-built case cannot pass as a trivial
one."""
import numpy as np
import pytest

import segment_cases as SC
from segment_cases import BF16, F16, F32

PS = [2, 5, 9]


def bits(x):
    return x.view(np.uint8)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("cls", ["benign"] + SC.CLASSES)
def test_oracles_agree_and_classes_are_what_they_say(oracle_c, cls, dtype):
    from oracle import oracle_np
    cs = SC.CS
    for p in PS:
        for k in SC.positions(p):
            recv = SC.crafted(cls, dtype, p, cs, k)
            assert recv.size == p * SC.stride(cs) and recv.size % p == 0
            for average in (0, 1):
                target = (k + 1) % p
                dc, rc, sc = SC.middle_step(oracle_c, recv, dtype, p, cs, target, average)
                dn, rn, sn = SC.middle_step(oracle_np, recv, dtype, p, cs, target, average)
                what = f"{cls} {SC.NAMES[dtype]} p={p} k={k} average={average}"
                assert np.array_equal(bits(dc), bits(dn)), f"decompress differs: {what}"
                assert np.array_equal(bits(rc), bits(rn)), f"reduce differs: {what}"
                assert np.array_equal(sc, sn), f"compress(target) differs: {what}"
                fc = SC.decode_segment(oracle_c, sc, dtype, cs)
                fn = SC.decode_segment(oracle_np, sn, dtype, cs)
                assert np.array_equal(bits(fc), bits(fn)), f"final decompress differs: {what}"
                check_class(cls, dtype, p, cs, k, average, recv, dc, rc, sc, what)


def check_class(cls, dtype, p, cs, k, average, recv, dec, red, seg, what):
    """The class produces what it is named for (read off the oracle's output)."""
    d = SC.to_f32(dec, dtype).reshape(p, cs)
    r = SC.to_f32(red, dtype)
    pay = recv.reshape(p, -1)[:, 32:32 + cs]
    hdr = SC.to_f32(SC.header_of(seg, dtype), dtype)
    if cls in ("benign", "payload_all_0", "payload_all_255", "constant", "inverted"):
        assert np.isfinite(d).all() and np.isfinite(r).all(), what
        assert hdr[0] <= r.min() and r.max() <= hdr[1] and hdr[0] == r.min() and hdr[1] == r.max(), what
    if cls in ("nan_min", "nan_max", "nan_both", "pos_inf_max", "both_inf"):
        assert np.isnan(d[k]).all() and np.isnan(r).all(), what
    elif cls == "neg_inf_min":
        assert np.all(d[k][pay[k] < 255] == -np.inf) and np.isnan(d[k][pay[k] == 255]).all(), what
        assert (pay[k] < 255).any() and (pay[k] == 255).any() and (r == -np.inf).any() and np.isnan(r).any(), what
    elif cls == "inverted":
        lo, hi = pay[k].argmin(), pay[k].argmax()
        assert d[k][lo] > 0.2 and d[k][hi] < -0.2, what  # negative scale: values fall as the byte rises
    elif cls == "empty_init":
        if dtype == F16:
            assert np.all(d[k] == -np.inf) and np.all(r == -np.inf), what
        else:
            assert np.isnan(d[k]).all() and np.isnan(r).all(), what
    elif cls == "constant":
        assert np.all(np.abs(d[k] - 0.5) <= 2e-7), what
    elif cls == "huge_range":
        if dtype == F16:
            assert np.isfinite(d[:, :32]).all() and np.all(np.abs(d[:, :32]) > 65000), what
            if average:
                assert np.isfinite(r[:32]).all(), what
            else:  # the p-fold sum overflows f16
                assert np.all(r[:16] == np.inf) and np.all(r[16:32] == -np.inf), what
        else:
            assert np.all(d[k][pay[k] < 255] == -np.inf) and np.isnan(d[k][pay[k] == 255]).all(), what
            assert (r == -np.inf).any(), what
    elif cls == "denormal":
        tiny_normal = {F32: 2.0 ** -126, F16: 2.0 ** -14, BF16: 2.0 ** -126}[dtype]
        assert np.isfinite(r).all(), what
        zero_sign = np.signbit(r[r == 0])
        assert (~zero_sign).any() and np.all(r[:32] == 0) and not np.signbit(r[:32]).any(), what
        if dtype == F16:
            if average:  # -0: the mean of one smallest denormal underflowed
                assert zero_sign.any() and np.signbit(r[32:64]).all() and np.all(r[32:64] == 0), what
            else:
                assert np.all(r[32:64] == -2.0 ** -24), what
            assert ((r != 0) & (np.abs(r) < tiny_normal)).any(), what  # denormals of f16
            assert ((d != 0) & (np.abs(d) < tiny_normal)).any(), what
        else:
            # the format cannot carry a denormal or a -0 of f32 / bf16 (segment_cases.py): the
            # smallest magnitudes it does carry
            assert not zero_sign.any() and np.all(r[32:64] < 0) and np.all(r[32:64] > -1e-7), what
            assert np.all(np.abs(r[r != 0]) >= tiny_normal), what
    elif cls == "signed_zero_min":
        assert np.isfinite(r).all() and np.all(r[:32] == 0) and not np.signbit(r[:32]).any(), what
        neg = np.arange(32, 64) % 4 != 0
        if dtype == F16 and average:  # {+0, -0, positive denormals}: the minimum is -0
            assert np.all(r >= 0) and (r > 0).any() and np.all(r[32:64] == 0), what
            assert np.array_equal(np.signbit(r[32:64]), neg) and np.signbit(r).sum() == neg.sum(), what
            assert SC.header_of(seg, dtype).view(np.uint16)[0] == 0x8000 and hdr[1] > 0, what
        elif dtype == F16:
            assert np.all(r[32:64][neg] == -2.0 ** -24) and not np.signbit(r[r == 0]).any(), what
        else:
            assert not np.signbit(r[r == 0]).any(), what
    elif cls == "inf_cancel":
        k2 = (k + 1) % p
        h = cs // 2
        assert np.all(d[k][:h] == -np.inf) and np.all(d[k2][:h] == np.inf) and np.isnan(r[:h]).all(), what
    elif cls == "every_segment_nan":
        assert np.isnan(d).all() and np.isnan(r).all(), what
        assert np.array_equal(SC.header_of(seg, dtype), SC.init_header(dtype)), what
    elif cls == "payload_all_0":
        assert np.all(d[k] == d[k][0]) and abs(d[k][0] + 1e-3) < 2e-5, what
    elif cls == "payload_all_255":
        assert np.all(d[k] == d[k][0]) and abs(d[k][0] - 1e-3) < 2e-5, what
