"""GPU tests of the MXFP8 kernels on the boundary table (tests/mxfp8_boundary_cases.py): every
tie of the E4M3 grid and its one-ulp neighbours under every scale byte, the edges of the scale
rule and the planted maxima go through the encode, the decode and the fused middle step, byte
for byte against the numpy reference -- with the hardware conversions and with the arithmetic
(BAGUA_MXFP8_HWCVT is read at every launch, so the switch is set in this process), on the
vector and the guarded paths (a view offset by one element), under the default grid and under
a grid of two workgroups.  And all 256 scale bytes x 256 element bytes are decoded."""
import numpy as np
import pytest
import torch

import mxfp8_boundary_cases as B
import mxfp8_reference as R
from test_gpu_multirank import dev, host
from test_gpu_mxfp8 import DTYPES, GRID_KNOBS, OK, TORCH, dev_at, same_bytes, u8

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(scope="module")
def reference():
    """per dtype, computed once: the table as three chunks, its compressed bytes and their decode"""
    out = {}
    for dtype in DTYPES:
        x = B.table(dtype).x
        comp = R.compress(x, dtype, 3)
        comp.setflags(write=False)
        dec = R.decompress(comp, 3, np.zeros(x.size, R.STORAGE[dtype]), dtype)
        dec.setflags(write=False)
        out[dtype] = (x, comp, dec)
    return out


@pytest.mark.parametrize("two_workgroups", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("hw", ["1", "0"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_table_through_encode_and_decode(bc, reference, dtype, hw, offset, two_workgroups, monkeypatch):
    K = bc._native.K
    monkeypatch.setenv("BAGUA_MXFP8_HWCVT", hw)
    if two_workgroups:
        for k in GRID_KNOBS:
            monkeypatch.setenv(k, "6")  # the cap is shared by the three chunks: two workgroups each
    x, comp, dec = reference[dtype]
    p, cs, S = 3, x.size // 3, comp.size
    what = f"dtype={dtype} hw={hw} offset={offset} two_workgroups={two_workgroups}"
    xt = dev_at(x, dtype, offset)
    out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp8_compress(dtype, xt.data_ptr(), x.size, cs, p, out.data_ptr(), S, -1, None) == OK
    got = u8(out)
    same_bytes(got, comp, f"{what}: encode")
    # what the table promises, on the GPU's bytes themselves: every block its byte, every tie its code
    t = B.table(dtype)
    nb, sb, seg = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    segs = got.reshape(p, seg)
    assert np.array_equal(segs[:, :nb].ravel(), t.byte)
    pay = segs[:, sb:sb + 32 * nb].reshape(-1, 32)
    m = t.kind == B.TIE
    assert np.array_equal(pay[m], t.code[m].astype(np.uint8))
    ct = torch.from_numpy(np.array(comp)).cuda()
    back = dev_at(np.zeros_like(x), dtype, offset)
    back.fill_(7.0)
    assert K.bagua_mxfp8_decompress(dtype, ct.data_ptr(), S, cs, p, back.data_ptr(), None) == OK
    same_bytes(host(back, dtype), dec, f"{what}: decode")


@pytest.mark.parametrize("two_workgroups", [False, True])
@pytest.mark.parametrize("hw", ["1", "0"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_table_through_the_middle_step(bc, reference, dtype, hw, two_workgroups, monkeypatch):
    """the table's encode as segment 0 beside an all-zero segment (sum: the decode itself, re-encoded)
    and beside itself and a zero segment (mean of three: 2 d / 3, off every grid point)"""
    K = bc._native.K
    monkeypatch.setenv("BAGUA_MXFP8_HWCVT", hw)
    if two_workgroups:
        monkeypatch.setenv("BAGUA_TUNE_MX8_MIDDLE_BLOCKS", "2")
    x, _, _ = reference[dtype]
    cs = x.size
    one = R.compress(x, dtype, 1)
    zero = np.zeros_like(one)
    for segs, average, target in (([one, zero], 0, 1), ([one, zero, one], 1, 0)):
        p = len(segs)
        recv = np.concatenate(segs)
        S = recv.size
        want, _ = R.reduce_requantize(recv, p, cs, dtype, target, bool(average), out=np.full(S, FILL, np.uint8))
        rt = torch.from_numpy(recv).cuda()
        out = torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
        assert K.bagua_mxfp8_reduce_requantize(dtype, rt.data_ptr(), S, cs, p, None, average, out.data_ptr(), S, target,
                                               None) == OK
        same_bytes(u8(out), want, f"dtype={dtype} hw={hw} p={p} average={average} two_workgroups={two_workgroups}")


@pytest.mark.parametrize("hw", ["1", "0"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_scale_byte_times_every_element_byte(bc, dtype, hw, monkeypatch):
    K = bc._native.K
    monkeypatch.setenv("BAGUA_MXFP8_HWCVT", hw)
    nb = 256 * 8                      # eight blocks per scale byte hold the 256 element bytes
    cs = 32 * nb
    buf = np.zeros(R.compressed_bytes(cs, 1), np.uint8)
    buf[:nb] = np.repeat(np.arange(256, dtype=np.uint8), 8)
    sb = R.scale_bytes(cs)
    buf[sb:sb + 32 * nb] = np.tile(np.arange(256, dtype=np.uint8), 256)
    want = R.decompress(buf, 1, np.zeros(cs, R.STORAGE[dtype]), dtype)
    ct = torch.from_numpy(buf).cuda()
    out = torch.zeros(cs, dtype=TORCH[dtype], device="cuda")
    assert K.bagua_mxfp8_decompress(dtype, ct.data_ptr(), buf.size, cs, 1, out.data_ptr(), None) == OK
    same_bytes(host(out, dtype), want, f"dtype={dtype} hw={hw}")
    # and through the middle step's decode: one segment, sum -- the re-encode of every decodable value
    rt = torch.from_numpy(buf).cuda()
    o2 = torch.full((buf.size,), FILL, dtype=torch.uint8, device="cuda")
    assert K.bagua_mxfp8_reduce_requantize(dtype, rt.data_ptr(), buf.size, cs, 1, None, 0, o2.data_ptr(), buf.size, 0,
                                           None) == OK
    w2, _ = R.reduce_requantize(buf, 1, cs, dtype, 0, False, out=np.full(buf.size, FILL, np.uint8))
    same_bytes(u8(o2), w2, f"dtype={dtype} hw={hw}: middle step")
