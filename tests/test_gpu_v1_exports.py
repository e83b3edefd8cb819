"""The v1-style exports no other test calls (include/bagua_kernels.h, "v1-style extensions",
and array_min_max_size_f16_host): one parity call each on a small valid input, against the
oracle and against the v2 entry point they wrap -- a wrapper passing the wrong dtype code
or argument order does not survive it.  These functions exit() on error, so every argument
is valid."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_codec import BF16, F16, F32, STORAGE, TORCH, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401

pytestmark = pytest.mark.gpu

P, CS = 3, 1000 + 5
vp, sz, i32, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
COMPRESS = (None, [vp, i32, i32, i32, vp, sz, vp, sz, i32, vp])
DECOMPRESS = (None, [vp, sz, i32, i32, vp, vp])
REDUCE = (None, [vp, i32, i32, i32, vp])
SIGNATURES = {
    "compress_bf16_to_uint8_host": COMPRESS, "decompress_uint8_to_bf16_host": DECOMPRESS,
    "array_min_max_size_bf16_host": (sz, [vp, i32, vp, vp]), "array_min_max_size_f16_host": (sz, [vp, i32, vp, vp]),
    "reduce_mean_bf16_inplace_host": REDUCE, "reduce_sum_bf16_inplace_host": REDUCE,
    "add_inplace_bf16_host": (None, [vp, vp, i32, vp]), "addmul_inplace_bf16_host": (None, [vp, vp, i32, f32, vp]),
    "compress_f32_to_onebit_host": COMPRESS, "decompress_onebit_to_f32_host": DECOMPRESS,
    "compress_bf16_to_onebit_host": COMPRESS, "decompress_onebit_to_bf16_host": DECOMPRESS,
    "onebit_temp_size_host": (sz, [i32, i32]),
}


@pytest.fixture(scope="module")
def V(bc):
    lib = bc._native.kernels
    ns = type("V1", (), {})()
    for name, (res, args) in SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
        setattr(ns, name, f)
    return ns


def sample(dtype, seed, offset=0.1):
    from oracle import oracle_np as NP
    x = (np.random.default_rng(seed).standard_normal(P * CS) * 1e-2 + offset).astype(np.float32)
    return NP.from_f32(x, dtype)


def test_workspace_size_queries(bc, V):
    K = bc._native.K
    x = to_dev(sample(BF16, 1), BF16)
    want = K.array_min_max_size_f32_host(x.data_ptr(), P * CS, x.data_ptr(), None)
    assert want >= K.bagua_minmax_u8_workspace_bytes(CS, P) > 0
    assert V.array_min_max_size_bf16_host(x.data_ptr(), P * CS, x.data_ptr(), None) == want
    assert V.array_min_max_size_f16_host(x.data_ptr(), P * CS, x.data_ptr(), None) == want
    assert V.onebit_temp_size_host(CS, P) == K.bagua_onebit_workspace_bytes(CS, P) > 0


def test_bf16_minmax_compress_decompress(bc, oracle_c, V):
    K = bc._native.K
    x = sample(BF16, 2)
    xd = to_dev(x, BF16)
    S = K.bagua_minmax_u8_compressed_bytes(BF16, CS, P)
    tmp_bytes = V.array_min_max_size_bf16_host(xd.data_ptr(), P * CS, None, None)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
    want = oracle_c.compress_minmax_u8(x, BF16, P)
    for target in (-1, 1):
        out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
        V.compress_bf16_to_uint8_host(xd.data_ptr(), P * CS, CS, P, out.data_ptr(), S, tmp.data_ptr(), tmp_bytes,
                                      target, None)
        got = out.cpu().numpy()
        if target < 0:
            assert np.array_equal(got, want)
        else:
            co = S // P
            assert np.array_equal(got[co:2 * co], want[co:2 * co]) and np.all(np.delete(got, np.s_[co:2 * co]) == 0xA5)
    dec = torch.full((P * CS + 8,), 7.0, dtype=torch.bfloat16, device="cuda")
    comp_d = torch.from_numpy(want).cuda()
    V.decompress_uint8_to_bf16_host(comp_d.data_ptr(), S, CS, P, dec.data_ptr(), None)
    dw = oracle_c.decompress_minmax_u8(want, P, np.zeros(P * CS, np.uint16), BF16)
    got = to_host(dec, BF16)
    assert_float_bits_equal(got[:P * CS], dw, BF16, "v1 bf16 decode")
    assert np.all(got[P * CS:] == 0x40E0)


@pytest.mark.parametrize("average", [1, 0])
def test_bf16_reduce(bc, oracle_c, V, average):
    x = sample(BF16, 3 + average)
    for target in range(P):
        xd = to_dev(x, BF16)
        f = V.reduce_mean_bf16_inplace_host if average else V.reduce_sum_bf16_inplace_host
        f(xd.data_ptr(), CS, P, target, None)
        want = oracle_c.reduce_chunks(x.copy(), BF16, P, target, bool(average))
        assert_float_bits_equal(to_host(xd, BF16), want, BF16, f"v1 bf16 reduce average={average} target={target}")


def test_bf16_add_addmul(bc, oracle_c, V):
    x, y = sample(BF16, 5), sample(BF16, 6)
    xd, yd = to_dev(x, BF16), to_dev(y, BF16)
    factor = float(np.float32(-5.0 / 3.0))
    V.addmul_inplace_bf16_host(xd.data_ptr(), yd.data_ptr(), P * CS, factor, None)
    want = oracle_c.addmul_inplace(x.copy(), y, BF16, factor)
    assert_float_bits_equal(to_host(xd, BF16), want, BF16, "v1 bf16 addmul")
    V.add_inplace_bf16_host(xd.data_ptr(), yd.data_ptr(), P * CS, None)
    oracle_c.add_inplace(want, y, BF16)
    assert_float_bits_equal(to_host(xd, BF16), want, BF16, "v1 bf16 add")
    assert np.array_equal(to_host(yd, BF16), y)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_onebit_compress_decompress(bc, oracle_c, V, dtype):
    K = bc._native.K
    x = sample(dtype, 7 + dtype, offset=1e-3)  # both signs
    xd = to_dev(x, dtype)
    S = K.bagua_onebit_compressed_bytes(CS, P)
    tmp_bytes = V.onebit_temp_size_host(CS, P)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
    out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
    comp = V.compress_f32_to_onebit_host if dtype == F32 else V.compress_bf16_to_onebit_host
    comp(xd.data_ptr(), P * CS, CS, P, out.data_ptr(), S, tmp.data_ptr(), tmp_bytes, -1, None)
    want = oracle_c.compress_onebit(x, dtype, P)
    assert np.array_equal(out.cpu().numpy(), want)
    out2 = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")  # the v2 entry point's bytes
    assert K.bagua_onebit_compress(dtype, xd.data_ptr(), P * CS, CS, P, out2.data_ptr(), S, tmp.data_ptr(), tmp_bytes,
                                   -1, None) == 0
    assert torch.equal(out, out2)
    dec = torch.full((P * CS + 8,), 7.0, dtype=TORCH[dtype], device="cuda")
    decomp = V.decompress_onebit_to_f32_host if dtype == F32 else V.decompress_onebit_to_bf16_host
    decomp(out.data_ptr(), S, CS, P, dec.data_ptr(), None)
    dw = oracle_c.decompress_onebit(want, P, np.zeros(P * CS, STORAGE[dtype]), dtype)
    got = to_host(dec, dtype)
    assert_float_bits_equal(got[:P * CS], dw, dtype, "v1 1-bit decode")
    assert np.all(got[P * CS:].view(STORAGE[dtype]) == (7.0 if dtype == F32 else 0x40E0))
