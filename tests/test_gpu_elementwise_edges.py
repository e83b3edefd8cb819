"""elementwise.hip at the v2 C ABI (bagua_{add,addmul,substract,average,divide}_inplace) for
f32, f16 and bf16 on the launch shapes and values the small tests never reach: the scalar
kernel with only x, only y or both one element off 16 B, more vectors (and more scalar
elements) than the 2048-workgroup grid cap, NaN, +-inf, inf - inf, +-0, denormals, overflow, and
factors / divisors that round (or overflow) when stored in T.

Reference: add and addmul are the C oracle's (orc_add_inplace / orc_addmul_inplace),
cross-checked against the numpy oracle at the small sizes; substract, average and divide
restate elementwise.hip's stated numerics in numpy -- one f32 operation then RNE to T, the
16-bit average rounds the sum to T first, factor and divisor are rounded to T for 16-bit types,
and the f16 divide is the correctly rounded quotient (f32 division of two f16 values, then
RNE to f16: 24 >= 2 * 11 + 2 bits).  Floats are compared bit for bit, NaN as NaN-ness; the
elements in front of and behind x keep their fill and y is never written."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_np as NP
from test_gpu_codec import BF16, F16, F32, STORAGE, TORCH, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
IDS = ["f32", "f16", "bf16"]
NAMES = dict(zip(DTYPES, IDS))
VEC_N = {F32: 4, F16: 8, BF16: 8}
INVALID_ARG, UNSUPPORTED = 1, 4
OPS = ["add", "addmul", "substract", "average", "divide"]
FACTORS = [0.0, -5.0 / 3.0, 1.0 / 3.0, 1e-8, 65520.0, float("inf"), float("nan")]
DIVISORS = [3.7, -0.0, 0.0, float("inf"), 1e-8]
T_MAX = {F32: float(np.finfo(np.float32).max), F16: 65504.0, BF16: float(NP.INIT_MAX[BF16])}
DENORMAL = {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}  # the smallest of T
HALF_ULP_OF_MAX = {F32: 2.0 ** 103, F16: 16.0, BF16: 2.0 ** 119}


def sizes(dtype):
    n = VEC_N[dtype]
    return [1, 7, n, n + 1, 256 * n + 3]


def past_cap(dtype):
    """more vectors than 2048 workgroups x 256 lanes (a second trip), then a scalar tail"""
    n = VEC_N[dtype]
    return 2048 * 256 * n + 256 * n + 3


def special_pairs(dtype):
    inf, nan, big, den = np.inf, np.nan, T_MAX[dtype], DENORMAL[dtype]
    pairs = [(nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf), (inf, -inf), (inf, inf), (-inf, -inf),
             (0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (den, den), (den, -den), (-den, 0.0), (3 * den, -den),
             (big, big), (-big, -big), (big, -big), (big, 1.0), (1.0, den), (-0.0, den),
             # max + half an ulp: the tie rounds to inf in T while the f32 sum is still finite (for
             # 16-bit T), so an average that skips the rounding of the sum gives max / 2 instead
             (big, HALF_ULP_OF_MAX[dtype]), (-big, -HALF_ULP_OF_MAX[dtype])]
    if dtype == F32:
        pairs += [(1e-40, 1e-40), (1e-40, -3e-40), (1.0, 1e-40)]
    return np.array(pairs, np.float32)


def operands(dtype, n, seed):
    """random values; the specials at the front (the vector body) and at the very end (the
    scalar tail), rotated by the seed so the short sizes see different ones"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    y = (rng.standard_normal(n) * 3).astype(np.float32)
    sp = np.roll(special_pairs(dtype), seed, axis=0)
    m = min(n, len(sp))
    x[:m], y[:m] = sp[:m, 0], sp[:m, 1]
    if n > 2 * len(sp):
        x[n - len(sp):], y[n - len(sp):] = sp[:, 0], sp[:, 1]
    return NP.from_f32(x, dtype), NP.from_f32(y, dtype)


def rounded(v, dtype):
    """v as stored in T, back in f32"""
    return NP.to_f32(NP.from_f32(np.asarray(v, np.float32), dtype), dtype).astype(np.float32)


def expected(op, oracle_c, x, y, dtype, f, cross_check):
    with np.errstate(all="ignore"):
        if op == "add":
            want = oracle_c.add_inplace(x.copy(), y, dtype)
            if cross_check:
                assert_float_bits_equal(NP.add_inplace(x.copy(), y, dtype), want, dtype, "the oracles differ on add")
            return want
        if op == "addmul":
            want = oracle_c.addmul_inplace(x.copy(), y, dtype, f)
            if cross_check:
                assert_float_bits_equal(NP.addmul_inplace(x.copy(), y, dtype, f), want, dtype,
                                        f"the oracles differ on addmul factor={f}")
            return want
        xf, yf = NP.to_f32(x, dtype).astype(np.float32), NP.to_f32(y, dtype).astype(np.float32)
        if op == "substract":
            r = xf - yf
        elif op == "average":
            r = ((xf + yf) if dtype == F32 else rounded(xf + yf, dtype)) / np.float32(2)
        else:
            d = np.float32(f) if dtype == F32 else rounded(np.array([f], np.float32), dtype)[0]
            r = xf / d
        return NP.from_f32(r.astype(np.float32), dtype)


def call(K, op, dtype, xp, yp, n, f):
    if op == "addmul":
        return K.bagua_addmul_inplace(dtype, xp, yp, n, f, None)
    if op == "divide":
        return K.bagua_divide_inplace(dtype, xp, f, n, None)
    return getattr(K, f"bagua_{op}_inplace")(dtype, xp, yp, n, None)


def seven_bits(dtype):
    return NP.from_f32(np.array([7.0], np.float32), dtype).view(np.uint16 if dtype != F32 else np.uint32)[0]


def run_case(K, oracle_c, op, dtype, n, ox, oy, f, seed, cross_check):
    x, y = operands(dtype, n, seed)
    want = expected(op, oracle_c, x, y, dtype, f, cross_check)
    pad = 16
    xb = torch.full((ox + n + pad,), 7.0, dtype=TORCH[dtype], device="cuda")
    xb[ox:ox + n] = to_dev(x, dtype)
    yd = to_dev(y, dtype, oy)
    xd = xb[ox:ox + n]
    es = NP.esize(dtype)
    assert xd.data_ptr() % 16 == (ox * es) % 16 and yd.data_ptr() % 16 == (oy * es) % 16
    what = f"{op} {NAMES[dtype]} n={n} x+{ox} y+{oy} f={f}"
    assert call(K, op, dtype, xd.data_ptr(), yd.data_ptr(), n, f) == 0, what
    got = to_host(xb, dtype)
    assert_float_bits_equal(got[ox:ox + n], want, dtype, what)
    bits = np.uint32 if dtype == F32 else np.uint16
    assert np.all(got[:ox].view(bits) == seven_bits(dtype)) and np.all(got[ox + n:].view(bits) == seven_bits(dtype)), \
        f"{what}: written outside x"
    assert np.array_equal(to_host(yd, dtype).view(bits), y.view(bits)), f"{what}: y changed"


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_small_sizes_alignments_and_specials(bc, oracle_c, dtype, op):
    """1, 7, one vector, one vector + 1, 256 vectors + 3 elements; x and y aligned or one
    element off in every combination (any misalignment selects the scalar kernel); every factor
    and divisor."""
    K = bc._native.K
    params = FACTORS if op == "addmul" else DIVISORS if op == "divide" else [0.0]
    for n in sizes(dtype):
        for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            for i, f in enumerate(params):
                run_case(K, oracle_c, op, dtype, n, ox, oy, f, seed=n + 3 * ox + 5 * oy + i, cross_check=True)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_past_the_grid_cap(bc, oracle_c, dtype, op):
    """2048 * 256 vectors + 256 vectors + 3 elements: the lanes of the vector kernel take a second
    trip and a scalar tail follows; misaligned, the scalar kernel strides several times."""
    K = bc._native.K
    n = past_cap(dtype)
    params = [-5.0 / 3.0, 65520.0] if op == "addmul" else [3.7] if op == "divide" else [0.0]
    for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        if op == "divide" and oy:
            continue  # no y
        for f in params:
            run_case(K, oracle_c, op, dtype, n, ox, oy, f, seed=ox + 2 * oy, cross_check=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_and_invalid_calls(bc, dtype):
    K = bc._native.K
    x = torch.full((64,), 7.0, dtype=TORCH[dtype], device="cuda")
    y = torch.full((64,), 3.0, dtype=TORCH[dtype], device="cuda")
    for op in OPS:
        assert call(K, op, dtype, x.data_ptr(), y.data_ptr(), 0, 2.0) == 0, op              # n = 0: nothing to do
        assert call(K, op, dtype, x.data_ptr(), y.data_ptr(), -1, 2.0) == INVALID_ARG, op
        assert call(K, op, dtype, None, y.data_ptr(), 8, 2.0) == INVALID_ARG, op
        if op != "divide":
            assert call(K, op, dtype, x.data_ptr(), None, 8, 2.0) == INVALID_ARG, op
        assert call(K, op, 3, x.data_ptr(), y.data_ptr(), 8, 2.0) == UNSUPPORTED, op        # u8
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((y == 3.0).all())


@pytest.mark.parametrize("nranks", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 2048 * 256 + 77])
def test_async_model_average_edges(bc, n, nranks):
    """async_model_average_host: tensor[i] += reduced[i] / nranks - copy[i] past its grid cap and
    at one element, with specials in each operand; N = 0 writes nothing."""
    K = bc._native.K
    rng = np.random.default_rng(n + nranks)
    t, r, c = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1e-40, 3.4e38, -3.4e38], np.float32)
    if n > 64:
        m = len(sp)
        t[0:m] = sp
        r[m:2 * m] = sp
        c[2 * m:3 * m] = sp
        t[n - m:], r[n - m:], c[n - m:] = sp, np.roll(sp, 1), np.roll(sp, 2)  # inf - inf, 0 - 0, overflow
    else:
        t[0], r[0], c[0] = -0.0, 0.0, 0.0
    td = torch.full((n + 16,), 7.0, dtype=torch.float32, device="cuda")
    td[:n] = torch.from_numpy(t).cuda()
    rd, cd = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
    K.async_model_average_host(td.data_ptr(), rd.data_ptr(), cd.data_ptr(), 0.0, 0, None)  # N = 0
    assert np.array_equal(td[:n].cpu().numpy().view(np.uint32), t.view(np.uint32)), "N = 0 wrote"
    K.async_model_average_host(td.data_ptr(), rd.data_ptr(), cd.data_ptr(), float(nranks), n, None)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = (t + ((r / np.float32(nranks)) - c)).astype(np.float32)
    assert_float_bits_equal(td[:n].cpu().numpy(), want, F32, f"n={n} nranks={nranks}")
    assert bool((td[n:] == 7.0).all()), "written past the tensor"
    assert np.array_equal(rd.cpu().numpy().view(np.uint32), r.view(np.uint32))
    assert np.array_equal(cd.cpu().numpy().view(np.uint32), c.view(np.uint32))
