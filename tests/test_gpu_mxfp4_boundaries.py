"""GPU tests of the MXFP4 kernels (csrc/kernels/mxfp4.hip) at the decision boundaries of the
format: the boundary table of tests/mxfp4_boundary_cases.py (every scale byte a finite T can
produce, every tie of the E2M1 grid and the T values one ulp beside it, the edge of the scale
rule, a planted amax at every position of a block) through the encode, the decode, the
error-feedback encode and the middle step; every scale byte decoded; and the built variants
that no bucket of test size selects on its own: the arithmetic in place of gfx950's FP4
conversions (BAGUA_MXFP4_HWCVT=0), the non-temporal decode stores and the non-temporal
residual accesses.  Segments are compared byte for byte, decoded tensors and residuals bit
for bit, with tests/mxfp4_reference.py and tests/mxfp4_ef_reference.py.

The knobs are read from the environment on every call, so they are set with monkeypatch as
the grid knobs are."""
import functools

import numpy as np
import pytest
import torch

import mxfp4_boundary_cases as B
import mxfp4_ef_reference as REF
import mxfp4_reference as R
from oracle import oracle_np as NP
from test_gpu_codec import assert_float_bits_equal
from test_gpu_multirank import host
from test_gpu_mxfp4 import GRID_KNOBS, OK, TORCH, dev_at, grads, same_bytes, u8
from test_gpu_mxfp4_ef import codec_steps, f32_host

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(autouse=True)
def default_variants(monkeypatch):
    """every test starts from the shipped choice of variants"""
    for k in ("BAGUA_MXFP4_HWCVT", "BAGUA_MX_DECODE_NT", "BAGUA_MX_EF_RESIDUAL_NT") + GRID_KNOBS:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------ references, computed once ----
@functools.lru_cache(maxsize=None)
def table_reference(dtype, p):
    """(compressed buffer, decoded tensor) of the table cut into p chunks"""
    x = B.table(dtype).x
    comp = R.compress(x, dtype, p)
    dec = R.decompress(comp, p, np.zeros_like(x), dtype)
    comp.setflags(write=False)
    dec.setflags(write=False)
    return comp, dec


@functools.lru_cache(maxsize=None)
def table_ef_reference(dtype, p, steps=2):
    """[(compressed buffer, residual)] of `steps` steps with the table as the gradient, state zero before"""
    x = B.table(dtype).x
    st = REF.WorkerState(x.size)
    out = []
    for _ in range(steps):
        buf = REF.compress_ef(x, dtype, p, st)
        out.append((buf, st.residual.copy()))
    return out


@functools.lru_cache(maxsize=None)
def middle_reference(kind, dtype, target):
    """(Middle, buffer with the target's segment, reduced tensor, [(segment, residual)] of two EF steps)"""
    m = {"exact": B.middle_exact, "neighbours": lambda d: B.middle_neighbours(),
         "table": table_as_received}[kind](dtype)
    S = m.recv.size
    buf, t = R.reduce_requantize(m.recv, m.p, m.cs, dtype, target, False, out=np.full(S, 0xCD, np.uint8))
    res = np.zeros(m.cs, np.float32)
    ef = []
    for _ in range(2):
        seg = REF.middle_ef(NP, m.recv, m.p, m.cs, dtype, target, False, res)
        ef.append((seg, res.copy()))
    return m, buf, t, ef


def table_as_received(dtype):
    """the table's own segment as the single received one: the middle step decodes every scale byte and
    encodes, a whole block in one lane, grid values at every scale byte"""
    t = B.table(dtype)
    return B.Middle(dtype, 1, t.x.size, table_reference(dtype, 1)[0], None, None, t.byte, None, None)


def set_grid(monkeypatch, n_chunks):
    for k in GRID_KNOBS:
        monkeypatch.setenv(k, str(2 * n_chunks))  # the cap is shared by the chunks: two workgroups each


def table_roundtrip(bc, dtype, p, offset, what):
    """the table through compress + decompress_from; returns the compressed bytes"""
    x = B.table(dtype).x
    want, dec = table_reference(dtype, p)
    xt = dev_at(x, dtype, offset)
    assert (xt.data_ptr() % 16 != 0) == bool(offset)
    comp = bc.BaguaTensorPy(xt, "x").compress("MXFP4", p, -1)
    got = comp.to_numpy_u8()
    same_bytes(got, want, f"{what}: compressed")
    out = dev_at(np.zeros_like(x), dtype, offset)
    out.fill_(7.0)
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP4", p, comp)
    same_bytes(host(out, dtype), dec, f"{what}: decoded")
    return got


# ------------------------------------- 1. encode and decode at the boundaries ----
@pytest.mark.parametrize("two_workgroups", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_table_encode_decode(bc, dtype, n_chunks, offset, two_workgroups, monkeypatch):
    """16-byte aligned (vector loads) and one element into the allocation (guarded loads); the default
    grid and two workgroups per chunk (one chunk: the table reaches the second grid-stride iteration)"""
    if two_workgroups:
        set_grid(monkeypatch, n_chunks)
    table_roundtrip(bc, dtype, n_chunks, offset, f"table p={n_chunks} offset={offset} two_workgroups={two_workgroups}")


# ------------------------------------------ 2. EF encode at the boundaries ----
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_table_error_feedback_encode(bc, dtype, n_chunks, offset):
    x = B.table(dtype).x
    state = bc.MXFP4ErrorFeedbackState(x.size, n_chunks, 0)
    xt = dev_at(x, dtype, offset)
    t = bc.BaguaTensorPy(xt, "g")
    for step, (want, res) in enumerate(table_ef_reference(dtype, n_chunks)):
        got = t.compress_with_error_feedback(n_chunks, state).to_numpy_u8()
        same_bytes(got, want, f"step {step}: payload")
        if step == 0:  # zero state, no -0 in the table: the plain codec's bytes
            same_bytes(got, table_reference(dtype, n_chunks)[0], "step 0 against the plain codec")
        same_bytes(f32_host(state.worker_residual), res, f"step {step}: residual")
    same_bytes(host(xt, dtype), x, "the gradient is read only")
    assert res.any()


# ------------------------------------------ 3. middle step at the boundaries ----
def run_middle(bc, kind, dtype, what):
    """bagua_mxfp4_reduce_requantize (stored and not stored) and two steps of _ef, sum mode"""
    K = bc._native.K
    target = 0
    m, want_buf, want_t, want_ef = middle_reference(kind, dtype, target)
    p, cs, S = m.p, m.cs, m.recv.size
    seg = R.segment_bytes(cs)
    rt = torch.from_numpy(m.recv.copy()).cuda()
    for store in (False, True):
        out = torch.full((S,), 0xCD, dtype=torch.uint8, device="cuda")
        tensor = torch.full((p * cs,), 5.0, dtype=TORCH[dtype], device="cuda")
        rc = K.bagua_mxfp4_reduce_requantize(dtype, rt.data_ptr(), S, cs, p, tensor.data_ptr() if store else None, 0,
                                             out.data_ptr(), S, target, None)
        assert rc == OK, what
        same_bytes(u8(out), want_buf, f"{what} store={store}")
        got_t = host(tensor, dtype)
        if store:
            assert_float_bits_equal(got_t[:cs], want_t[:cs], dtype, what)
        else:
            assert (NP.to_f32(got_t, dtype) == 5.0).all(), f"{what}: the tensor must not be written"
    res = torch.zeros(cs, dtype=torch.float32, device="cuda")
    for step, (want_seg, want_res) in enumerate(want_ef):
        out = torch.full((S,), 0xCD, dtype=torch.uint8, device="cuda")
        assert K.bagua_mxfp4_reduce_requantize_ef(dtype, rt.data_ptr(), S, cs, p, 0, out.data_ptr(), S, target,
                                                  res.data_ptr(), None) == OK, what
        got = u8(out)
        same_bytes(got[:seg], want_seg, f"{what}: EF step {step}")
        assert (got[seg:] == 0xCD).all()
        same_bytes(f32_host(res), want_res, f"{what}: EF step {step} residual")
        if step == 0:
            same_bytes(want_seg, want_buf[:seg], "zero state: the plain middle step's bytes")
    return want_buf[:seg]


@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step_exact_boundaries(bc, dtype):
    """p = 2, sum mode: two received segments whose decoded values sum exactly to each boundary under
    a pin of 3 + 3 = 6, at a dozen output scale bytes from the lowest to the highest reachable
    (mxfp4_boundary_cases.MIDDLE_EXACT_BYTES)"""
    run_middle(bc, "exact", dtype, "exact boundaries")


def test_middle_step_one_ulp_neighbours(bc):
    """p = 3, f32, sum mode: a third segment far below supplies the single ulp.  Output scale bytes
    below 26 are left out: the smallest boundary's f32 ulp is 2^(e - 26), and no scale byte below 0
    exists to hold it (mxfp4_boundary_cases.MIDDLE_NEIGHBOUR_BYTES)"""
    run_middle(bc, "neighbours", F32, "one-ulp neighbours")


@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step_of_the_table(bc, dtype):
    """p = 1: the table's own segment decoded and encoded again, a whole block in one lane, at every
    scale byte"""
    run_middle(bc, "table", dtype, "table as the received segment")


# ----------------------------------------------- 4. every scale byte decoded ----
def all_scale_bytes():
    """bytes 0 to 255 twice, every nibble value in both nibble positions (and mixed), a ragged last block"""
    nb = 512
    cs = 32 * nb - 5  # the last block decodes 27 elements
    sb = R.scale_bytes(cs)
    buf = np.zeros(R.compressed_bytes(cs, 1), np.uint8)
    buf[:nb] = np.arange(nb) % 256
    pay = np.empty((nb, 16), np.uint8)
    pay[:256] = np.arange(16, dtype=np.uint8) * 0x11          # the same nibble in both positions
    k = np.arange(16, dtype=np.uint8)
    pay[256:] = (k << 4) | (15 - k)                            # every value high beside another one low
    buf[sb:sb + 16 * nb] = pay.ravel()
    return buf, cs


@pytest.mark.parametrize("nt", [None, "1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_of_every_scale_byte(bc, dtype, nt, monkeypatch):
    """the default store policy and the non-temporal stores (BAGUA_MX_DECODE_NT=1); for f16 this holds the
    bytes around 100 to 104, where a decoded half step is a tie of f16's denormal grid"""
    if nt is not None:
        monkeypatch.setenv("BAGUA_MX_DECODE_NT", nt)
    buf, cs = all_scale_bytes()
    comp = bc.BaguaTensorPy(torch.from_numpy(buf).cuda(), "every scale byte")
    out = torch.zeros(cs, dtype=TORCH[dtype], device="cuda")
    bc.BaguaTensorPy(out, "out").decompress_from("MXFP4", 1, comp)
    want = R.decompress(buf, 1, np.zeros(cs, R.STORAGE[dtype]), dtype)
    same_bytes(host(out, dtype), want, "decode")
    if dtype == F16:  # the ties are there (element 2k holds code k): 0.5 and 1.5 steps of 2^-24 give 0 and 2^-23
        w = NP.to_f32(want, dtype)[:32 * 256].reshape(256, 32)
        assert w[103, 2] == 0 and w[103, 6] == 2.0 ** -23 and w[102, 4] == 0 and w[102, 10] == 2.0 ** -23


# ---------------------------------- 5. the arithmetic builds of the plain kernels ----
CUT_SIZES = [1, 31, 33, 2049, 8193, 16385]


def plain_cases(bc, dtype):
    """name -> bytes: the table's encode (one and three chunks, each decoded), the cut-down size list
    and the middle step, each checked against the reference on the way"""
    out = {}
    for p in (1, 3):
        out[f"table p={p}"] = table_roundtrip(bc, dtype, p, 0, f"table p={p}")
    rng = np.random.default_rng(500 + dtype)
    for cs in CUT_SIZES:
        for p in (1, 2):
            x = grads(rng, p * cs, dtype)
            comp = bc.BaguaTensorPy(dev_at(x, dtype), "x").compress("MXFP4", p, -1)
            want = R.compress(x, dtype, p)
            same_bytes(comp.to_numpy_u8(), want, f"cs={cs} p={p}: compressed")
            t = torch.zeros(p * cs, dtype=TORCH[dtype], device="cuda")
            bc.BaguaTensorPy(t, "out").decompress_from("MXFP4", p, comp)
            same_bytes(host(t, dtype), R.decompress(want, p, np.zeros_like(x), dtype), f"cs={cs} p={p}: decoded")
            out[f"cs={cs} p={p}"] = comp.to_numpy_u8()
    out["middle exact"] = run_middle(bc, "exact", dtype, "exact boundaries")
    out["middle table"] = run_middle(bc, "table", dtype, "table as the received segment")
    if dtype == F32:
        out["middle neighbours"] = run_middle(bc, "neighbours", dtype, "one-ulp neighbours")
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_arithmetic_builds_of_the_plain_kernels(bc, dtype, monkeypatch):
    """BAGUA_MXFP4_HWCVT=0: mxfp4_encode_kernel, mxfp4_decode_kernel and mxfp4_reduce_encode_kernel
    built on the arithmetic of mxfp4_common.hpp give the reference's bytes and the hardware path's"""
    hw = plain_cases(bc, dtype)
    monkeypatch.setenv("BAGUA_MXFP4_HWCVT", "0")
    sw = plain_cases(bc, dtype)
    assert sorted(hw) == sorted(sw)
    for k in hw:
        same_bytes(sw[k], hw[k], f"{k}: arithmetic against hardware conversions")


@pytest.mark.parametrize("dtype", DTYPES)
def test_arithmetic_builds_two_workgroups_and_guarded_loads(bc, dtype, monkeypatch):
    monkeypatch.setenv("BAGUA_MXFP4_HWCVT", "0")
    table_roundtrip(bc, dtype, 3, 1, "table p=3 offset=1")
    set_grid(monkeypatch, 1)
    table_roundtrip(bc, dtype, 1, 0, "table p=1 two workgroups")
    monkeypatch.setenv("BAGUA_MX_DECODE_NT", "1")
    table_roundtrip(bc, dtype, 1, 0, "table p=1 two workgroups, non-temporal decode")


# ------------------------------------------------- 6. non-temporal residual ----
@pytest.mark.parametrize("nt", ["1", "0"])
@pytest.mark.parametrize("n_chunks,cs", [(3, 4100), (8, 20000)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_error_feedback_residual_policy_forced(bc, dtype, n_chunks, cs, nt, monkeypatch):
    """BAGUA_MX_EF_RESIDUAL_NT=1 launches the NT = true build of mxfp4_encode_ef_kernel, which a bucket
    takes on its own only past 256 MiB; =0 the other one"""
    monkeypatch.setenv("BAGUA_MX_EF_RESIDUAL_NT", nt)
    codec_steps(bc, dtype, n_chunks, cs, steps=3)
