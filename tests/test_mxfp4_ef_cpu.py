"""CPU tests of the MXFP4 codec's error feedback (MXFP4.md, "Error feedback"): the kernels'
block arithmetic compiled for the host against the reference composition
(tests/mxfp4_ef_reference.py), the rule's properties on that reference, and the new C-ABI
surface.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mxfp4_ef_reference as REF
import mxfp4_reference as R
import onebit_ef_reference as OB
from oracle import oracle_np as NP
from test_abi import LIB, built, declared, exported  # noqa: F401  (built: fixture)
from test_mxfp4_cpu import hostile_blocks, random_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]

KERNEL_SYMBOLS = ["bagua_mxfp4_ef_state_bytes", "bagua_mxfp4_compress_ef", "bagua_mxfp4_reduce_requantize_ef"]
CORE_SYMBOLS = ["bagua_centralized_mxfp4_error_feedback", "bagua_tensor_compress_mxfp4_error_feedback"]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mxfp4_ef") / "mxfp4_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp4_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host(exe, x32, e32, dtype):
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    raw = np.concatenate([x32, e32], axis=1).astype(np.float32).tobytes()
    out = subprocess.run([exe, "ef", maxf, str(dtype)], input=raw, capture_output=True, check=True).stdout
    rec = np.frombuffer(out, np.uint8).reshape(-1, 17 + 128)
    return rec[:, 0], rec[:, 1:17], np.ascontiguousarray(rec[:, 17:]).view(np.float32).reshape(-1, 32)


def ef_inputs(dtype):
    """(x, e) blocks: random blocks under residuals of every relative size, the hostile blocks of
    the plain codec's test with zero and with non-zero residuals, ties reached only through the
    residual, signed zeros, a NaN in x and one in e, and |x + e| just past the largest finite T"""
    rng = np.random.default_rng(77 + dtype)
    x = random_blocks(dtype, 4000, 41 + dtype)
    amax = np.abs(np.where(np.isfinite(x), x, 0)).max(axis=1, keepdims=True)
    e = rng.standard_normal(x.shape) * amax * 10.0 ** rng.uniform(-4, 0, (x.shape[0], 1))
    e[::7] = 0.0
    h = hostile_blocks(dtype)
    hz = np.zeros(h.shape)
    hm = np.abs(np.where(np.isfinite(h), h, 0)).max(axis=1, keepdims=True)
    he = rng.standard_normal(h.shape) * hm * 0.25
    # ties of the grid reached through the residual: x = 6, 1, 1, ... and e = tie - x under e = 0
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    tx = np.zeros((1, 32))
    tx[0, 0] = 6.0
    tx[0, 1:8] = 1.0
    tx[0, 8:15] = -1.0
    te = np.zeros((1, 32))
    te[0, 1:8] = ties - 1.0
    te[0, 8:15] = -(ties - 1.0)
    mx = R.MAX_FINITE[dtype]
    sx = np.zeros((5, 32))
    se = np.zeros((5, 32))
    sx[0, :] = -0.0                                  # -0 + (+0) = +0
    sx[1, :16], se[1, :16] = -0.0, -0.0              # -0 + -0 = -0
    sx[1, 16:], se[1, 16:] = 1.0, -1.0               # x + e = +0
    sx[2, 0], se[2, 0], sx[2, 1:] = mx, mx * 2.0 ** -6, 1.0           # past M: clamped
    sx[2, 1], se[2, 1] = -mx, -mx * 2.0 ** -6
    sx[3, 3], sx[3, 4:] = np.nan, 2.0                # NaN in x
    se[3, :] = 0.5
    sx[4, :], se[4, 9], se[4, 10] = 3.0, np.nan, 0.25   # NaN in e
    ix = np.array([[np.inf, -np.inf] + [1.0] * 30, [mx, -mx] + [1.0] * 30])
    ie = np.array([[0.0] * 32, [np.inf, -np.inf] + [0.125] * 30])    # inf in x, inf in e
    xs = np.concatenate([x, h, h, tx, sx, ix])
    es = np.concatenate([e, hz, he, te, se, ie])
    with np.errstate(over="ignore", invalid="ignore"):
        x32 = NP.to_f32(NP.from_f32(xs.astype(np.float32).ravel(), dtype), dtype).astype(np.float32).reshape(xs.shape)
        e32 = es.astype(np.float32)
    return x32, e32


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_matches_the_reference(host_check, dtype):
    x32, e32 = ef_inputs(dtype)
    scale, payload, new = REF.ef_blocks(x32, e32, dtype)
    g_scale, g_payload, g_new = run_host(host_check, x32, e32, dtype)
    assert np.array_equal(g_scale, scale)
    assert np.array_equal(g_payload, payload)
    bad = np.nonzero((u32(g_new) != u32(new)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], g_new[bad[:1]], new[bad[:1]])
    assert (scale == 0xFF).sum() >= 3 and (scale == 0).sum() >= 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_state_reproduces_the_plain_codec(dtype):
    n_chunks, cs = 3, 1025
    rng = np.random.default_rng(3 + dtype)
    x = NP.from_f32((rng.standard_normal(n_chunks * cs) * 1e-3).astype(np.float32), dtype)
    f = NP.to_f32(x, dtype)
    assert not (np.signbit(f) & (f == 0)).any()
    st = REF.WorkerState(x.size)
    assert np.array_equal(REF.compress_ef(x, dtype, n_chunks, st), R.compress(x, dtype, n_chunks))
    assert st.residual.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_bound(dtype):
    """where the scale byte is above 0 and amax is below M / 2: |e'| <= 2^(byte - 127), step after step"""
    x = random_blocks(dtype, 3000, 91 + dtype).astype(np.float32)
    x = x[np.isfinite(x).all(axis=1)]
    e = np.zeros_like(x)
    m = R.MAX_FINITE[dtype]
    checked = 0
    for step in range(4):
        with np.errstate(over="ignore"):
            v = np.clip(x + e, -m, m)
        scale, _, e = REF.ef_blocks(x, e, dtype)
        ok = (scale > 0) & (np.abs(v).max(axis=1) < m / 2)
        checked += int(ok.sum())
        bound = np.ldexp(1.0, scale.astype(np.int64) - 127)[:, None]
        assert (np.abs(e.astype(np.float64))[ok] <= bound[ok]).all(), step
    assert checked > 4000


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_block_resets_its_residuals_only(dtype):
    n = 5 * 32
    rng = np.random.default_rng(13)
    x = NP.from_f32(rng.standard_normal(n).astype(np.float32), dtype)
    st = REF.WorkerState(n)
    REF.compress_ef(x, dtype, 1, st)
    before = st.residual.copy()
    assert before[64:96].any()
    x2 = NP.to_f32(x, dtype).copy()
    x2[70] = np.nan
    clean = REF.WorkerState(n)
    clean.residual[...] = before
    REF.compress_ef(x, dtype, 1, clean)
    buf = REF.compress_ef(NP.from_f32(x2, dtype), dtype, 1, st)
    assert buf[2] == 0xFF and (buf[:5] != 0xFF).sum() == 4
    assert not u32(st.residual[64:96]).any()
    keep = np.r_[0:64, 96:n]
    assert np.array_equal(u32(st.residual[keep]), u32(clean.residual[keep]))
    # the next step is clean: the block encodes as under zero state
    buf3 = REF.compress_ef(x, dtype, 1, st)
    plain = R.compress(x, dtype, 1)
    sb = R.scale_bytes(n)
    assert buf3[2] == plain[2] and np.array_equal(buf3[sb + 32:sb + 48], plain[sb + 32:sb + 48])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,cs", [(2, 4096), (4, 4096), (8, 2048)])
def test_time_averaged_error_against_the_plain_op(dtype, p, cs):
    """constant gradients: the time-averaged result's mean absolute error against the true mean,
    relative to the plain op's, is below 0.2 after 8 steps and below 0.06 after 32"""
    xs = OB.appendix_inputs(p, cs, dtype)
    true = np.mean([NP.to_f32(x, dtype).astype(np.float64) for x in xs], axis=0)
    plain = NP.to_f32(R.centralized(xs, dtype, True)[0], dtype).astype(np.float64)
    err_plain = np.mean(np.abs(plain - true))
    states = [REF.OpState(p * cs, p) for _ in range(p)]
    acc = np.zeros(p * cs, np.float64)
    gmax = max(np.abs(NP.to_f32(x, dtype)).max() for x in xs)
    ratios = {}
    for step in range(1, 33):
        outs, _ = REF.centralized_step(NP, xs, dtype, states)
        acc += NP.to_f32(outs[0], dtype).astype(np.float64)
        if step in (8, 32):
            ratios[step] = np.mean(np.abs(acc / step - true)) / err_plain
    rmax = max(max(np.abs(s.worker).max(), np.abs(s.server).max()) for s in states)
    print(f"p={p} cs={cs} dt={dtype}: plain {err_plain / np.mean(np.abs(true)):.3f} of mean|true|, ratio after 8 "
          f"{ratios[8]:.3f}, after 32 {ratios[32]:.3f}, largest residual {rmax / gmax:.3f} of the largest gradient")
    assert ratios[8] < 0.2
    assert ratios[32] < 0.06


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_backends_agree(oracle_c, dtype):
    p, cs = 4, 1025
    rng = np.random.default_rng(5)
    sa = [REF.OpState(p * cs, p) for _ in range(p)]
    sb = [REF.OpState(p * cs, p) for _ in range(p)]
    for step in range(3):
        xs = [NP.from_f32((rng.standard_normal(p * cs) * 1e-3 + 0.0005 * r).astype(np.float32), dtype)
              for r in range(p)]
        oa, pa = REF.centralized_step(oracle_c, xs, dtype, sa)
        ob, pb = REF.centralized_step(NP, xs, dtype, sb)
        for r in range(p):
            assert np.array_equal(pa[r], pb[r]), (step, r)
            assert np.array_equal(oa[r].view(np.uint8), ob[r].view(np.uint8)), (step, r)
            assert np.array_equal(u32(sa[r].worker), u32(sb[r].worker)) and np.array_equal(u32(sa[r].server),
                                                                                           u32(sb[r].server))
        if step == 0:  # zero state: the plain op
            want = R.centralized(xs, dtype, True)
            assert all(np.array_equal(oa[r].view(np.uint8), want[r].view(np.uint8)) for r in range(p))


# ---- the C-ABI surface ---------------------------------------------------------------------
def test_new_symbols_declared_and_exported(built):
    k_decl, c_decl = declared("bagua_kernels.h"), declared("bagua_core.h")
    k_exp = exported(os.path.join(LIB, "libbagua_kernels.so"))
    c_exp = exported(os.path.join(LIB, "libbagua_core.so"))
    assert not [n for n in KERNEL_SYMBOLS if n not in k_decl or n not in k_exp]
    assert not [n for n in CORE_SYMBOLS if n not in c_decl or n not in c_exp]
    from bagua_core import _native as N
    assert set(KERNEL_SYMBOLS) <= set(N.KERNEL_SIGNATURES) and set(CORE_SYMBOLS) <= set(N.CORE_SIGNATURES)
    assert N.BUCKET_OP_CENTRALIZED_MXFP4_ERROR_FEEDBACK == 6
    # the struct's layout is the one the 1-bit op left
    assert [f[0] for f in N.bagua_bucket_op_t._fields_][-5:] == ["intranode", "ef_worker_carry", "ef_worker_scales",
                                                                 "ef_server_carry", "ef_server_scale"]


def test_state_sizes_and_argument_checks(built):
    from bagua_core import _native as N
    wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert N.K.bagua_mxfp4_ef_state_bytes(1025, 4, ctypes.byref(wb), ctypes.byref(sb)) == 0
    assert (wb.value, sb.value) == (4 * 1025 * 4, 1025 * 4)
    assert N.K.bagua_mxfp4_ef_state_bytes(1025, 0, ctypes.byref(wb), ctypes.byref(sb)) == 1
    assert N.K.bagua_mxfp4_ef_state_bytes(1025, 4, None, ctypes.byref(sb)) == 1
    # refusals decided before any launch (the stand-in addresses are never dereferenced on the host)
    ok = 1 << 20
    S = N.K.bagua_mxfp4_compressed_bytes(1024, 2)
    f = N.K.bagua_mxfp4_compress_ef
    assert f(F32, ok, 2048, 1024, 2, ok, S, -1, None, None) == 1          # null residual
    assert f(F32, ok, 2048, 1024, 2, ok, S, -1, ok + 2, None) == 1        # residual not 4-B aligned
    assert f(F32, ok, 2047, 1024, 2, ok, S, -1, ok, None) == 1            # partly valid input
    assert f(F32, ok, 2048, 1024, 2, ok, S - 1, -1, ok, None) == 1        # short buffer
    assert f(F32, ok, 2048, 1024, 2, ok + 8, S, -1, ok, None) == 1        # misaligned output
    assert f(F32, ok, 2048, 1024, 2, ok, S, 0, ok, None) == 1             # a target chunk
    g = N.K.bagua_mxfp4_reduce_requantize_ef
    assert g(F32, ok, S, 1024, 2, 1, ok, S, 0, None, None) == 1
    assert g(F32, ok, S, 1024, 2, 1, ok, S, 0, ok + 2, None) == 1
    assert g(F32, ok, S - 1, 1024, 2, 1, ok, S, 0, ok, None) == 1
    assert g(F32, ok, S, 1024, 2, 1, ok + 8, S, 0, ok, None) == 1
    for dt in (3, 4, 5):                                                  # U8, I64, U64
        assert f(dt, ok, 2048, 1024, 2, ok, S, -1, ok, None) == 4
        assert g(dt, ok, S, 1024, 2, 1, ok, S, 0, ok, None) == 4
    S17 = N.K.bagua_mxfp4_compressed_bytes(1024, 17)
    assert g(F32, ok, S17, 1024, 17, 1, ok, S17, 0, ok, None) == 4


def test_state_class_checks_divisibility(built):
    import bagua_core
    with pytest.raises(ValueError):
        bagua_core.MXFP4ErrorFeedbackState(1025, 4, 0)
