"""CPU tests of the 1-bit codec's error feedback: the new C-ABI surface, and the
algorithm itself on the oracle composition (tests/onebit_ef_reference.py) -- zero
state equals the plain op, the time-averaged output beats the memoryless op, and
the residuals telescope.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import onebit_ef_reference as REF
from oracle import oracle_np as NP
from oracle import simulate
from test_abi import LIB, built, declared, exported  # noqa: F401  (built: fixture)

F32, F16, BF16 = 0, 1, 2

KERNEL_SYMBOLS = ["bagua_onebit_ef_state_bytes", "bagua_onebit_compress_ef", "bagua_onebit_encode_range_ef",
                  "bagua_onebit_finalize_ef", "bagua_onebit_reduce_requantize_ef"]
CORE_SYMBOLS = ["bagua_centralized_onebit_error_feedback", "bagua_tensor_compress_error_feedback"]


def test_new_symbols_declared_and_exported(built):
    k_decl, c_decl = declared("bagua_kernels.h"), declared("bagua_core.h")
    k_exp = exported(os.path.join(LIB, "libbagua_kernels.so"))
    c_exp = exported(os.path.join(LIB, "libbagua_core.so"))
    assert not [n for n in KERNEL_SYMBOLS if n not in k_decl or n not in k_exp]
    assert not [n for n in CORE_SYMBOLS if n not in c_decl or n not in c_exp]
    from bagua_core import _native as N
    assert set(KERNEL_SYMBOLS) <= set(N.KERNEL_SIGNATURES) and set(CORE_SYMBOLS) <= set(N.CORE_SIGNATURES)
    src = open(os.path.join(os.path.dirname(LIB), "..", "include", "bagua_core.h")).read()
    assert "BAGUA_BUCKET_OP_CENTRALIZED_ONEBIT_ERROR_FEEDBACK" in src
    # the bucket op struct of the binding matches the header's (the state descriptors come last)
    assert [f[0] for f in N.bagua_bucket_op_t._fields_][-5:] == ["intranode", "ef_worker_carry", "ef_worker_scales",
                                                                 "ef_server_carry", "ef_server_scale"]


def test_state_sizes_and_argument_checks(built):
    from bagua_core import _native as N
    cb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert N.K.bagua_onebit_ef_state_bytes(1025, 4, ctypes.byref(cb), ctypes.byref(sb)) == 0
    assert (cb.value, sb.value) == (4 * 1025 * 4, 16)
    assert N.K.bagua_onebit_ef_state_bytes(1025, 0, ctypes.byref(cb), ctypes.byref(sb)) == 1
    assert N.K.bagua_onebit_ef_state_bytes(1025, 4, None, ctypes.byref(sb)) == 1
    # refusals that are decided before any launch (pointers are never dereferenced on the host)
    ok = 1 << 20  # a 16-B aligned, non-null stand-in address
    S = N.K.bagua_onebit_compressed_bytes(1024, 2)
    base = [ok, 2048, 1024, 2, ok, S, ok, 1 << 16]
    f = N.K.bagua_onebit_compress_ef
    assert f(F32, *base, -1, None, ok, None) == 1             # null carry
    assert f(F32, *base, -1, ok, ok + 4, None) == 1           # misaligned scales
    assert f(F32, *base, -1, ok + 8, ok, None) == 1           # misaligned carry
    assert f(F32, *base, 0, ok, ok, None) == 1                # a target chunk
    assert f(F32, ok, 2047, 1024, 2, ok, S, ok, 1 << 16, -1, ok, ok, None) == 1  # partly valid input
    for dt in (3, 4, 5):                                      # U8, I64, U64
        assert f(dt, *base, -1, ok, ok, None) == 1
        assert N.K.bagua_onebit_reduce_requantize_ef(dt, ok, S, 1024, 2, 1, ok, S, 0, ok, 1 << 16, ok, ok, None) == 1
    assert N.K.bagua_onebit_reduce_requantize_ef(F32, ok, S, 1024, 2, 1, ok, S, 0, ok, 1 << 16, ok + 4, ok, None) == 1
    S17 = N.K.bagua_onebit_compressed_bytes(1024, 17)
    assert N.K.bagua_onebit_reduce_requantize_ef(F32, ok, S17, 1024, 17, 1, ok, S17, 0, ok, 1 << 16, ok, ok, None) == 4
    assert N.K.bagua_onebit_encode_range_ef(F32, *base, 0, 1, ok, None, None) == 1


def test_state_class_checks_divisibility(built):
    import bagua_core
    with pytest.raises(ValueError):
        bagua_core.OneBitErrorFeedbackState(1025, 4, 0)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_reference_backends_agree(oracle_c, dt):
    """oracle_c and oracle_np through the helper: payloads and state equal byte for byte, 4 steps"""
    p, cs = 4, 1025
    rng = np.random.default_rng(5)
    sa = [REF.OpState(p * cs, p) for _ in range(p)]
    sb = [REF.OpState(p * cs, p) for _ in range(p)]
    wa, wb = REF.WorkerState(p * cs, p), REF.WorkerState(p * cs, p)
    for step in range(4):
        xs = [NP.from_f32((rng.standard_normal(p * cs) * 1e-3 + 0.0005 * r).astype(np.float32), dt) for r in range(p)]
        oa, pa = REF.centralized_step(oracle_c, xs, dt, sa)
        ob, pb = REF.centralized_step(NP, xs, dt, sb)
        for r in range(p):
            assert np.array_equal(pa[r], pb[r]), (step, r)
            assert np.array_equal(oa[r].view(np.uint8), ob[r].view(np.uint8)), (step, r)
            for f in ("wc", "ws", "sc", "ss"):
                assert np.array_equal(getattr(sa[r], f).view(np.uint32), getattr(sb[r], f).view(np.uint32)), (step, r, f)
        assert np.array_equal(REF.compress_ef(oracle_c, xs[0], dt, p, wa), REF.compress_ef(NP, xs[0], dt, p, wb))
        assert np.array_equal(wa.carry.view(np.uint32), wb.carry.view(np.uint32))
        assert np.array_equal(wa.scales.view(np.uint32), wb.scales.view(np.uint32))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_zero_state_equals_plain_op(oracle_c, dt, p):
    cs = 1025
    xs = REF.appendix_inputs(p, cs, dt)
    want = simulate.centralized_low_precision(oracle_c, xs, dt, True, method="OneBit")
    got, sent = REF.centralized_step(oracle_c, xs, dt, [REF.OpState(p * cs, p) for _ in range(p)])
    for r in range(p):
        assert np.array_equal(got[r].view(np.uint8), want[r].view(np.uint8)), r
        assert np.array_equal(sent[r], oracle_c.compress_onebit(xs[r], dt, p)), r


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("p", [2, 4, 8])
@pytest.mark.parametrize("cs", [3000, 1025, 2048])
def test_error_against_memoryless_op(oracle_c, dt, p, cs):
    """constant gradients, 32 steps: the time-averaged output's mean absolute error against
    the true mean is at most half the memoryless op's"""
    steps = 32
    xs = REF.appendix_inputs(p, cs, dt)
    true = np.mean([NP.to_f32(x, dt).astype(np.float64) for x in xs], axis=0)
    plain = NP.to_f32(simulate.centralized_low_precision(oracle_c, xs, dt, True, method="OneBit")[0], dt)
    err_plain = np.mean(np.abs(plain.astype(np.float64) - true))
    states = [REF.OpState(p * cs, p) for _ in range(p)]
    acc = np.zeros(p * cs, np.float64)
    for _ in range(steps):
        outs, _ = REF.centralized_step(oracle_c, xs, dt, states)
        acc += NP.to_f32(outs[0], dt).astype(np.float64)
    err_ef = np.mean(np.abs(acc / steps - true))
    print(f"p={p} cs={cs} dt={dt}: memoryless {err_plain / np.mean(np.abs(true)):.3f} of mean|true|, "
          f"error feedback {err_ef / np.mean(np.abs(true)):.3f}, ratio {err_ef / err_plain:.3f}")
    assert err_ef <= 0.5 * err_plain


@pytest.mark.parametrize("dt", [F32, BF16])
def test_telescoping_identity(oracle_c, dt):
    """the codec alone, one gradient held for K = 64 steps: K g - sum(decoded) is the final
    residual (every step's residual is what the next one adds back)"""
    K, n = 64, 3000
    g = REF.appendix_inputs(1, n, dt)[0]
    g32 = NP.to_f32(g, dt)
    st = REF.WorkerState(n, 1)
    total = np.zeros(n, np.float64)
    dec = g.copy()
    for _ in range(K):
        buf = REF.compress_ef(oracle_c, g, dt, 1, st)
        oracle_c.decompress_onebit(buf, 1, dec, dt)
        total += NP.to_f32(dec, dt).astype(np.float64)
    s = np.repeat(st.scales, n)
    residual = st.carry - REF.stored(np.where(st.carry < 0, -s, s).astype(np.float32), dt)
    diff = np.max(np.abs(K * g32.astype(np.float64) - total - residual))
    bound = 1e-3 * np.mean(np.abs(g32))
    print(f"dt={dt}: max |K g - sum decoded - residual| = {diff:.3e}, {diff / np.mean(np.abs(g32)):.2e} of mean|g|")
    assert diff <= bound
