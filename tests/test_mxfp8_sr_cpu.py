"""CPU tests of MXFP8 stochastic rounding (MXFP8.md): the kernels' arithmetic compiled for the host, plain and
under the host sanitizers, against tests/mxfp8_sr_reference.py; its unbiasedness; the op simulated.  No GPU."""
import subprocess

import numpy as np
import pytest

import mxfp8_boundary_cases as B
import mxfp8_reference as R
import mxfp8_sr_reference as SR
import onebit_ef_reference as OB
from test_mxfp8_cpu import hostile_blocks, random_blocks
from test_mxfp8_ef_cpu import host_checks  # noqa: F401  (fixture: tools/mxfp8_host_check.cpp, plain and sanitized)

F32, DTYPES = 0, [0, 1, 2]
KEY = SR.key(0xB0A8, 3, 1, 0)


def run_host(exe, mode, dtype, args, x, extra=()):
    raw = np.concatenate([x.astype(np.float32).view(np.uint32), *extra], axis=1).tobytes()
    out = subprocess.run([exe, mode, "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)] + args, input=raw,
                         capture_output=True)
    assert out.returncode == 0 and not out.stderr, out.stderr.decode()
    got = np.frombuffer(out.stdout, np.uint8).reshape(-1, 33)
    return got[:, 0], got[:, 1:]


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_against_the_reference(host_checks, dtype):  # noqa: F811
    """under a key from an even and an odd first index (a pair of the hash then straddles every group of 8), and under
    explicit r: r = 0 gives the floor code, r = 0xffff moves no grid value and every F >= 1 up; no magnitude 0x7F;
    signs kept; the scale bytes are the plain encode's"""
    x = np.concatenate([random_blocks(dtype, 2000, 141 + dtype), hostile_blocks(dtype), B.table(dtype).values()])
    p_scale, _ = R.encode_blocks(x, dtype)
    ok = p_scale != 0xFF
    floor_code, F, _ = SR.floor_code_and_fraction(R.scaled(x, dtype)[1])
    assert (~ok).any() and (p_scale == 0).any() and (F[ok] == 0).sum() > 1000 and (F[ok] == 32768).sum() > 300
    keyed = [("sr", ["%016x" % KEY, str(j0)], [], SR.rbits(KEY, np.uint64(j0) + np.arange(x.size, dtype=np.uint64)))
             for j0 in (0, 5 * 32 + 7)]
    fixed = [("srr", [], [np.full(x.shape, rv, np.uint32)], rv) for rv in (0, 1, 0x7FFF, 0x8000, 0xFFFF)]
    for mode, args, extra, r in keyed + fixed:
        scale, payload = SR.encode_blocks_sr(x, dtype, extra[0] if extra else r)
        for exe in host_checks:
            got = run_host(exe, mode, dtype, args, x, extra)
            assert np.array_equal(got[0], scale) and np.array_equal(got[1], payload), (mode, args, r)
        assert np.array_equal(scale, p_scale) and ((payload & 0x7F) != R.NAN_CODE).all()
        assert np.array_equal((payload >> 7)[ok], np.signbit(x)[ok])
        if extra:
            assert np.array_equal((payload & 0x7F)[ok], (floor_code + (F + r >= 65536))[ok])


def test_unbiased(host_checks):  # noqa: F811
    """mx8_encode_block_sr (the host program's `srs` mode) on 4096 f32 elements N(0, 1e-3^2), K = 1024 steps of one seed:
    every mean decode within 5 s 2^e / (2 sqrt(K)) of x, five standard deviations of the worst Bernoulli draw (worst
    element: 3.47 of those units); round-to-nearest misses that bound for 0.83 of the elements"""
    K = 1024
    x = (np.random.default_rng(2024).standard_normal(4096) * 1e-3).astype(np.float32).astype(np.float64).reshape(-1, 32)
    scale, payload = run_host(host_checks[0], "srs", F32, ["5eed", str(K)], x)
    first = SR.encode_blocks_sr(x, F32, SR.rbits(SR.key(0x5EED, 0), np.arange(x.size, dtype=np.uint64)))
    assert np.array_equal(payload[:x.shape[0]], first[1]) and np.array_equal(scale[:x.shape[0]], first[0])
    e, y = R.scaled(x, F32)
    unit = SR.floor_code_and_fraction(y)[2] * np.ldexp(1.0, e)[:, None] / (2.0 * np.sqrt(K))
    decode = lambda s, p: R.decode_blocks(s, p, F32).astype(np.float64).reshape(-1, *x.shape)  # noqa: E731
    worst = (np.abs(decode(scale, payload).mean(axis=0) - x) / unit).max()
    missed = (np.abs(decode(*R.encode_blocks(x, F32))[0] - x) > 5.0 * unit).mean()
    print(f"worst element {worst:.2f} s 2^e / (2 sqrt(K)), bound 5; round-to-nearest misses {missed:.3f} of the elements")
    assert worst <= 5.0 and missed > 0.5


@pytest.mark.parametrize("p", [2, 4, 8])
def test_time_averaged_error_against_the_plain_op(p):
    """constant gradients, chunks of 1024: the time-averaged result's relative L2 error falls by 1.5 or more between 16
    and 64 steps (0.5 expected) and ends below the plain op's (0.0106-0.0132 -> 0.0052-0.0066, plain 0.0295-0.0380)"""
    xs = OB.appendix_inputs(p, 1024, F32)
    true = np.mean([x.astype(np.float64) for x in xs], axis=0)
    rel = lambda v: np.linalg.norm(v - true) / np.linalg.norm(true)  # noqa: E731
    plain = rel(R.centralized(xs, F32, True)[0].astype(np.float64))
    acc, curve = np.zeros(p * 1024), {}
    for step in range(64):
        acc += SR.centralized_sr(xs, F32, True, 0xC0FFEE, step)[0].astype(np.float64)
        curve[step + 1] = rel(acc / (step + 1))
    print(f"p={p}: plain {plain:.5f}, stochastic " + ", ".join(f"{k}: {curve[k]:.5f}" for k in (1, 4, 16, 64)))
    assert curve[64] * 1.5 <= curve[16] and curve[64] < plain
