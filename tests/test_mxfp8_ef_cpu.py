"""CPU tests of the MXFP8 codec's error feedback (MXFP8.md, "Error feedback"): the kernels'
block arithmetic compiled for the host (tools/mxfp8_host_check.cpp ef) against the reference
composition (tests/mxfp8_ef_reference.py), and the rule's effect on that reference.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mxfp8_ef_reference as REF
import mxfp8_reference as R
import onebit_ef_reference as OB
from oracle import oracle_np as NP
from test_mxfp8_cpu import hostile_blocks, random_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [0, 1, 2]  # f32, f16, bf16


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def host_checks(tmp_path_factory):
    """the stand-alone program (its own main), plain and under the host sanitizers; both run directly"""
    exes = []
    for name, extra in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes.append(str(tmp_path_factory.mktemp("mxfp8_ef") / name))
        subprocess.run(["g++", "-O1", *extra, "-ffp-contract=off", "-std=c++17",
                        "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                        os.path.join(ROOT, "tools", "mxfp8_host_check.cpp"), "-o", exes[-1]], check=True)
    return exes


def ef_inputs(dtype):
    """(x, e) blocks as f32: random blocks under residuals of every relative size, the plain codec's hostile blocks
    (all ties, NaN, +-inf, -0, the largest finite T) under zero and non-zero residuals, and the six rows below"""
    rng = np.random.default_rng(88 + dtype)
    x = random_blocks(dtype, 3000, 51 + dtype)
    e = rng.standard_normal(x.shape) * np.abs(x).max(axis=1, keepdims=True) * 10.0 ** rng.uniform(-4, 0, (len(x), 1))
    e[::7] = 0.0
    h = hostile_blocks(dtype)
    he = rng.standard_normal(h.shape) * np.abs(np.where(np.isfinite(h), h, 0)).max(axis=1, keepdims=True) * 0.25
    mx = R.MAX_FINITE[dtype]
    sx, se = np.zeros((6, 32)), np.zeros((6, 32))
    sx[1, :] = -0.0                                           # row 0 all zero; -0 + (+0) = +0
    sx[2, :16], se[2, :16] = -0.0, -0.0                       # -0 + -0 = -0
    sx[2, 16:], se[2, 16:] = 1.0, -1.0                        # x + e = +0
    sx[3, :2], se[3, :2], sx[3, 2:] = (mx, -mx), (mx * 2.0 ** -6, -mx * 2.0 ** -6), 1.0   # past M: clamped
    sx[4, :], se[4, 9], se[4, 10] = 3.0, np.nan, 0.25         # NaN in e
    sx[5, :], se[5, :2], se[5, 2:] = 1.0, (np.inf, -np.inf), 0.125   # inf in e
    xs, es = np.concatenate([x, h, h, sx]), np.concatenate([e, np.zeros(h.shape), he, se])
    with np.errstate(over="ignore", invalid="ignore"):
        x32 = NP.to_f32(NP.from_f32(xs.astype(np.float32).ravel(), dtype), dtype).astype(np.float32).reshape(xs.shape)
        return x32, es.astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_matches_the_reference(host_checks, dtype):
    x32, e32 = ef_inputs(dtype)
    scale, payload, new = REF.ef_blocks(x32, e32, dtype)
    assert (scale == 0xFF).sum() >= 3 and (scale == 0).sum() >= 2 and np.isinf(x32).any()
    assert not u32(new[scale == 0xFF]).any()
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    raw = np.concatenate([x32, e32], axis=1).astype(np.float32).tobytes()
    for exe in host_checks:
        out = subprocess.run([exe, "ef", maxf, str(dtype)], input=raw, capture_output=True)
        assert out.returncode == 0 and not out.stderr, out.stderr.decode()
        rec = np.frombuffer(out.stdout, np.uint8).reshape(-1, 33 + 128)
        assert np.array_equal(rec[:, 0], scale) and np.array_equal(rec[:, 1:33], payload)
        got = np.ascontiguousarray(rec[:, 33:]).view(np.uint32)
        bad = np.nonzero((got != u32(new)).any(axis=1))[0]
        assert bad.size == 0, (bad[:5], got[bad[:1]], u32(new)[bad[:1]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [2, 4, 8])
def test_time_averaged_error_against_the_plain_op(dtype, p):
    """constant gradients, chunks of 1024: the time-averaged result's mean absolute distance from
    the true mean is at most 0.25 of the plain op's after 8 steps and 0.08 after 32 (measured
    here: 0.126-0.142 and 0.015-0.041; the limits are about twice that, for other seeds), and no
    residual exceeds 2^-4 of the largest gradient (the codec's relative rounding error; measured:
    at most 0.048)"""
    cs = 1024
    xs = OB.appendix_inputs(p, cs, dtype)
    true = np.mean([NP.to_f32(x, dtype).astype(np.float64) for x in xs], axis=0)
    err_plain = np.mean(np.abs(NP.to_f32(R.centralized(xs, dtype, True)[0], dtype).astype(np.float64) - true))
    states = [REF.OpState(p * cs, p) for _ in range(p)]
    acc = np.zeros(p * cs, np.float64)
    gmax = max(np.abs(NP.to_f32(x, dtype)).max() for x in xs)
    ratios = {}
    for step in range(1, 33):
        acc += NP.to_f32(REF.centralized_step(NP, xs, dtype, states)[0][0], dtype).astype(np.float64)
        ratios[step] = np.mean(np.abs(acc / step - true)) / err_plain
        rmax = max(max(np.abs(s.worker).max(), np.abs(s.server).max()) for s in states)
        assert rmax <= 2.0 ** -4 * gmax, step
    print(f"p={p} dt={dtype}: plain {err_plain / np.mean(np.abs(true)):.4f} of mean|true|, ratio after 8 "
          f"{ratios[8]:.3f}, after 32 {ratios[32]:.3f}, largest residual {rmax / gmax:.4f} of the largest gradient")
    assert ratios[8] <= 0.25 and ratios[32] <= 0.08
