"""CPU tests of the MXFP6 codec's error feedback (MXFP6.md, "Error feedback"): the kernels'
block arithmetic compiled for the host (tools/mxfp6_host_check.cpp ef) against the reference
composition (tests/mxfp6_ef_reference.py), and the rule's effect on that reference.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mxfp6_ef_reference as REF
import mxfp6_reference as R
import onebit_ef_reference as OB
from oracle import oracle_np as NP
from test_mxfp8_ef_cpu import DTYPES, ROOT, ef_inputs, u32  # the inputs are MXFP8's: the same T, the same hostile blocks


@pytest.fixture(scope="module")
def host_checks(tmp_path_factory):
    """the stand-alone program (its own main), plain and under the host sanitizers; both run directly"""
    exes = []
    for name, extra in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes.append(str(tmp_path_factory.mktemp("mxfp6_ef") / name))
        subprocess.run(["g++", "-O1", *extra, "-ffp-contract=off", "-std=c++17",
                        "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                        os.path.join(ROOT, "tools", "mxfp6_host_check.cpp"), "-o", exes[-1]], check=True)
    return exes


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
        rec = np.frombuffer(out.stdout, np.uint8).reshape(-1, 25 + 128)
        assert np.array_equal(rec[:, 0], scale) and np.array_equal(rec[:, 1:25], payload)
        got = np.ascontiguousarray(rec[:, 25:]).view(np.uint32)
        bad = np.nonzero((got != u32(new)).any(axis=1))[0]
        assert bad.size == 0, (bad[:5], got[bad[:1]], u32(new)[bad[:1]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [2, 4, 8])
def test_time_averaged_error_against_the_plain_op(dtype, p, monkeypatch):
    """constant gradients, chunks of 1024: the time-averaged result's mean absolute distance from
    the true mean is at most 0.25 of the plain op's after 8 steps and 0.08 after 32 (MXFP8's
    limits, about twice what the numpy composition gave when the rule was proposed), and no
    residual exceeds 16/225 of the largest gradient: the codec's error is at most 2^-4 relative,
    so the worker residual's fixed point is r <= (g + r) / 16 = g / 15, the server sees values
    up to g * 16/15 and keeps at most 1/15 of those.  Measured: MXFP6.md, "Error feedback"."""
    import mxfp8_reference as M8   # its composed plain op over this codec's compress and decompress
    monkeypatch.setattr(M8, "compress", R.compress)
    monkeypatch.setattr(M8, "decompress", R.decompress)
    cs = 1024
    xs = OB.appendix_inputs(p, cs, dtype)
    true = np.mean([NP.to_f32(x, dtype).astype(np.float64) for x in xs], axis=0)
    err_plain = np.mean(np.abs(NP.to_f32(M8.centralized(xs, dtype, True)[0], dtype).astype(np.float64) - true))
    states = [REF.OpState(p * cs, p) for _ in range(p)]
    acc = np.zeros(p * cs, np.float64)
    gmax = max(np.abs(NP.to_f32(x, dtype)).max() for x in xs)
    ratios = {}
    for step in range(1, 33):
        acc += NP.to_f32(REF.centralized_step(NP, xs, dtype, states)[0][0], dtype).astype(np.float64)
        ratios[step] = np.mean(np.abs(acc / step - true)) / err_plain
        rmax = max(max(np.abs(s.worker).max(), np.abs(s.server).max()) for s in states)
        assert rmax <= gmax * 16 / 225, step
    print(f"p={p} dt={dtype}: plain {err_plain / np.mean(np.abs(true)):.4f} of mean|true|, ratio after 8 "
          f"{ratios[8]:.3f}, after 32 {ratios[32]:.3f}, largest residual {rmax / gmax:.4f} of the largest gradient")
    assert ratios[8] <= 0.25 and ratios[32] <= 0.08
