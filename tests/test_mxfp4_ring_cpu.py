"""CPU test of the decentralized ring op's MXFP4 arithmetic (MXFP4.md, "Ring op"): the
per-element statement the fused kernels are built from (csrc/kernels/ring_mix.hpp and
mxfp4_common.hpp: mix -> block encode -> decode -> apply), compiled for the host as the
`ring` mode of tools/mxfp4_host_check.cpp, against the composed op sequence of the numpy
reference (tests/mxfp4_reference.py::decentralized) at one rank.  All four tensors are
compared byte for byte, and so is the segment of the mixed t.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mxfp4_boundary_cases as B
import mxfp4_reference as R
import op_edge_cases as E
from oracle import oracle_np as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
N_RANDOM = 3017  # 94 blocks and a ragged one of 9 elements


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mxfp4_ring") / "mxfp4_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp4_host_check.cpp"), "-o", exe], check=True)
    return exe


def grads(rng, n, dtype, scale=1e-3):
    """gradient-like values whose magnitude changes from block to block"""
    mag = np.repeat(10.0 ** rng.uniform(-3, 2, (n + 31) // 32), 32)[:n]
    return NP.from_f32((rng.standard_normal(n) * mag * scale).astype(np.float32), dtype)


def mixed_reference(t, w, l, r, dtype):
    """the mixed t of one rank, as the composed sequence stores it before the compress"""
    m = t.copy()
    f13, f53 = float(np.float32(1.0 / 3.0)), float(np.float32(-5.0 / 3.0))
    with np.errstate(all="ignore"):
        NP.addmul_inplace(m, l, dtype, f13)
        NP.addmul_inplace(m, r, dtype, f13)
        NP.addmul_inplace(m, w, dtype, f53)
    return m


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"


def check_one_rank(host_check, t, w, l, r, dtype, what):
    n = t.size
    maxf = "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in (t, w, l, r))
    out = subprocess.run([host_check, "ring", maxf, str(dtype), str(n)], input=raw, capture_output=True,
                         check=True).stdout
    es = 4 if dtype == F32 else 2
    assert len(out) == 4 * n * es + R.compressed_bytes(n, 1), what
    got = [np.frombuffer(out[k * n * es:(k + 1) * n * es], R.STORAGE[dtype]) for k in range(4)]
    with np.errstate(all="ignore"):
        want = R.decentralized([t], [w], [l], [r], dtype)
        seg = R.compress(mixed_reference(t, w, l, r, dtype), dtype, 1)
    for name, g, wk in zip(("t", "weight", "left", "right"), got, want):
        same_bytes(g, wk[0], f"{what}: {name}")
    same_bytes(np.frombuffer(out[4 * n * es:], np.uint8), seg, f"{what}: segment")


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_gradients(host_check, dtype):
    rng = np.random.default_rng(400 + dtype)
    t, w, l, r = (grads(rng, N_RANDOM, dtype) for _ in range(4))
    check_one_rank(host_check, t, w, l, r, dtype, "random")


@pytest.mark.parametrize("cls", E.RING_CLASSES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_classes(host_check, dtype, cls):
    a = E.build_ring(cls, 1, N_RANDOM, dtype, E.case_rng("mxfp4 ring cpu", dtype, cls))
    check_one_rank(host_check, a["t"][0], a["w"][0], a["l"][0], a["r"][0], dtype, cls)


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_table(host_check, dtype):
    """t = the table, L = R = W = 0: the mix returns t (a -0 would become +0), so every tie, every
    scale byte and every amax position goes through the op's encode and decode"""
    tab = B.table(dtype)
    t = tab.x.copy()
    zero = np.zeros_like(t)
    m = mixed_reference(t, zero, zero, zero, dtype)
    mv, tv = NP.to_f32(m, dtype), NP.to_f32(t, dtype)
    assert np.array_equal(mv, tv) and not np.signbit(mv[mv == 0]).any(), "the mix must hand the table on"
    check_one_rank(host_check, t, zero.copy(), zero.copy(), zero.copy(), dtype, "boundary table")
