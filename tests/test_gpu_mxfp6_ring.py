"""GPU tests of the ring op's fused MXFP6 kernels (csrc/kernels/mxfp6_ring.hip, MXFP6.md "Ring op"): the
three C entries, the dispatch of decentralized() and the op, byte for byte against the composed sequence
of the float64 reference (tests/mxfp6_reference.py), guards behind every tensor and the segment.

Sizes (a wave tile is w = 512 / 1024 elements, a workgroup 4 w): 5; 32, 64, 96, 128 (payload slack 24, 16,
8, 0 bytes); w, w - 32, w + 32; w + 17 (a ragged block, a partial vector and, for f32, a group of four lanes
with one valid element); 9 w + 17 with the grid caps at 2: a second, ragged grid-stride iteration."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp6_reference as R
import op_edge_cases as E
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
# `composed` puts this codec's compress and decompress into mxfp8_reference, so that module's composed ops
# and the helpers of test_gpu_mxfp8_ring that call it (reference_apply, ring_case) compute this codec's results
from test_gpu_mxfp6 import composed  # noqa: F401
from test_gpu_mxfp8_ring import (INVALID_ARG, OK, U8, UNSUPPORTED, WAVE_TILE, bc, check4, guarded, ptrs,  # noqa: F401
                                 reference_apply, ring_case)
from test_gpu_op_edges import KernelNames
from test_mxfp4_ring_cpu import grads, mixed_reference, same_bytes
from test_mxfp6_cpu import code_table, tie_table

pytestmark = pytest.mark.gpu

F32, F16, BF16 = DTYPES = [0, 1, 2]
GRID_KNOBS = ["BAGUA_TUNE_MX6_RING_%s_BLOCKS" % k for k in ("MIX", "APPLY", "ONE_RANK")]
FUSED = ["mxfp6_ring_mix_kernel", "mxfp6_ring_apply_kernel"]
ONE_RANK = ["mxfp6_ring_one_rank_kernel"]


def check_entries(K, M, dtype, arrs, what, hostile=False, one_segment=False):
    """the mix, the apply (on three different segments, or on one in all three places) and the one-rank kernel"""
    t, w, l, r = arrs
    n, rng = t.size, np.random.default_rng(t.size)
    with np.errstate(all="ignore"):
        seg = R.compress(mixed_reference(t, w, l, r, dtype), dtype, 1)
        one = [x[0] for x in M.decentralized([t], [w], [l], [r], dtype)]
    assert K.bagua_mxfp6_compressed_bytes(n, 1) == seg.size
    (ds, full), pad = guarded(arrs, dtype), np.full(32, 0xAB, np.uint8)
    out = torch.from_numpy(np.concatenate([np.zeros_like(seg) + 0xAB, pad])).cuda()
    dt, dw, dl, dr = ptrs(ds)
    assert K.bagua_ring_mix_mxfp6(dtype, dt, dl, dr, dw, n, out.data_ptr(), seg.size, None) == OK, what
    same_bytes(host(out, U8), np.concatenate([seg, pad]), f"{what}: segment, both slacks and the bytes behind it")
    check4(ds, arrs, full, dtype, f"{what}: after the mix")
    segs = [seg] * 3 if one_segment else [seg] + [R.compress(grads(rng, n, dtype), dtype, 1) for _ in range(2)]
    if hostile:  # a hostile peer: NaN, smallest and largest scale bytes; the largest magnitude of both signs and -0
        sb, nb = R.scale_bytes(n), R.blocks(n)
        for s, first in zip(segs, (0, 3, 6)):
            s[first:first + 3] = 0xFF, 0, 254
            codes = R.unpack(s[sb:sb + 24 * nb])
            codes[first:first + 4, ::3] = np.resize([0x1F, 0x3F, 0x20], 11)
            s[sb:sb + 24 * nb] = R.pack(codes).ravel()
    dsegs = {id(s): torch.from_numpy(s).cuda() for s in segs}  # one array in several places is one buffer
    assert K.bagua_ring_apply_mxfp6(dtype, *[dsegs[id(s)].data_ptr() for s in segs], seg.size, n, *ptrs(ds), None) == OK
    for s in segs:
        same_bytes(host(dsegs[id(s)], U8), s, f"{what}: a segment after the apply")
    check4(ds, reference_apply(segs, w, l, r, dtype), full, dtype, f"{what}: after the apply")
    ds, full = guarded(arrs, dtype)
    assert K.bagua_ring_one_rank_mxfp6(dtype, *ptrs(ds), n, None) == OK, what
    check4(ds, one, full, dtype, f"{what}: one rank")


@pytest.mark.parametrize("dtype", DTYPES)
def test_entry_points_against_the_reference(bc, composed, dtype, monkeypatch):
    w = WAVE_TILE[dtype]
    rng = np.random.default_rng(600 + dtype)
    for n, hostile in [(5, 0), (32, 0), (64, 0), (96, 0), (128, 0), (w, 0), (w - 32, 0), (w + 32, 0), (w + 17, 0),
                       (w + 17, 1), (9 * w + 17, 0)]:
        for k in GRID_KNOBS:
            monkeypatch.setenv(k, "2") if n > 9 * w else monkeypatch.delenv(k, raising=False)
        check_entries(bc._native.K, composed, dtype, [grads(rng, n, dtype) for _ in range(4)], f"dtype={dtype} n={n}",
                      hostile)


@pytest.mark.parametrize("dtype", DTYPES)
def test_code_and_tie_tables(bc, composed, dtype):
    """t = both tables, L = R = W = 0, the one segment in all three places: every code at every position, every tie"""
    t = NP.from_f32(np.concatenate([code_table(dtype)[0], tie_table(dtype)[0]]).astype(np.float32).ravel(), dtype)
    check_entries(bc._native.K, composed, dtype, [t] + [np.zeros_like(t)] * 3, "tables", one_segment=True)


def check_op(bc, comms, entry, data, want, dtype, what, offset=0, num_elem=None):
    """test_gpu_mxfp8_ring's check_op with this codec's method: returns the kernel names of rank 0"""
    N, names, offs = bc._native, [], [offset] + [0] * 8
    dts = {k: [dev(np.concatenate([np.zeros(o, a.dtype), a]), dtype)[o:] for a, o in zip(data[k], offs)]
           for k in "twlr"}
    op = getattr(N.C, "bagua_decentralized_low_precision_" + entry)

    def rank(r):
        raws = [bc.BaguaTensorPy(dts[k][r], f"{k}{r}").raw() for k in "twlr"]
        for x in raws:
            x.num_elem = num_elem or x.num_elem
        args = (comms[r].handle, *[ctypes.byref(x) for x in raws], N.COMPRESSION_MXFP6)
        args += (3,) * (entry == "pipelined")  # the piece count
        if r == 0:
            with KernelNames(N, comms[0]) as k:
                rc = op(*args)
            names.extend(k.names)
        else:
            rc = op(*args)
        N.check(rc, f"{entry} rank {r}")

    torch.cuda.synchronize()
    run_ranks(rank, len(comms))
    for k, wk in zip("twlr", want or []):
        for r in range(len(comms)):
            same_bytes(host(dts[k][r], dtype), wk[r], f"{what}: {k} rank {r}")
    return names


def unfused(names):  # the elementwise sequence and none of the three new kernels
    return "binary_kernel" in names and "mxfp6_decode_kernel" in names and not set(names) & set(FUSED + ONE_RANK)


def test_op_on_hostile_inputs(bc, composed):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(4, 0)
    for cls in E.RING_CLASSES:
        names = check_op(bc, comms, "synchronous", *ring_case(cls, 4, F16), F16, cls)
        assert cls != E.RING_CLASSES[0] or names == FUSED, names


@pytest.mark.parametrize("p", [1, 2, 3])
def test_every_dispatch_path(bc, composed, p, monkeypatch):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    for dtype in (F32, BF16):
        case, off = ring_case("benign", p, dtype), 1 if dtype == F32 else 2  # 4 bytes: aligned copies
        kernels = ONE_RANK if p == 1 else FUSED
        assert check_op(bc, comms, "synchronous", *case, dtype, "synchronous") == kernels
        assert check_op(bc, comms, "pipelined", *case, dtype, "pipelined, 3 pieces") == kernels  # stays unpieced
        assert check_op(bc, comms, "synchronous", *case, dtype, "4-byte offset", offset=off) == kernels
        assert unfused(check_op(bc, comms, "synchronous_unfused", *case, dtype, "unfused"))
        for env in ("BAGUA_MXFP6_RING_FUSED",) + (("BAGUA_ONE_RANK_FUSED",) if p == 1 else ()):
            monkeypatch.setenv(env, "0")  # the composed steps; at one rank mix + apply, `mine` in all three places
            names = check_op(bc, comms, "synchronous", *case, dtype, env + "=0")
            assert names == FUSED if env == "BAGUA_ONE_RANK_FUSED" else unfused(names), names
            monkeypatch.delenv(env)
        # dispatch only: a partly valid tensor runs the composed steps (their bytes are the unfused entry's business)
        assert unfused(check_op(bc, comms, "synchronous", case[0], None, dtype, "partly valid", num_elem=4099 - 5))


def test_refusals(bc):
    K, n = bc._native.K, 1000
    S = R.compressed_bytes(n, 1)
    hosts = [grads(np.random.default_rng(650), n + 8, F32) for _ in range(4)]
    ds = [dev(a, F32) for a in hosts]
    out = torch.full((S + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    (t, w, l, r), o = ptrs(ds), out.data_ptr()
    mix, app, one = K.bagua_ring_mix_mxfp6, K.bagua_ring_apply_mxfp6, K.bagua_ring_one_rank_mxfp6
    for rc in (mix(F32, t + 4, l, r, w, n, o, S, None), mix(F32, t, l, r, w + 4, n, o, S, None),
               mix(3, t, l, r, w, n, o, S, None), app(F32, o, o, o, S, n, t, w, l + 4, r, None),
               app(7, o, o, o, S, n, t, w, l, r, None), one(F32, t, w, l, r + 4, n, None), one(5, t, w, l, r, n, None)):
        assert rc == UNSUPPORTED  # a tensor that is not 16-B aligned, a dtype outside the three (U8 and beyond)
    for rc in (mix(F32, None, l, r, w, n, o, S, None), mix(F32, t, l, r, w, n, None, S, None),
               mix(F32, t, l, r, w, 0, o, S, None), mix(F32, t, l, r, w, -1, o, S, None),
               mix(F32, t, l, r, w, n, o, S - 1, None), mix(F32, t, l, r, w, n, o + 8, S, None),
               app(F32, o, None, o, S, n, t, w, l, r, None), app(F32, o, o, o, S, n, t, None, l, r, None),
               app(F32, o, o, o, S, 0, t, w, l, r, None), app(F32, o, o, o, S - 1, n, t, w, l, r, None),
               app(F32, o, o, o + 4, S, n, t, w, l, r, None), one(F32, t, w, None, r, n, None),
               one(F32, t, w, l, r, 0, None)):
        assert rc == INVALID_ARG  # a null pointer, n <= 0, a short buffer, a misaligned one
    for d, h in zip(ds + [out], hosts + [np.full(S + 16, 0xAB, np.uint8)]):  # nothing was launched
        same_bytes(host(d, F32), h, "a buffer after the refusals")
