"""GPU tests of the decentralized ring op's fused MXFP8 kernels (csrc/kernels/mxfp8_ring.hip,
MXFP8.md "Ring op"): the three C entries, the dispatch of decentralized() in comm_ops.cpp and
the op, byte for byte against the composed sequence of the float64 numpy reference
(tests/mxfp8_reference.py), guard elements behind every tensor and the segment included.
Every test runs with BAGUA_MXFP8_HWCVT=1 and =0.

Sizes, from the shipped geometry: a lane of the mix and of the one-rank kernel owns one 16-B
vector (4 f32 / 8 16-bit elements) of each of two blocks, so a wave tile is w = 512 / 1024
elements and a workgroup of four waves covers 4 w; a lane of the apply owns two vector
positions and its workgroup covers 4 w as well.  Hence 5 (less than a block), 32, w, w - 32,
w + 32, w + 17 (a partial block and a partial vector), and 9 w + 17 with the three grid caps at
2 workgroups = 8 wave tiles: tile 8 is the second grid-stride iteration and is ragged."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp8_boundary_cases as B
import mxfp8_reference as R
import op_edge_cases as E
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_op_edges import KernelNames
from test_mxfp4_ring_cpu import grads, mixed_reference, same_bytes

pytestmark = pytest.mark.gpu

F32, F16, BF16 = DTYPES = [0, 1, 2]
OK, INVALID_ARG, UNSUPPORTED, U8 = 0, 1, 4, 3  # status codes; the dtype code of bytes
WAVE_TILE = {F32: 512, F16: 1024, BF16: 1024}
GRID_KNOBS = ["BAGUA_TUNE_MX8_RING_%s_BLOCKS" % k for k in ("MIX", "APPLY", "ONE_RANK")]
GUARD, HUGE = 40, 6e4  # elements behind every tensor, never to be read or written
FUSED = ["mxfp8_ring_mix_kernel", "mxfp8_ring_apply_kernel"]
ONE_RANK = ["mxfp8_ring_one_rank_kernel"]
NAMES = ("t", "weight", "left", "right")


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(params=["1", "0"], ids=["hwcvt", "arith"], autouse=True)
def hwcvt(request, monkeypatch):
    monkeypatch.setenv("BAGUA_MXFP8_HWCVT", request.param)


def guarded(arrays, dtype):
    """each array followed by GUARD huge elements: the device tensors and their host copies"""
    full = [np.concatenate([x, NP.from_f32(np.full(GUARD, HUGE, np.float32), dtype)]) for x in arrays]
    return [dev(f, dtype) for f in full], full


def check4(ds, want, full, dtype, what):
    """t, w, l, r on the device against `want`, and the guards behind them against the host copies"""
    for name, d, wk, h in zip(NAMES, ds, want, full):
        same_bytes(host(d, dtype), np.concatenate([wk, h[wk.size:]]), f"{what}: {name}")


def reference_apply(segs, w, l, r, dtype):
    """decompress / add with three segments (mine, from_left, from_right): t, w, l, r"""
    with np.errstate(all="ignore"):
        t = R.decompress(segs[1], 1, np.zeros(w.size, R.STORAGE[dtype]), dtype)
        l = NP.add_inplace(l.copy(), t, dtype)
        r = NP.add_inplace(r.copy(), R.decompress(segs[2], 1, t, dtype), dtype)
        t = NP.add_inplace(R.decompress(segs[0], 1, t, dtype), w, dtype)
    return t, t.copy(), l, r


def ptrs(ds):
    return [d.data_ptr() for d in ds]


def check_entries(K, dtype, arrs, what, hostile=False, one_segment=False):
    """the mix, the apply (on three different segments, or on one in all three places) and the one-rank kernel"""
    t, w, l, r = arrs
    n, rng = t.size, np.random.default_rng(t.size)
    with np.errstate(all="ignore"):
        seg = R.compress(mixed_reference(t, w, l, r, dtype), dtype, 1)
        one = [x[0] for x in R.decentralized([t], [w], [l], [r], dtype)]
    (ds, full), pad = guarded(arrs, dtype), np.full(32, 0xAB, np.uint8)
    out = torch.from_numpy(np.concatenate([np.zeros_like(seg) + 0xAB, pad])).cuda()
    dt, dw, dl, dr = ptrs(ds)
    assert K.bagua_ring_mix_mxfp8(dtype, dt, dl, dr, dw, n, out.data_ptr(), seg.size, None) == OK, what
    same_bytes(host(out, U8), np.concatenate([seg, pad]), f"{what}: segment and the bytes behind it")
    check4(ds, arrs, full, dtype, f"{what}: after the mix")
    segs = [seg] * 3 if one_segment else [seg] + [R.compress(grads(rng, n, dtype), dtype, 1) for _ in range(2)]
    if hostile:  # a hostile peer: NaN, smallest and largest scale bytes, magnitude 0x7F of both signs
        for s, first in zip(segs, (0, 3, 6)):
            s[first:first + 3] = 0xFF, 0, 254
            s[R.scale_bytes(n) + 32 * (first + 3) + np.arange(0, 64, 7)] = np.tile([0x7F, 0xFF], 5)
    dsegs = {id(s): torch.from_numpy(s).cuda() for s in segs}  # one array in several places is one buffer
    assert K.bagua_ring_apply_mxfp8(dtype, *[dsegs[id(s)].data_ptr() for s in segs], seg.size, n, *ptrs(ds), None) == OK
    for s in segs:
        same_bytes(host(dsegs[id(s)], U8), s, f"{what}: a segment after the apply")
    check4(ds, reference_apply(segs, w, l, r, dtype), full, dtype, f"{what}: after the apply")
    ds, full = guarded(arrs, dtype)
    assert K.bagua_ring_one_rank_mxfp8(dtype, *ptrs(ds), n, None) == OK, what
    check4(ds, one, full, dtype, f"{what}: one rank")


@pytest.mark.parametrize("dtype", DTYPES)
def test_entry_points_against_the_reference(bc, dtype, monkeypatch):
    w = WAVE_TILE[dtype]
    rng = np.random.default_rng(900 + dtype)
    for n, hostile in [(5, 0), (32, 0), (w, 0), (w - 32, 0), (w + 32, 0), (w + 17, 0), (w + 17, 1), (9 * w + 17, 0)]:
        for k in GRID_KNOBS:
            monkeypatch.setenv(k, "2") if n > 9 * w else monkeypatch.delenv(k, raising=False)
        assert bc._native.K.bagua_mxfp8_compressed_bytes(n, 1) == R.compressed_bytes(n, 1)
        check_entries(bc._native.K, dtype, [grads(rng, n, dtype) for _ in range(4)], f"dtype={dtype} n={n}", hostile)


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_table(bc, dtype):
    """t = the table, L = R = W = 0: every tie, scale byte and amax position through the mix and the
    apply, the one segment in all three places, and through the one-rank kernel"""
    t = B.table(dtype).x.copy()
    check_entries(bc._native.K, dtype, [t] + [np.zeros_like(t)] * 3, "boundary table", one_segment=True)


def check_op(bc, comms, entry, data, want, dtype, what, offset=0, num_elem=None):
    """the ring op on every rank's thread, on fresh device copies of data ({"t", "w", "l", "r"}: every
    rank's array), rank 0 placed `offset` elements into its allocation; all four tensors of every rank
    against `want` unless that is None; returns the kernel names of rank 0"""
    N, names, offs = bc._native, [], [offset] + [0] * 8
    dts = {k: [dev(np.concatenate([np.zeros(o, a.dtype), a]), dtype)[o:] for a, o in zip(data[k], offs)]
           for k in "twlr"}
    op = getattr(N.C, "bagua_decentralized_low_precision_" + entry)

    def rank(r):
        raws = [bc.BaguaTensorPy(dts[k][r], f"{k}{r}").raw() for k in "twlr"]
        for x in raws:
            x.num_elem = num_elem or x.num_elem
        args = (comms[r].handle, *[ctypes.byref(x) for x in raws], N.COMPRESSION_MXFP8)
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


def ring_case(cls, p, dtype, n=4099):
    """one input class of op_edge_cases and the reference's result"""
    data = E.build_ring(cls, p, n, dtype, E.case_rng("mxfp8 ring", cls, p, dtype))
    with np.errstate(all="ignore"):
        return data, R.decentralized(data["t"], data["w"], data["l"], data["r"], dtype)


def composed(names):  # the elementwise sequence and none of the three new kernels
    return "binary_kernel" in names and "mxfp8_decode_kernel" in names and not set(names) & set(FUSED + ONE_RANK)


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_on_hostile_inputs(bc, dtype):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(4, 0)
    for cls in E.RING_CLASSES:
        names = check_op(bc, comms, "synchronous", *ring_case(cls, 4, dtype), dtype, f"{cls} dtype={dtype}")
        assert cls != E.RING_CLASSES[0] or names == FUSED, names


@pytest.mark.parametrize("p", [1, 2, 3])
def test_every_dispatch_path(bc, p, monkeypatch):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    for dtype in (F32, BF16):
        case, off = ring_case("benign", p, dtype), 1 if dtype == F32 else 2  # 4 bytes: rank 0 runs on aligned copies
        kernels = ONE_RANK if p == 1 else FUSED
        assert check_op(bc, comms, "synchronous", *case, dtype, "synchronous") == kernels
        assert check_op(bc, comms, "pipelined", *case, dtype, "pipelined, 3 pieces") == kernels  # stays unpieced
        assert check_op(bc, comms, "synchronous", *case, dtype, "4-byte offset", offset=off) == kernels
        assert composed(check_op(bc, comms, "synchronous_unfused", *case, dtype, "unfused"))
        for env in ("BAGUA_MXFP8_RING_FUSED",) + (("BAGUA_ONE_RANK_FUSED",) if p == 1 else ()):
            monkeypatch.setenv(env, "0")  # the composed steps; at one rank mix + apply, `mine` in all three places
            names = check_op(bc, comms, "synchronous", *case, dtype, env + "=0")
            assert names == FUSED if env == "BAGUA_ONE_RANK_FUSED" else composed(names), names
            monkeypatch.delenv(env)
        # dispatch only: a partly valid tensor runs the composed steps (their bytes are the unfused entry's business)
        assert composed(check_op(bc, comms, "synchronous", case[0], None, dtype, "partly valid", num_elem=4099 - 5))


def test_refusals(bc):
    K, n = bc._native.K, 1000
    S = R.compressed_bytes(n, 1)
    hosts = [grads(np.random.default_rng(950), n + 8, F32) for _ in range(4)]
    ds = [dev(a, F32) for a in hosts]
    out = torch.full((S + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    (t, w, l, r), o = ptrs(ds), out.data_ptr()
    mix, app, one = K.bagua_ring_mix_mxfp8, K.bagua_ring_apply_mxfp8, K.bagua_ring_one_rank_mxfp8
    # a tensor that is not 16-B aligned, a dtype outside the three (U8 and beyond)
    for rc in (mix(F32, t + 4, l, r, w, n, o, S, None), mix(F32, t, l, r, w + 4, n, o, S, None),
               mix(3, t, l, r, w, n, o, S, None), app(F32, o, o, o, S, n, t, w, l + 4, r, None),
               app(7, o, o, o, S, n, t, w, l, r, None), one(F32, t, w, l, r + 4, n, None), one(5, t, w, l, r, n, None)):
        assert rc == UNSUPPORTED
    # a null pointer, n <= 0, a short buffer, a misaligned one
    for rc in (mix(F32, None, l, r, w, n, o, S, None), mix(F32, t, l, r, w, n, None, S, None),
               mix(F32, t, l, r, w, 0, o, S, None), mix(F32, t, l, r, w, -1, o, S, None),
               mix(F32, t, l, r, w, n, o, S - 1, None), mix(F32, t, l, r, w, n, o + 4, S, None),
               app(F32, o, None, o, S, n, t, w, l, r, None), app(F32, o, o, o, S, n, t, None, l, r, None),
               app(F32, o, o, o, S, 0, t, w, l, r, None), app(F32, o, o, o, S - 1, n, t, w, l, r, None),
               app(F32, o, o, o + 2, S, n, t, w, l, r, None), one(F32, t, w, None, r, n, None),
               one(F32, t, w, l, r, 0, None)):
        assert rc == INVALID_ARG
    for d, h in zip(ds + [out], hosts + [np.full(S + 16, 0xAB, np.uint8)]):  # nothing was launched
        same_bytes(host(d, F32), h, "a buffer after the refusals")
