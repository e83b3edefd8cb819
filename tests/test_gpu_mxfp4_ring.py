"""GPU tests of the decentralized ring op's fused MXFP4 kernels (csrc/kernels/mxfp4_ring.hip,
MXFP4.md "Ring op"): the three C entry points, the dispatch of decentralized() in
csrc/runtime/comm_ops.cpp and the bucket op, byte for byte against the composed op sequence
of the numpy reference (tests/mxfp4_reference.py).  Every byte of all four tensors and of
the segment is compared, the guard elements behind the tensors included.  Every test runs
with BAGUA_MXFP4_HWCVT=1 and =0.

Launch geometry of mxfp4_ring.hip, from which the sizes follow: a lane of the mix (and of
the one-rank kernel) owns one 16-B vector (4 f32 / 8 16-bit elements) of each of two blocks,
so a wave tile is 16 / 32 blocks = 512 / 1024 elements (WAVE_TILE) and a workgroup of four
waves covers 2048 / 4096.  A lane of the apply owns two vector positions per iteration and
its workgroup covers 2048 / 4096 elements as well.  BAGUA_TUNE_MX_RING_*_BLOCKS=2 caps a grid
at two workgroups, eight wave tiles: wave tile 8 is then the second grid-stride iteration of
the first wave, and 9 * WAVE_TILE + 17 ends in a ragged tile on the second."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp4_boundary_cases as B
import mxfp4_reference as R
import op_edge_cases as E
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_op_edges import KernelNames
from test_mxfp4_ring_cpu import grads, mixed_reference, same_bytes

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
WAVE_TILE = {F32: 512, F16: 1024, BF16: 1024}
GRID_KNOBS = ("BAGUA_TUNE_MX_RING_MIX_BLOCKS", "BAGUA_TUNE_MX_RING_APPLY_BLOCKS", "BAGUA_TUNE_MX_RING_ONE_RANK_BLOCKS")
GUARD = 40       # elements behind every tensor, never to be read or written
HUGE = 6e4       # their value: a segment built from them would hold another scale byte
FUSED = ["mxfp4_ring_mix_kernel", "mxfp4_ring_apply_kernel"]
ONE_RANK = ["mxfp4_ring_one_rank_kernel"]
ALL_FUSED = FUSED + ONE_RANK
ENTRIES = ("synchronous", "unfused", "pipelined")


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(params=["1", "0"], ids=["hwcvt", "arith"], autouse=True)
def hwcvt(request, monkeypatch):
    monkeypatch.setenv("BAGUA_MXFP4_HWCVT", request.param)
    return request.param


def sizes(dtype):
    """(n, two workgroups): less than a block; a block; a wave tile; one block less and more; a
    partial last block and a non-vector tail; the second grid-stride iteration of two workgroups"""
    w = WAVE_TILE[dtype]
    return [(5, False), (32, False), (w, False), (w - 32, False), (w + 32, False), (w + 17, False), (9 * w + 17, True)]


def guarded(x, dtype):
    """x followed by GUARD huge elements, on the device and as the host copy to compare against"""
    full = np.concatenate([x, NP.from_f32(np.full(GUARD, HUGE, np.float32), dtype)])
    return dev(full, dtype), full


def reference_apply(segs, w, l, r, dtype):
    """decompress / add with three segments (mine, from_left, from_right): t, w, l, r"""
    n = w.size
    with np.errstate(all="ignore"):
        t = R.decompress(segs[1], 1, np.zeros(n, R.STORAGE[dtype]), dtype)
        l = NP.add_inplace(l.copy(), t, dtype)
        t = R.decompress(segs[2], 1, t, dtype)
        r = NP.add_inplace(r.copy(), t, dtype)
        t = R.decompress(segs[0], 1, t, dtype)
        t = NP.add_inplace(t, w, dtype)
    return t, t.copy(), l, r


def u8(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------ 1. kernel ABI ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_entry_points_against_the_reference(bc, dtype, monkeypatch):
    K = bc._native.K
    rng = np.random.default_rng(700 + dtype)
    for n, two in sizes(dtype):
        what = f"dtype={dtype} n={n}"
        for k in GRID_KNOBS:
            monkeypatch.setenv(k, "2") if two else monkeypatch.delenv(k, raising=False)
        t, w, l, r = (grads(rng, n, dtype) for _ in range(4))
        S = R.compressed_bytes(n, 1)
        assert K.bagua_mxfp4_compressed_bytes(n, 1) == S
        # the mix: addmul x 3 + compress; t and the bytes behind the segment untouched
        (dt, ht), (dw, hw), (dl, hl), (dr, hr) = (guarded(a, dtype) for a in (t, w, l, r))
        out = torch.full((S + 32,), 0xAB, dtype=torch.uint8, device="cuda")
        assert K.bagua_ring_mix_mxfp4(dtype, dt.data_ptr(), dl.data_ptr(), dr.data_ptr(), dw.data_ptr(), n,
                                      out.data_ptr(), S, None) == OK, what
        seg = R.compress(mixed_reference(t, w, l, r, dtype), dtype, 1)
        same_bytes(u8(out), np.concatenate([seg, np.full(32, 0xAB, np.uint8)]), f"{what}: segment")
        for name, d, h in (("t", dt, ht), ("weight", dw, hw), ("left", dl, hl), ("right", dr, hr)):
            same_bytes(host(d, dtype), h, f"{what}: {name} after the mix")
        # the apply on three different segments
        segs = [seg] + [R.compress(grads(rng, n, dtype), dtype, 1) for _ in range(2)]
        ds = [torch.from_numpy(s).cuda() for s in segs]
        assert K.bagua_ring_apply_mxfp4(dtype, ds[0].data_ptr(), ds[1].data_ptr(), ds[2].data_ptr(), S, n,
                                        dt.data_ptr(), dw.data_ptr(), dl.data_ptr(), dr.data_ptr(), None) == OK, what
        want = reference_apply(segs, w, l, r, dtype)
        for name, d, h, wk in zip(("t", "weight", "left", "right"), (dt, dw, dl, dr), (ht, hw, hl, hr), want):
            same_bytes(host(d, dtype), np.concatenate([wk, h[n:]]), f"{what}: {name} after the apply")
        for s, d in zip(segs, ds):
            same_bytes(u8(d), s, f"{what}: a segment after the apply")
        # the one-rank kernel: the p = 1 op
        (dt, ht), (dw, hw), (dl, hl), (dr, hr) = (guarded(a, dtype) for a in (t, w, l, r))
        assert K.bagua_ring_one_rank_mxfp4(dtype, dt.data_ptr(), dw.data_ptr(), dl.data_ptr(), dr.data_ptr(), n,
                                           None) == OK, what
        want = R.decentralized([t], [w], [l], [r], dtype)
        for name, d, h, wk in zip(("t", "weight", "left", "right"), (dt, dw, dl, dr), (ht, hw, hl, hr), want):
            same_bytes(host(d, dtype), np.concatenate([wk[0], h[n:]]), f"{what}: {name} after the one-rank kernel")


# -------------------------------------------------------- 2. boundary table ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_table(bc, dtype):
    """t = the table, L = R = W = 0: the mix hands the table on (tests/test_mxfp4_ring_cpu.py asserts
    that on the reference), so every tie, scale byte and amax position goes through both paths"""
    K = bc._native.K
    t = B.table(dtype).x.copy()
    n = t.size
    zero = np.zeros_like(t)
    want = R.decentralized([t], [zero], [zero], [zero], dtype)
    S = R.compressed_bytes(n, 1)
    ds = [dev(a, dtype) for a in (t, zero, zero, zero)]
    out = torch.full((S,), 0xAB, dtype=torch.uint8, device="cuda")
    assert K.bagua_ring_mix_mxfp4(dtype, ds[0].data_ptr(), ds[2].data_ptr(), ds[3].data_ptr(), ds[1].data_ptr(), n,
                                  out.data_ptr(), S, None) == OK
    same_bytes(u8(out), R.compress(t, dtype, 1), "segment")
    assert K.bagua_ring_apply_mxfp4(dtype, out.data_ptr(), out.data_ptr(), out.data_ptr(), S, n,
                                    *[d.data_ptr() for d in ds], None) == OK
    for name, d, wk in zip(("t", "weight", "left", "right"), ds, want):
        same_bytes(host(d, dtype), wk[0], f"mix + apply: {name}")
    ds = [dev(a, dtype) for a in (t, zero, zero, zero)]
    assert K.bagua_ring_one_rank_mxfp4(dtype, *[d.data_ptr() for d in ds], n, None) == OK
    for name, d, wk in zip(("t", "weight", "left", "right"), ds, want):
        same_bytes(host(d, dtype), wk[0], f"one rank: {name}")


# ------------------------------------------------------------------ the op ----
def run_op(bc, comms, entry, tensors, pieces=3, num_elem=None):
    """the ring op on every rank's thread; tensors[k][r] for k in "twlr".  Returns the names of the
    kernels launched on rank 0's thread."""
    N = bc._native
    C = N.C
    names = []

    def rank(r):
        raws = [bc.BaguaTensorPy(tensors[k][r], f"{k}{r}").raw() for k in "twlr"]
        if num_elem is not None:  # the elementwise steps want the four tensors alike
            for x in raws:
                x.num_elem = num_elem
        refs = [ctypes.byref(x) for x in raws]
        h = comms[r].handle

        def call():
            if entry == "synchronous":
                return C.bagua_decentralized_low_precision_synchronous(h, *refs, N.COMPRESSION_MXFP4)
            if entry == "unfused":
                return C.bagua_decentralized_low_precision_synchronous_unfused(h, *refs, N.COMPRESSION_MXFP4)
            return C.bagua_decentralized_low_precision_pipelined(h, *refs, N.COMPRESSION_MXFP4, pieces)

        if r == 0:
            with KernelNames(N, comms[0]) as k:
                rc = call()
            names.extend(k.names)
        else:
            rc = call()
        N.check(rc, f"{entry} rank {r}")

    torch.cuda.synchronize()
    run_ranks(rank, len(comms))
    return names


def check_op(bc, comms, entry, data, dtype, what, want=None, offsets=None, **kw):
    """runs the op on fresh device copies of data ({"t", "w", "l", "r"}: every rank's array) and compares
    all four tensors of every rank with the reference; returns the kernel names of rank 0"""
    p = len(comms)
    if want is None:
        with np.errstate(all="ignore"):
            want = R.decentralized(data["t"], data["w"], data["l"], data["r"], dtype)
    offsets = offsets or [0] * p

    def place(a, off):
        return dev(np.concatenate([np.zeros(off, a.dtype), a]), dtype)[off:]

    dts = {k: [place(a, off) for a, off in zip(data[k], offsets)] for k in "twlr"}
    names = run_op(bc, comms, entry, dts, **kw)
    for k, wk in zip("twlr", want):
        for r in range(p):
            same_bytes(host(dts[k][r], dtype), wk[r], f"{what}: {k} rank {r}")
    return names


def ring_data(rng, p, n, dtype):
    return {k: [grads(rng, n, dtype) for _ in range(p)] for k in "twlr"}


# ---------------------------------------------------- 3. hostile inputs ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_on_hostile_inputs(bc, dtype):
    from bagua_core.communicator import loopback_communicators
    p, n = 4, 4099
    comms = loopback_communicators(p, 0)
    for cls in E.RING_CLASSES:
        data = E.build_ring(cls, p, n, dtype, E.case_rng("mxfp4 ring", dtype, cls))
        names = check_op(bc, comms, "synchronous", data, dtype, f"{cls} dtype={dtype}")
        if cls == E.RING_CLASSES[0]:  # the path really is the path: no binary_kernel, no mxfp4_decode_kernel
            assert names == FUSED, names


# ------------------------------------------------ 4. every dispatch path ----
@pytest.mark.parametrize("p", [2, 3])
def test_every_entry_gives_the_same_bytes(bc, p, monkeypatch):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    n = 4099
    for dtype in (F32, BF16):
        data = ring_data(np.random.default_rng(810 + 10 * p + dtype), p, n, dtype)
        with np.errstate(all="ignore"):
            want = R.decentralized(data["t"], data["w"], data["l"], data["r"], dtype)
        assert check_op(bc, comms, "synchronous", data, dtype, "synchronous", want) == FUSED
        # the pipelined entry stays unpieced for this codec: one mix, one apply
        assert check_op(bc, comms, "pipelined", data, dtype, "pipelined, 3 pieces", want, pieces=3) == FUSED
        names = check_op(bc, comms, "unfused", data, dtype, "unfused", want)
        assert "binary_kernel" in names and "mxfp4_decode_kernel" in names and not set(names) & set(ALL_FUSED), names
        monkeypatch.setenv("BAGUA_MXFP4_RING_FUSED", "0")
        names = check_op(bc, comms, "synchronous", data, dtype, "BAGUA_MXFP4_RING_FUSED=0", want)
        assert "binary_kernel" in names and "mxfp4_decode_kernel" in names and not set(names) & set(ALL_FUSED), names
        monkeypatch.delenv("BAGUA_MXFP4_RING_FUSED")


def test_one_rank(bc, monkeypatch):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(1, 0)
    for dtype in DTYPES:
        data = ring_data(np.random.default_rng(820 + dtype), 1, 4099, dtype)
        assert check_op(bc, comms, "synchronous", data, dtype, "one rank") == ONE_RANK
        monkeypatch.setenv("BAGUA_ONE_RANK_FUSED", "0")  # mix + apply with `mine` in all three places
        assert check_op(bc, comms, "synchronous", data, dtype, "one rank, two kernels") == FUSED
        monkeypatch.delenv("BAGUA_ONE_RANK_FUSED")


def test_a_rank_at_a_4_byte_offset(bc):
    """rank 0's tensors are not 16-B aligned: it runs the fused kernels on aligned copies"""
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(2, 0)
    data = ring_data(np.random.default_rng(830), 2, 4099, F32)
    assert check_op(bc, comms, "synchronous", data, F32, "offset", offsets=[1, 0]) == FUSED
    one = loopback_communicators(1, 0)
    data = ring_data(np.random.default_rng(831), 1, 4099, F32)
    assert check_op(bc, one, "synchronous", data, F32, "offset, one rank", offsets=[1]) == ONE_RANK


def test_a_partially_valid_tensor_runs_the_composed_steps(bc):
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(2, 0)
    n = 4099
    data = ring_data(np.random.default_rng(840), 2, n, F32)
    dts = {k: [dev(a, F32) for a in data[k]] for k in "twlr"}
    names = run_op(bc, comms, "synchronous", dts, num_elem=n - 5)
    assert "binary_kernel" in names and not set(names) & set(ALL_FUSED), names
    # the same bytes as the entry that never fuses
    ref = {k: [dev(a, F32) for a in data[k]] for k in "twlr"}
    run_op(bc, comms, "unfused", ref, num_elem=n - 5)
    for k in "twlr":
        for r in range(2):
            same_bytes(host(dts[k][r], F32), host(ref[k][r], F32), f"{k} rank {r}")


# ---------------------------------------------------------- 5. refusals ----
def test_refusals(bc):
    K = bc._native.K
    n = 1000
    S = R.compressed_bytes(n, 1)
    rng = np.random.default_rng(850)
    hosts = [grads(rng, n + 8, F32) for _ in range(4)]
    t, w, l, r = (dev(a, F32) for a in hosts)
    out = torch.full((S + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    tp, wp, lp, rp, op = t.data_ptr(), w.data_ptr(), l.data_ptr(), r.data_ptr(), out.data_ptr()
    mix = K.bagua_ring_mix_mxfp4
    assert mix(F32, tp + 4, lp, rp, wp, n, op, S, None) == UNSUPPORTED        # a tensor that is not 16-B aligned
    assert mix(F32, tp, lp, rp, wp + 4, n, op, S, None) == UNSUPPORTED
    assert mix(3, tp, lp, rp, wp, n, op, S, None) == UNSUPPORTED              # U8 is no codec dtype
    assert mix(F32, None, lp, rp, wp, n, op, S, None) == INVALID_ARG
    assert mix(F32, tp, lp, rp, wp, n, None, S, None) == INVALID_ARG
    assert mix(F32, tp, lp, rp, wp, 0, op, S, None) == INVALID_ARG
    assert mix(F32, tp, lp, rp, wp, -1, op, S, None) == INVALID_ARG
    assert mix(F32, tp, lp, rp, wp, n, op, S - 1, None) == INVALID_ARG        # short output
    assert mix(F32, tp, lp, rp, wp, n, op + 4, S, None) == INVALID_ARG        # misaligned output
    apply = K.bagua_ring_apply_mxfp4
    assert apply(F32, op, op, op, S, n, tp, wp, lp + 4, rp, None) == UNSUPPORTED
    assert apply(7, op, op, op, S, n, tp, wp, lp, rp, None) == UNSUPPORTED
    assert apply(F32, op, None, op, S, n, tp, wp, lp, rp, None) == INVALID_ARG
    assert apply(F32, op, op, op, S, n, tp, None, lp, rp, None) == INVALID_ARG
    assert apply(F32, op, op, op, S, 0, tp, wp, lp, rp, None) == INVALID_ARG
    assert apply(F32, op, op, op, S - 1, n, tp, wp, lp, rp, None) == INVALID_ARG
    assert apply(F32, op, op, op + 2, S, n, tp, wp, lp, rp, None) == INVALID_ARG   # misaligned segment
    one = K.bagua_ring_one_rank_mxfp4
    assert one(F32, tp, wp, lp, rp + 4, n, None) == UNSUPPORTED
    assert one(5, tp, wp, lp, rp, n, None) == UNSUPPORTED
    assert one(F32, tp, wp, None, rp, n, None) == INVALID_ARG
    assert one(F32, tp, wp, lp, rp, 0, None) == INVALID_ARG
    # nothing was launched: every buffer is as it was
    for name, d, h in zip(("t", "weight", "left", "right"), (t, w, l, r), hosts):
        same_bytes(host(d, F32), h, name)
    assert (u8(out) == 0xAB).all()


# ------------------------------------------- 6. the bucket op, the backend ----
def test_bucket_op_through_the_backend(bc):
    from bagua_core.communicator import loopback_communicators
    comm = loopback_communicators(1, 0)[0]
    n = 3 * 5000 + 7
    rng = np.random.default_rng(860)
    arrs = [grads(rng, n, F32) for _ in range(4)]  # t, w, l, r
    want = R.decentralized(*[[a] for a in arrs], F32)
    ts = [dev(a, F32) for a in arrs]
    bt = [bc.BaguaTensorPy(x, nm) for x, nm in zip(ts, "twlr")]
    bk = bc.BaguaBucketPy("mxfp4_ring", [bt[0]])
    bk.append_low_precision_decentralized_synchronous_op(comm, None, hierarchical=False, peer_selection_mode="ring",
                                                          compression="MXFP4", weight=bt[1], left_peer_weight=bt[2],
                                                          right_peer_weight=bt[3])
    backend = bc.BaguaCommBackendPy(4, 0)
    backend.register_ordered_buckets([bk])
    ev = torch.cuda.Event()
    ev.record()
    backend.mark_communication_ready(bt[0], ev.cuda_event)
    assert backend.wait_pending_comm_ops() == 1
    for name, d, wk in zip(("t", "weight", "left", "right"), ts, want):
        same_bytes(host(d, F32), wk[0], name)
