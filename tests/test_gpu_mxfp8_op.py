"""GPU tests of the comm ops with the MXFP8 codec (MXFP8.md, "Surfaces"): the centralized op on
the in-process loopback transport against the numpy reference's composition
(tests/mxfp8_reference.py), unpieced and pipelined, every piece count giving the unpieced
op's bytes; hostile gradients (tests/op_edge_cases.py); the decentralized ring op by name; the
bucket op through the backend; the refusals; the schedule check; and one run over real RCCL
between two processes (tests/mxfp8_rccl_worker.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mxfp8_reference as R
import op_edge_cases as E
from test_gpu_codec import assert_float_bits_equal
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_mxfp8 import BF16, DTYPES, F16, F32, dev_at, grads, run_centralized, same_bytes
from test_gpu_schedule_check import _run_each

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mxfp8_rccl_worker.py")
TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
ERR_INVALID_ARG = 1
SCHEDULE_ENV = ("BAGUA_PIPELINE_TAPER", "BAGUA_PIPELINE_PIECES", "BAGUA_PIPELINE_MIN_PIECE", "BAGUA_CHECK_SCHEDULE")
KERNELS = ("mxfp8_encode_kernel", "mxfp8_reduce_encode_kernel", "mxfp8_decode_kernel")
CS = 4 * 4096 + 77   # four granule boundaries, a ragged last tile and block; chunks past the first are unaligned,
#                      so the op runs unpieced whatever is asked for (a chunk must be whole 16-B vectors)
CS_VEC = 4 * 4096 + 80   # the same with whole vectors for every dtype: the op runs pieced


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(autouse=True)
def default_schedule_env(monkeypatch):
    for k in SCHEDULE_ENV:
        monkeypatch.delenv(k, raising=False)


def pipelined(bc, pieces):
    op = bc._native.C.bagua_centralized_low_precision_pipelined
    return lambda comm, raw, average, method: op(comm, raw, average, method, pieces)


def filled_pieces(cs, schedule):
    return sum(e > b for b, e in (R.piece_range(cs, schedule, q) for q in range(schedule & 0xFFFF)))


def counts(names):
    return [names.count(k) for k in KERNELS]


def run_op(bc, comms, xs, dtype, average, pieces, timed=False, offsets=None):
    ts = [dev_at(x, dtype, offsets[r] if offsets else 0) for r, x in enumerate(xs)]
    names = run_centralized(bc, comms, pipelined(bc, pieces), ts, average, timed=timed)
    return [host(t, dtype).copy() for t in ts], names


@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 17])
def test_centralized_op_every_piece_count(bc, p, average):
    """n = p * (4 * 4096 + 77) and p * (4 * 4096 + 80): unpieced, 4 pieces and 8 | TAPERED against the
    reference's composition and against each other; the path from the kernel names of rank 0"""
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(500 + 10 * p + average)
    for cs, dtype in ((CS, F32), (CS_VEC, F32)) + (((CS_VEC, BF16),) if p in (2, 3) else ()):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        want = R.centralized(xs, dtype, bool(average))
        one = None
        for pieces in (1, 4, 8 | TAPERED):
            got, names = run_op(bc, comms, xs, dtype, average, pieces, timed=True)
            what = f"p={p} cs={cs} dtype={dtype} average={average} pieces={pieces:#x}"
            for r in range(p):
                same_bytes(got[r], want[r], f"{what} rank {r} against the reference")
                if one is not None:
                    same_bytes(got[r], one[r], f"{what} rank {r} against the unpieced op")
            one = one or got
            if p == 17:    # more than the fused middle step takes: the composed steps, unpieced
                assert counts(names) == [2, 0, 2] and "reduce_chunks_kernel" in names, names
            elif p == 1 or pieces == 1 or cs == CS:
                assert counts(names) == [1, 1, 1] and "reduce_chunks_kernel" not in names, names
            else:
                k = filled_pieces(cs, pieces)
                assert k > 1 and counts(names) == [k, k, k] and "reduce_chunks_kernel" not in names, names


def test_one_rank_not_16_byte_aligned(bc):
    """one rank's tensor starts one element into its allocation: it runs the same pieced schedule on
    an aligned copy, every rank posts the same exchanges"""
    from bagua_core.communicator import loopback_communicators
    p = 3
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(808)
    cs = CS_VEC
    for dtype in (F32, F16):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        got, names = run_op(bc, comms, xs, dtype, 1, 4, timed=True, offsets=[0, 1, 0])
        k = filled_pieces(cs, 4)
        assert k > 1 and counts(names) == [k, k, k], names
        want = R.centralized(xs, dtype, True)
        for r in range(p):
            same_bytes(got[r], want[r], f"dtype={dtype} rank {r}")


@pytest.mark.parametrize("cls", ["one_nan", "all_nan_chunk", "pos_inf", "neg_inf", "inf_cancel", "constant", "zero",
                                 "neg_zero", "denormal", "huge"])
def test_hostile_gradients(bc, cls):
    from bagua_core.communicator import loopback_communicators
    p, cs = 4, 2 * 4096 + 40
    comms = loopback_communicators(p, 0)
    for dtype in DTYPES:
        xs = E.build(cls, p, cs, dtype, E.case_rng("mxfp8", cls, dtype))
        with np.errstate(over="ignore", invalid="ignore"):
            want = R.centralized(xs, dtype, True)
        for pieces in (1, 3):
            got, _ = run_op(bc, comms, xs, dtype, 1, pieces)
            for r in range(p):
                assert_float_bits_equal(got[r], want[r], dtype, f"{cls} dtype={dtype} pieces={pieces} rank {r}")


@pytest.mark.parametrize("p", [1, 2, 3])
def test_ring_op_by_name(bc, p):
    """the decentralized op takes the method through its elementwise sequence"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    comms = loopback_communicators(p, 0)
    n = 3000 + 17
    for dt in (F32, F16):
        rng = np.random.default_rng(60 + p + dt)
        data = [[grads(rng, n, dt) for _ in range(p)] for _ in range(4)]  # t, weight, left, right
        devs = [[dev(a, dt) for a in group] for group in data]
        buckets = []
        for r in range(p):
            names = ("g", "w", "l", "r")
            ts = [bc.BaguaTensorPy(devs[k][r], f"{names[k]}{r}") for k in range(4)]
            bk = bc.BaguaBucketPy(f"ring{r}", [ts[0]])
            bk.append_low_precision_decentralized_synchronous_op(comms[r], None, hierarchical=False,
                                                                 peer_selection_mode="ring", compression="MXFP8",
                                                                 weight=ts[1], left_peer_weight=ts[2],
                                                                 right_peer_weight=ts[3])
            assert len(bk.ops()) == 1
            buckets.append(bk)

        def rank(r):
            raws = [bc.BaguaTensorPy(devs[k][r], f"r{r}.{k}").raw() for k in range(4)]
            N.check(N.C.bagua_decentralized_low_precision_synchronous(
                comms[r].handle, *[ctypes.byref(x) for x in raws], N.COMPRESSION_MXFP8), f"rank {r}")

        torch.cuda.synchronize()
        run_ranks(rank, p)
        want = R.decentralized(*data, dt)
        for k, name in enumerate(("t", "weight", "left", "right")):
            for r in range(p):
                same_bytes(host(devs[k][r], dt), want[k][r], f"p={p} dtype={dt} {name} rank {r}")


def test_bucket_op_and_refusals(bc):
    from bagua_core.communicator import loopback_communicators
    comm = loopback_communicators(1, 0)[0]
    n = 3 * 5000 + 7
    rng = np.random.default_rng(3)
    x = grads(rng, n, F32)
    t = torch.zeros(n, device="cuda")
    bt = bc.BaguaTensorPy(t, "g")
    bk = bc.BaguaBucketPy("mxfp8_bucket", [bt])
    bk.append_centralized_synchronous_op(comm, None, hierarchical=False, average=True, compression="MXFP8")
    backend = bc.BaguaCommBackendPy(4, 0)
    backend.register_ordered_buckets([bk])
    t.copy_(torch.from_numpy(x))
    ev = torch.cuda.Event()
    ev.record()
    backend.mark_communication_ready(bt, ev.cuda_event)
    assert backend.wait_pending_comm_ops() == 1
    same_bytes(host(t, F32), R.centralized([x], F32, True)[0], "bucket op")
    # error feedback and stochastic rounding do not exist for this codec
    with pytest.raises(NotImplementedError):
        bk.append_centralized_synchronous_op(comm, None, compression="MXFP8",
                                             error_feedback=bc.MXFP4ErrorFeedbackState(n, 1, 0))
    with pytest.raises(NotImplementedError):
        bk.append_centralized_synchronous_op(comm, None, compression="MXFP8",
                                             stochastic_rounding=bc.MXFP4StochasticRounding(7))
    assert len(bk.ops()) == 1


def test_schedule_check(bc, monkeypatch):
    """BAGUA_CHECK_SCHEDULE=1 at p = 2: ranks that ask for different piece counts, or for different
    block codecs, all fail before anything is posted; matching ranks pass"""
    monkeypatch.setenv("BAGUA_CHECK_SCHEDULE", "1")
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    p, cs = 2, 5 * 4096
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(17)
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    ts = [dev(x, F32) for x in xs]
    torch.cuda.synchronize()
    raws = [bc.BaguaTensorPy(t, "g").raw() for t in ts]
    op = N.C.bagua_centralized_low_precision_pipelined
    for mine in ((4, 2), (3, 1), (3, 3 | TAPERED)):
        rcs = _run_each(p, lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP8, mine[r]))
        assert rcs == [ERR_INVALID_ARG] * p, (mine, rcs)
    methods = (N.COMPRESSION_MXFP8, N.COMPRESSION_MXFP4)
    rcs = _run_each(p, lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, methods[r], 3))
    assert rcs == [ERR_INVALID_ARG] * p, rcs
    for r in range(p):
        same_bytes(host(ts[r], F32), xs[r], f"rank {r} must be untouched")
    rcs = _run_each(p, lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP8, 3))
    assert rcs == [0] * p, rcs
    want = R.centralized(xs, F32, True)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"matching ranks, rank {r}")


def test_pipelined_op_over_rccl(tmp_path):
    """two processes, each its own RCCL communicator on the one GPU (set up as
    tests/test_gpu_mxfp4_pipelined_rccl.py): 3 pieces, then the automatic count, which
    BAGUA_PIPELINE_MIN_PIECE=4096 makes pieced too (a chunk's segment is 21120 bytes)"""
    world, cs = 2, 5 * 4096
    rng = np.random.default_rng(1300)
    mag = np.repeat(10.0 ** rng.uniform(-3, 2, world * cs // 32), 32)
    xs = [(rng.standard_normal(world * cs) * mag * 1e-3).astype(np.float32) for _ in range(world)]
    want = R.centralized(xs, F32, True)
    np.savez(tmp_path / "inputs.npz", **{f"x{r}": x for r, x in enumerate(xs)})
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"NCCL_HOSTID": f"bagua-test-rank-{r}", "NCCL_SOCKET_IFNAME": "lo", "NCCL_IB_DISABLE": "1",
                    "HSA_ENABLE_IPC_MODE_LEGACY": "0", "BAGUA_PIPELINE_MIN_PIECE": "4096"})
        log = open(tmp_path / f"rank{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, "-u", WORKER, str(r), str(world), str(tmp_path), "3,0"],
                                       stdout=log, stderr=subprocess.STDOUT, env=env, cwd=ROOT), log))
    failed = []
    for r, (p, log) in enumerate(procs):
        try:
            rc = p.wait(timeout=90)
        except subprocess.TimeoutExpired:
            for q, _ in procs:
                q.kill()
            rc = "timeout"
        log.close()
        if rc != 0:
            failed.append(r)
    if failed:
        tails = "\n".join(f"--- rank {r}:\n" + (tmp_path / f"rank{r}.log").read_text()[-1500:] for r in failed)
        pytest.fail(f"ranks {failed} failed:\n{tails}")
    for r in range(world):
        with np.load(tmp_path / f"out{r}.npz", allow_pickle=False) as z:
            for i, pieces in enumerate((3, 0)):
                assert np.array_equal(z[f"t{i}"], want[r].view(np.uint8)), f"rank {r}, pieces={pieces}"
