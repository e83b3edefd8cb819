"""GPU tests of the comm ops with the MXFP6 codec (MXFP6.md, "Surfaces"): what
csrc/runtime/comm_ops.cpp composes from the kernels that tests/test_gpu_mxfp6.py, _ring.py and
_ef.py pin one at a time.  Every dispatch path of the `kMxfp6` and `kMxfp6Ef` table entries on the
in-process loopback transport, bit for bit against the numpy references -- mxfp8_reference's composed
op over this codec's compress and decompress (the `composed` fixture) and
mxfp6_ef_reference.centralized_step, both checked on these inputs in tests/test_mxfp6_op_cpu.py --
with the path read from rank 0's kernel names: the synchronous and unfused entries, sum mode, the
composed middle steps past 16 ranks and on a partly valid tensor, every piece count, every payload
slack under the pieced exchange, a misaligned rank, hostile gradients (tests/op_edge_cases.py), the
hierarchical op, the bucket op through the backend, the schedule check with this codec's own op
kinds, the error-feedback op's fused and composed middle steps, and one run over real RCCL between
two processes (tests/mxfp6_rccl_worker.py).

A granule of the piece table is 128 blocks = 4096 elements; 1, 2, 3 and 4 blocks hold 24, 48, 72 and
96 payload bytes, so nb mod 4 = 1, 2, 3, 0 leaves 8, 16, 24 and 0 bytes of slack in the 32-B line."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mxfp6_ef_reference as REF
import mxfp6_reference as R
import op_edge_cases as E
from oracle import oracle_np as NP
from test_gpu_codec import assert_float_bits_equal
from test_gpu_multirank import dev, host, run_ranks
from test_gpu_mxfp6 import composed  # noqa: F401  (the fixture)
from test_gpu_mxfp8 import BF16, DTYPES, F16, F32, bc, dev_at, grads, run_centralized, same_bytes  # noqa: F401
from test_gpu_mxfp8_ef import step_grads
from test_gpu_mxfp8_op import default_schedule_env  # noqa: F401  (autouse: no schedule knob inherited)
from test_gpu_op_edges import KernelNames
from test_gpu_schedule_check import _run_each

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mxfp6_rccl_worker.py")
TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
ERR_INVALID_ARG = 1
KERNELS = ("mxfp6_encode_kernel", "mxfp6_reduce_encode_kernel", "mxfp6_decode_kernel")
EF_FUSED = ["mxfp6_encode_ef_kernel", "mxfp6_reduce_encode_ef_kernel", "mxfp6_decode_kernel"]
CS = 4 * 4096 + 77       # chunks past the first are not whole 16-B vectors: the op runs unpieced whatever is asked for
CS_VEC = 4 * 4096 + 80   # whole vectors for every dtype and a ragged last block: the op runs pieced


def mx6(N, entry):
    """the entry with this codec, in run_centralized's calling convention (which passes MXFP8's method)"""
    return lambda comm, raw, average, _method: entry(comm, raw, average, N.COMPRESSION_MXFP6)


def pipelined(N, pieces):
    op = N.C.bagua_centralized_low_precision_pipelined
    return lambda comm, raw, average, _method: op(comm, raw, average, N.COMPRESSION_MXFP6, pieces)


def filled_pieces(cs, schedule):
    return sum(e > b for b, e in (R.piece_range(cs, schedule, q) for q in range(schedule & 0xFFFF)))


def counts(names):
    return [names.count(k) for k in KERNELS]


def run_op(bc, comms, xs, dtype, average, pieces, timed=False, offsets=None):
    ts = [dev_at(x, dtype, offsets[r] if offsets else 0) for r, x in enumerate(xs)]
    names = run_centralized(bc, comms, pipelined(bc._native, pieces), ts, average, timed=timed)
    return [host(t, dtype).copy() for t in ts], names


# ------------------------------------------------ synchronous and unfused entries ----
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 17])
def test_synchronous_entries(bc, composed, p, fused):
    """cs = 1000, f32 and bf16, average and sum: the fused middle step up to 16 ranks, the composed steps
    (decompress + reduce_chunks_kernel + compress of the own chunk) past them, from the unfused entry and on
    a partly valid tensor"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    fn = mx6(N, N.C.bagua_centralized_low_precision_synchronous if fused
             else N.C.bagua_centralized_low_precision_synchronous_unfused)
    comms = loopback_communicators(p, 0)
    cs = 1000
    rng = np.random.default_rng(640 + p)
    first = True
    for dt in (F32, BF16):
        for average in (1, 0):
            xs = [grads(rng, p * cs, dt) for _ in range(p)]
            ts = [dev(x, dt) for x in xs]
            names = run_centralized(bc, comms, fn, ts, average, timed=first)
            if first:
                assert "mxfp6_encode_kernel" in names and "mxfp6_decode_kernel" in names, names
                if fused and p <= 16:
                    assert "mxfp6_reduce_encode_kernel" in names and "reduce_chunks_kernel" not in names, names
                else:
                    assert "reduce_chunks_kernel" in names and "mxfp6_reduce_encode_kernel" not in names, names
                first = False
            want = composed.centralized(xs, dt, bool(average))
            for r in range(p):
                same_bytes(host(ts[r], dt), want[r], f"p={p} dtype={dt} average={average} rank {r}")
    num_elem = p * cs - cs // 2 - 3
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    for x in xs:
        x[num_elem:] = 3e38
    ts = [dev(x, F32) for x in xs]
    names = run_centralized(bc, comms, fn, ts, 1, num_elem=num_elem, timed=True)
    assert "mxfp6_reduce_encode_kernel" not in names and "reduce_chunks_kernel" in names, names
    want = composed.centralized(xs, F32, True, num_elem=num_elem)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"p={p} partly valid rank {r}")


# ------------------------------------------------------------ the pieced schedule ----
@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 16, 17])
def test_every_piece_count(bc, composed, p, average):
    """n = p * (4 * 4096 + 77) and p * (4 * 4096 + 80): unpieced, 4 pieces and 8 | TAPERED (empty pieces on a
    chunk of four granules) against the reference and against each other; the path from rank 0's kernel names"""
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(600 + 10 * p + average)
    for cs, dtype in ((CS, F32), (CS_VEC, F32)) + (((CS_VEC, BF16),) if p in (2, 3) else ()):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        want = composed.centralized(xs, dtype, bool(average))
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
    assert filled_pieces(CS_VEC, 8 | TAPERED) < 8  # the tapered schedule leaves empty pieces here


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("d", [32, 64, 96, 128, 40])
def test_every_payload_slack_pieced(bc, composed, p, d):
    """cs = 4 * 4096 + d: nb mod 4 = 1, 2, 3, 0, and a ragged block of 8 elements at nb mod 4 = 2, in three
    pieces, the last one block or few.  One op on all-NaN tensors goes first on the same communicators: the
    pooled send and recv buffers the next op gets then hold 0xFF scale bytes wherever it does not write or
    exchange a range"""
    from bagua_core.communicator import loopback_communicators
    comms = loopback_communicators(p, 0)
    cs = 4 * 4096 + d
    assert filled_pieces(cs, 3) == 3 and R.piece_range(cs, 3, 2)[0] == 512
    rng = np.random.default_rng(900 + 10 * d + p)
    for dtype in (F32, F16):
        nan = [NP.from_f32(np.full(p * cs, np.nan, np.float32), dtype) for _ in range(p)]
        poisoned, _ = run_op(bc, comms, nan, dtype, 1, 1)
        assert all(E.is_nan(t, dtype).all() for t in poisoned)
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        got, names = run_op(bc, comms, xs, dtype, 1, 3, timed=True)
        assert counts(names) == [3, 3, 3], names
        want = composed.centralized(xs, dtype, True)
        for r in range(p):
            same_bytes(got[r], want[r], f"p={p} cs={cs} dtype={dtype} rank {r}")


def test_one_rank_not_16_byte_aligned(bc, composed):
    """one rank's tensor starts one element into its allocation: it runs the same pieced schedule on an
    aligned copy, every rank posts the same exchanges"""
    from bagua_core.communicator import loopback_communicators
    p, cs = 3, CS_VEC
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(868)
    for dtype in (F32, F16):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        got, names = run_op(bc, comms, xs, dtype, 1, 4, timed=True, offsets=[0, 1, 0])
        k = filled_pieces(cs, 4)
        assert k > 1 and counts(names) == [k, k, k], names
        want = composed.centralized(xs, dtype, True)
        for r in range(p):
            same_bytes(got[r], want[r], f"dtype={dtype} rank {r}")


@pytest.mark.parametrize("cls", E.CLASSES)
def test_hostile_gradients(bc, composed, cls):
    """p = 4, cs = 2 * 4096 + 40, unpieced and in three pieces; sum mode for the short list of classes"""
    from bagua_core.communicator import loopback_communicators
    p, cs = 4, 2 * 4096 + 40
    comms = loopback_communicators(p, 0)
    for dtype in DTYPES:
        xs = E.build(cls, p, cs, dtype, E.case_rng("mxfp6", cls, dtype))
        for average in (1, 0) if cls in E.SHORT_CLASSES else (1,):
            with np.errstate(over="ignore", invalid="ignore"):
                want = composed.centralized(xs, dtype, bool(average))
            for pieces in (1, 3):
                got, _ = run_op(bc, comms, xs, dtype, average, pieces)
                for r in range(p):
                    assert_float_bits_equal(got[r], want[r], dtype,
                                            f"{cls} dtype={dtype} average={average} pieces={pieces} rank {r}")


# -------------------------------------------------- hierarchical and the bucket op ----
def test_hierarchical_op(bc, composed):
    from test_gpu_hierarchical import _node_reduce, _run, _topology
    N = bc._native
    nodes, per_node = 2, 2
    p = nodes * per_node
    n = 1000 * nodes
    rng = np.random.default_rng(86)
    xs = [(rng.standard_normal(n) * 1e-3).astype(np.float32) for _ in range(p)]
    comms = _topology(bc, nodes, per_node)
    ts = [torch.from_numpy(x.copy()).cuda() for x in xs]
    torch.cuda.synchronize()

    def rank(g):
        intra, inter = comms[g]
        raw = bc.BaguaTensorPy(ts[g], "g").raw()
        N.check(N.C.bagua_centralized_low_precision_hierarchical(
            intra.handle, inter.handle if inter is not None else None, ctypes.byref(raw), 1, N.COMPRESSION_MXFP6),
            "hierarchical op")

    _run(p, rank)
    want = composed.centralized([_node_reduce(xs[k * per_node:(k + 1) * per_node], True) for k in range(nodes)], F32, True)
    for g in range(p):
        same_bytes(host(ts[g], F32), want[g // per_node], f"rank {g}")


def test_bucket_op_runs(bc, composed):
    from bagua_core.communicator import loopback_communicators
    comm = loopback_communicators(1, 0)[0]
    n = 3 * 5000 + 7
    x = grads(np.random.default_rng(36), n, F32)
    t = torch.zeros(n, device="cuda")
    bt = bc.BaguaTensorPy(t, "g")
    bk = bc.BaguaBucketPy("mxfp6_bucket", [bt])
    bk.append_centralized_synchronous_op(comm, None, hierarchical=False, average=True, compression="MXFP6")
    backend = bc.BaguaCommBackendPy(4, 0)
    backend.register_ordered_buckets([bk])
    t.copy_(torch.from_numpy(x))
    ev = torch.cuda.Event()
    ev.record()
    backend.mark_communication_ready(bt, ev.cuda_event)
    assert backend.wait_pending_comm_ops() == 1
    same_bytes(host(t, F32), composed.centralized([x], F32, True)[0], "bucket op")


# --------------------------------------------------------------- schedule check ----
def _ef_raws(st):
    return [st._raw(t) for t in st.tensors()]


def test_schedule_check(bc, composed, monkeypatch, capfd):
    """BAGUA_CHECK_SCHEDULE=1 at p = 2: ranks that ask for different piece counts, for different block codecs,
    or for the plain and the error-feedback op all fail before anything is posted, and the first field that
    differs between two ops of different kinds is the op kind (kOpMxfp6Pipelined, kOpMxfp6ErrorFeedback are
    this codec's own); matching ranks pass, plain and with error feedback"""
    monkeypatch.setenv("BAGUA_CHECK_SCHEDULE", "1")
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    p, cs = 2, 5 * 4096
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(176)
    xs = [step_grads(rng, p * cs, F32, r) for r in range(p)]
    ts = [dev(x, F32) for x in xs]
    states = [bc.MXFP6ErrorFeedbackState(p * cs, p, 0) for _ in range(p)]
    torch.cuda.synchronize()
    raws = [bc.BaguaTensorPy(t, "g").raw() for t in ts]
    srs = [_ef_raws(st) for st in states]
    op = N.C.bagua_centralized_low_precision_pipelined

    def ef(r):
        return N.C.bagua_centralized_mxfp6_error_feedback(comms[r].handle, ctypes.byref(raws[r]), 1,
                                                          ctypes.byref(srs[r][0]), ctypes.byref(srs[r][1]))

    def mismatch(fn, what):
        capfd.readouterr()
        rcs = _run_each(p, fn)
        assert rcs == [ERR_INVALID_ARG] * p, (what, rcs)
        return capfd.readouterr().err

    for mine in ((4, 2), (3, 1), (3, 3 | TAPERED)):
        mismatch(lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP6, mine[r]), mine)
    methods = (N.COMPRESSION_MXFP6, N.COMPRESSION_MXFP8)
    log = mismatch(lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, methods[r], 3), "codecs")
    assert "op schedule mismatch" in log and ": op " in log and ": method " not in log, log
    log = mismatch(lambda r: ef(r) if r else op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP6, 3),
                   "plain against error feedback")
    assert ": op " in log and ": schedule " not in log, log
    for r in range(p):
        same_bytes(host(ts[r], F32), xs[r], f"rank {r} must be untouched")
        assert not any(t.any() for t in states[r].tensors()), f"rank {r}: residuals must be untouched"
    rcs = _run_each(p, lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP6, 3))
    assert rcs == [0] * p, rcs
    want = composed.centralized(xs, F32, True)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"matching ranks, rank {r}")
        ts[r].copy_(dev(xs[r], F32))
    torch.cuda.synchronize()
    assert _run_each(p, ef) == [0] * p
    refs = [REF.OpState(p * cs, p) for _ in range(p)]
    want, _ = REF.centralized_step(NP, xs, F32, refs, True)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"matching ranks with error feedback, rank {r}")
        same_bytes(host(states[r].worker_residual, F32), refs[r].worker, f"rank {r}: worker residual")
        same_bytes(host(states[r].server_residual, F32), refs[r].server, f"rank {r}: server residual")


# ---------------------------------------------------------- error-feedback op ----
def ef_steps(bc, p, dtype, average, steps, what, equal=same_bytes):
    """the op step by step against centralized_step: results and both residuals; returns rank 0's kernel names
    of the first step and, per step, every rank's (worker, server) residuals"""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    n = steps[0][0].size
    comms = loopback_communicators(p, 0)
    states = [bc.MXFP6ErrorFeedbackState(n, p, 0) for _ in range(p)]
    refs = [REF.OpState(n, p) for _ in range(p)]
    names = KernelNames(N, comms[0])
    residuals = []
    for step, xs in enumerate(steps):
        with np.errstate(over="ignore", invalid="ignore"):
            want, _ = REF.centralized_step(NP, xs, dtype, refs, bool(average))
        ts = [dev(x, dtype) for x in xs]
        torch.cuda.synchronize()

        def rank(r):
            raw, sr = bc.BaguaTensorPy(ts[r], f"g{r}").raw(), _ef_raws(states[r])
            with names if r == 0 and step == 0 else contextlib.nullcontext():
                N.check(N.C.bagua_centralized_mxfp6_error_feedback(comms[r].handle, ctypes.byref(raw), average,
                                                                   ctypes.byref(sr[0]), ctypes.byref(sr[1])), f"rank {r}")

        run_ranks(rank, p)
        residuals.append([(host(s.worker_residual, F32).copy(), host(s.server_residual, F32).copy()) for s in states])
        for r in range(p):
            equal(host(ts[r], dtype), want[r], f"{what} step {step} rank {r}: result")
            same_bytes(residuals[-1][r][0], refs[r].worker, f"{what} step {step} rank {r}: worker residual")
            same_bytes(residuals[-1][r][1], refs[r].server, f"{what} step {step} rank {r}: server residual")
    return names.names, residuals


def test_error_feedback_composed_middle_step_at_17_ranks(bc):
    """the fused middle step refuses 17 segments: decode + reduce_chunks_kernel into the tensor, then the worker
    encode on the own chunk alone as a one-chunk tensor, with the server residual (cs elements, this rank's)"""
    p, cs = 17, 1536
    rng = np.random.default_rng(1717)
    steps = [[step_grads(rng, p * cs, F32, r) for r in range(p)] for _ in range(2)]
    names, residuals = ef_steps(bc, p, F32, 1, steps, "p=17")
    assert names.count("mxfp6_encode_ef_kernel") == 2 and "reduce_chunks_kernel" in names, names
    assert "mxfp6_reduce_encode_ef_kernel" not in names, names
    assert all(w.any() and s.any() for w, s in residuals[-1])


@pytest.mark.parametrize("average", [1, 0])
@pytest.mark.parametrize("p", [3, 16])
def test_error_feedback_sum_and_average(bc, p, average):
    cs = 3072 + 40
    for dtype in (F16, BF16):
        rng = np.random.default_rng(100 * p + 10 * dtype + average)
        steps = [[step_grads(rng, p * cs, dtype, r) for r in range(p)] for _ in range(2)]
        names, _ = ef_steps(bc, p, dtype, average, steps, f"p={p} dtype={dtype} average={average}")
        assert names == EF_FUSED, names


@pytest.mark.parametrize("cls", E.EF_CLASSES)
def test_error_feedback_hostile_gradients(bc, cls):
    """the class on step 1, benign on step 2; the blocks that held the NaN keep +0 residuals after step 1: the
    worker's on rank p - 1, the server's on the rank that owns the planted chunk"""
    p, cs = 3, 3072
    for dtype in (F32, BF16):
        rng = E.case_rng("mxfp6ef", cls, dtype)
        steps = [E.build(cls, p, cs, dtype, rng), E.build("benign", p, cs, dtype, rng)]
        equal = lambda got, want, what: assert_float_bits_equal(got, want, dtype, what)  # noqa: E731
        names, residuals = ef_steps(bc, p, dtype, 1, steps, f"{cls} dtype={dtype}", equal)
        assert names == EF_FUSED, names
        assert all(np.isfinite(w).all() and np.isfinite(s).all() for step in residuals for w, s in step)
        if cls == "one_nan":
            (c,) = E.planted_chunks(p)
            b = cs // 2 // 32 * 32
            worker, server = residuals[0][p - 1][0], residuals[0][c][1]
            assert not worker[c * cs + b:c * cs + b + 32].view(np.uint32).any() and worker[c * cs:c * cs + b].any()
            assert not server[b:b + 32].view(np.uint32).any() and server[:b].any()


# ------------------------------------------------------------------- real RCCL ----
def test_ops_over_rccl(tmp_path, composed):
    """two processes, each its own RCCL communicator on the one GPU (set up as test_pipelined_op_over_rccl of
    tests/test_gpu_mxfp8_op.py): 3 pieces, the automatic count, which BAGUA_PIPELINE_MIN_PIECE=4096 makes
    pieced too (a chunk's segment is 640 + 15360 = 16000 bytes), then two error-feedback steps on one state"""
    world, cs = 2, 5 * 4096
    assert R.segment_bytes(cs) == 16000
    rng = np.random.default_rng(1360)
    xs = [step_grads(rng, world * cs, F32, r) for r in range(world)]
    want = composed.centralized(xs, F32, True)
    refs = [REF.OpState(world * cs, world) for _ in range(world)]
    want_ef = []
    for _ in range(2):
        outs, _sent = REF.centralized_step(NP, xs, F32, refs, True)
        want_ef.append((outs, [(s.worker.copy(), s.server.copy()) for s in refs]))
    np.savez(tmp_path / "inputs.npz", **{f"x{r}": x for r, x in enumerate(xs)})
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"NCCL_HOSTID": f"bagua-test-rank-{r}", "NCCL_SOCKET_IFNAME": "lo", "NCCL_IB_DISABLE": "1",
                    "HSA_ENABLE_IPC_MODE_LEGACY": "0", "BAGUA_PIPELINE_MIN_PIECE": "4096"})
        log = open(tmp_path / f"rank{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, "-u", WORKER, str(r), str(world), str(tmp_path), "3,0,ef"],
                                       stdout=log, stderr=subprocess.STDOUT, env=env, cwd=ROOT), log))
    failed = []
    for r, (proc, log) in enumerate(procs):
        try:
            rc = proc.wait(timeout=90)
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
                same_bytes(z[f"t{i}"], want[r], f"rank {r}, pieces={pieces}")
            for step, (outs, res) in enumerate(want_ef):
                same_bytes(z[f"ef{step}"], outs[r], f"rank {r}, error feedback step {step}")
                same_bytes(z[f"worker{step}"], res[r][0], f"rank {r}, step {step}: worker residual")
                same_bytes(z[f"server{step}"], res[r][1], f"rank {r}, step {step}: server residual")
