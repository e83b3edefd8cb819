"""GPU tests of the pipelined MXFP4 centralized op (csrc/runtime/comm_ops.cpp
centralized_pipelined_mxfp4; MXFP4.md, "Pipelined op") on the in-process loopback transport:
every rank's result byte for byte against the same call with one piece and against the numpy
reference of the op (tests/mxfp4_reference.py), the path taken from the kernel names rank 0
launched, the shapes that must run unpieced, reuse of a communicator, hostile values across
piece boundaries, the schedule check and the automatic piece count.

Chunk sizes: 3 * 4096 + 1192 (three granule boundaries, a ragged last tile and block),
5 * 4096 (all vector) and 8 * 4096 + 8 (a last piece of one 8-element block)."""
import ctypes

import numpy as np
import pytest
import torch

import mxfp4_reference as R
from oracle import oracle_np as NP
from test_gpu_multirank import dev, host
from test_gpu_mxfp4 import BF16, DTYPES, F16, F32, dev_at, grads, hostile_inputs, run_centralized, same_bytes
from test_gpu_schedule_check import _run_each

pytestmark = pytest.mark.gpu

TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
ERR_INVALID_ARG = 1
SCHEDULE_ENV = ("BAGUA_PIPELINE_TAPER", "BAGUA_PIPELINE_PIECES", "BAGUA_PIPELINE_MIN_PIECE", "BAGUA_CHECK_SCHEDULE")
KERNELS = ("mxfp4_encode_kernel", "mxfp4_reduce_encode_kernel", "mxfp4_decode_kernel")


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


@pytest.fixture(autouse=True)
def default_schedule_env(monkeypatch):
    for k in SCHEDULE_ENV:
        monkeypatch.delenv(k, raising=False)


def pipelined(bc, pieces):
    """the pipelined entry with `pieces`, in the shape run_centralized calls"""
    op = bc._native.C.bagua_centralized_low_precision_pipelined
    return lambda comm, raw, average, method: op(comm, raw, average, method, pieces)


def filled_pieces(bc, cs, schedule):
    b, e = ctypes.c_int(), ctypes.c_int()
    n = 0
    for q in range(schedule & 0xFFFF):
        assert bc._native.K.bagua_mxfp4_piece_range(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == 0
        n += e.value > b.value
    return n


def counts(names):
    return [names.count(k) for k in KERNELS]


def run_op(bc, comms, xs, dtype, average, pieces, timed=False, num_elem=None, offsets=None):
    """the op on fresh device copies of xs (rank r's tensor offsets[r] elements into its allocation);
    returns (every rank's result, the kernel names of rank 0 when timed)"""
    ts = [dev_at(x, dtype, offsets[r] if offsets else 0) for r, x in enumerate(xs)]
    names = run_centralized(bc, comms, pipelined(bc, pieces), ts, average, num_elem=num_elem, timed=timed)
    return [host(t, dtype).copy() for t in ts], names


@pytest.mark.parametrize("cs", [3 * 4096 + 1192, 5 * 4096, 8 * 4096 + 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [2, 3, 4, 8, 16])
def test_result_bytes(bc, monkeypatch, p, dtype, cs):
    from bagua_core.communicator import loopback_communicators
    rng = np.random.default_rng(10000 * p + 100 * dtype + cs % 97)
    comms = {}
    for taper in (None, "0", "1"):  # read when the communicators are created
        if taper is not None:
            monkeypatch.setenv("BAGUA_PIPELINE_TAPER", taper)
        comms[taper] = loopback_communicators(p, 0)
    for average in (0, 1):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        want = R.centralized(xs, dtype, bool(average))
        one, _ = run_op(bc, comms[None], xs, dtype, average, 1)
        for r in range(p):
            same_bytes(one[r], want[r], f"p={p} dtype={dtype} cs={cs} average={average} one piece, rank {r}")
        for taper in (None, "0", "1"):
            for pieces in (2, 3, 4, 8):
                got, _ = run_op(bc, comms[taper], xs, dtype, average, pieces)
                for r in range(p):
                    what = f"p={p} dtype={dtype} cs={cs} average={average} taper={taper} pieces={pieces} rank {r}"
                    same_bytes(got[r], one[r], f"{what} against one piece")
                    same_bytes(got[r], want[r], f"{what} against the reference")


@pytest.mark.parametrize("taper", [None, "1"])
@pytest.mark.parametrize("pieces", [2, 3, 4, 8, 4 | TAPERED])
def test_path_taken(bc, monkeypatch, pieces, taper):
    """as many encode, middle-step and decode launches as the schedule has non-empty pieces, and
    no reduce_chunks_kernel (a build that ignores `pieces` for MXFP4 launches one of each)"""
    from bagua_core.communicator import loopback_communicators
    if taper is not None:
        monkeypatch.setenv("BAGUA_PIPELINE_TAPER", taper)
    p, cs = 2, 3 * 4096 + 1192  # 3.3 granules: 8 pieces leave empty ones at the tail
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(321 + pieces)
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    got, names = run_op(bc, comms, xs, F32, 1, pieces, timed=True)
    schedule = pieces | (TAPERED if taper == "1" and (pieces & 0xFFFF) >= 3 else 0)
    k = filled_pieces(bc, cs, schedule)
    assert 1 < k <= (pieces & 0xFFFF)
    assert counts(names) == [k, k, k], (k, names)
    assert "reduce_chunks_kernel" not in names, names
    want = R.centralized(xs, F32, True)
    for r in range(p):
        same_bytes(got[r], want[r], f"rank {r}")


def test_shapes_that_run_unpieced(bc):
    from bagua_core.communicator import loopback_communicators
    rng = np.random.default_rng(55)
    # more ranks than the fused middle step takes: the composed steps, unpieced
    p, cs = 17, 2 * 4096
    comms = loopback_communicators(p, 0)
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    got, names = run_op(bc, comms, xs, F32, 1, 3, timed=True)
    assert counts(names) == [2, 0, 2] and "reduce_chunks_kernel" in names, names
    want = R.centralized(xs, F32, True)
    for r in range(p):
        same_bytes(got[r], want[r], f"p=17 rank {r}")
    # a partly valid tensor (huge values past the last valid element)
    p, cs = 2, 3 * 4096
    comms = loopback_communicators(p, 0)
    num_elem = p * cs - cs // 2 - 3
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    for x in xs:
        x[num_elem:] = 3e38
    got, names = run_op(bc, comms, xs, F32, 1, 3, timed=True, num_elem=num_elem)
    assert counts(names) == [2, 0, 2] and "reduce_chunks_kernel" in names, names
    want = R.centralized(xs, F32, True, num_elem=num_elem)
    for r in range(p):
        same_bytes(got[r], want[r], f"partly valid rank {r}")
    # chunks that are not 16-B multiples: the fused op, unpieced
    for dtype, cs in ((F32, 3 * 4096 + 2), (BF16, 3 * 4096 + 4)):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        got, names = run_op(bc, comms, xs, dtype, 0, 3, timed=True)
        assert counts(names) == [1, 1, 1] and "reduce_chunks_kernel" not in names, names
        want = R.centralized(xs, dtype, False)
        for r in range(p):
            same_bytes(got[r], want[r], f"dtype={dtype} cs={cs} rank {r}")
    # one piece asked for: the unpieced op
    xs = [grads(rng, p * 5 * 4096, F32) for _ in range(p)]
    _, names = run_op(bc, comms, xs, F32, 1, 1, timed=True)
    assert counts(names) == [1, 1, 1], names


@pytest.mark.parametrize("misaligned_rank", [0, 1])
@pytest.mark.parametrize("dtype", [F32, F16])
def test_one_rank_misaligned(bc, dtype, misaligned_rank):
    """one rank's tensor starts one element into its allocation: that rank runs the same pieced
    schedule on an aligned copy, every rank posts the same exchanges, the bytes are the same"""
    from bagua_core.communicator import loopback_communicators
    p, cs, pieces = 3, 3 * 4096 + 1192, 3
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(808 + dtype)
    xs = [grads(rng, p * cs, dtype) for _ in range(p)]
    offsets = [1 if r == misaligned_rank else 0 for r in range(p)]
    got, names = run_op(bc, comms, xs, dtype, 1, pieces, timed=True, offsets=offsets)
    k = filled_pieces(bc, cs, pieces)
    assert k > 1 and counts(names) == [k, k, k], names  # rank 0, misaligned or not
    want = R.centralized(xs, dtype, True)
    for r in range(p):
        same_bytes(got[r], want[r], f"rank {r}")


def test_back_to_back(bc):
    """several ops in a row on the same communicators with different piece counts: the pool's
    buffers, the events and the side stream are reused"""
    from bagua_core.communicator import loopback_communicators
    p, cs = 4, 5 * 4096
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(99)
    for dtype, pieces in ((F32, 3), (F32, 8), (BF16, 2), (F32, 4 | TAPERED), (F32, 1), (F32, 5)):
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        got, _ = run_op(bc, comms, xs, dtype, 1, pieces)
        want = R.centralized(xs, dtype, True)
        for r in range(p):
            same_bytes(got[r], want[r], f"dtype={dtype} pieces={pieces:#x} rank {r}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_values_across_piece_boundaries(bc, dtype):
    """the NaN-block and +-Inf classes of test_gpu_mxfp4.hostile_inputs, planted around the
    piece and granule boundaries of both chunks of rank 0's tensor and in the ragged tail of
    rank 1's, through 3 pieces (384, 384 and 38 blocks) at p = 2"""
    from bagua_core.communicator import loopback_communicators
    cases, p = hostile_inputs(dtype)
    assert p == 2
    cs = 6 * 4096 + 1192
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(4242 + dtype)
    for name in ("nan middle block", "nan last ragged block", "inf"):
        h = cases[name][:1000]
        xs = [grads(rng, p * cs, dtype) for _ in range(p)]
        for c in range(p):
            for edge in (4096, 3 * 4096, 6 * 4096):
                xs[0][c * cs + edge - 500:c * cs + edge + 500] = h
            xs[1][(c + 1) * cs - 1000:(c + 1) * cs] = h
        with np.errstate(over="ignore", invalid="ignore"):
            want = R.centralized(xs, dtype, True)
        got, names = run_op(bc, comms, xs, dtype, 1, 3, timed=True)
        assert counts(names) == [3, 3, 3], names
        for r in range(p):
            same_bytes(got[r], want[r], f"{name}: rank {r}")
        if name != "inf":
            assert np.isnan(NP.to_f32(want[0], dtype)).any()


def test_schedule_check(bc, monkeypatch):
    """BAGUA_CHECK_SCHEDULE=1: ranks that ask for different piece counts all fail with invalid
    argument before anything is posted (tensors untouched, nothing hangs); matching ranks pass"""
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
    for mine in ((4, 2), (3, 1), (3, 3 | TAPERED)):  # other counts, pieced against unpieced, other edges
        rcs = _run_each(p, lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP4, mine[r]))
        assert rcs == [ERR_INVALID_ARG] * p, (mine, rcs)
        for r in range(p):
            same_bytes(host(ts[r], F32), xs[r], f"{mine}: rank {r} must be untouched")
    rcs = _run_each(p, lambda r: op(comms[r].handle, ctypes.byref(raws[r]), 1, N.COMPRESSION_MXFP4, 3))
    assert rcs == [0] * p, rcs
    want = R.centralized(xs, F32, True)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"matching ranks, rank {r}")


@pytest.mark.parametrize("min_piece", [None, "4096"])
def test_automatic_piece_count(bc, monkeypatch, min_piece):
    """bagua_centralized_low_precision_synchronous (pieces = 0): a chunk's segment of 17408 bytes is
    one piece under the default BAGUA_PIPELINE_MIN_PIECE (1 MiB) and four tapered pieces (the
    cap) under 4096, read when the communicators are created"""
    from bagua_core.communicator import loopback_communicators
    if min_piece is not None:
        monkeypatch.setenv("BAGUA_PIPELINE_MIN_PIECE", min_piece)
    N = bc._native
    p, cs = 2, 8 * 4096
    comms = loopback_communicators(p, 0)
    rng = np.random.default_rng(23)
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    ts = [dev(x, F32) for x in xs]
    names = run_centralized(bc, comms, N.C.bagua_centralized_low_precision_synchronous, ts, 1, timed=True)
    k = 1 if min_piece is None else filled_pieces(bc, cs, 4 | TAPERED)
    assert k in (1, 4) and counts(names) == [k, k, k], names
    assert "reduce_chunks_kernel" not in names, names
    want = R.centralized(xs, F32, True)
    for r in range(p):
        same_bytes(host(ts[r], F32), want[r], f"rank {r}")
