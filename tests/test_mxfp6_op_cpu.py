"""The references of the MXFP6 op tests (tests/test_gpu_mxfp6_op.py) are sound on those tests'
inputs, without a GPU: mxfp8_reference's composed op over this codec's compress and decompress
(the `composed` fixture of tests/test_gpu_mxfp6.py) and mxfp6_ef_reference.centralized_step.

Every rank's result has the same bytes; a hostile class makes exactly the share of the result
NaN that its plant explains, never more than half (a NaN compares equal to any NaN, so it must
not cover a chunk that could be wrong); on benign f32 data every element lies within the codec's
error of the float64 mean, a bound that owes nothing to the reference's own code; the references
run at 17 ranks; and the byte ranges of the pieced exchange (csrc/runtime/schedule.cpp,
mx_block_pieces with 24 bytes per block) cover a segment exactly at every payload slack, which
they do not with another codec's block size."""
import numpy as np
import pytest

import mxfp6_ef_reference as REF
import mxfp6_reference as R
import op_edge_cases as E
from oracle import oracle_np as NP
from test_gpu_mxfp6 import composed  # noqa: F401  (the fixture; that module's tests stay its own)
from test_gpu_mxfp8 import grads

F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
CS, CS_VEC = 4 * 4096 + 77, 4 * 4096 + 80      # test_gpu_mxfp6_op.py
HOSTILE_P, HOSTILE_CS = 4, 2 * 4096 + 40
EF_P, EF_CS = 3, 3072
SLACK_SIZES = [4 * 4096 + d for d in (32, 64, 96, 128, 40)]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def ranks_agree(outs, what):
    for r, o in enumerate(outs[1:], 1):
        assert same(o, outs[0]), f"{what}: rank {r} differs from rank 0"


def within_codec_error(xs, out, p, cs, what):
    """|result - mean| <= (33/256) A (1 + 2^-20), A the largest |x| of the element's block of 32 over all
    ranks: one encode errs by at most amax/16 (MXFP6.md, "Decode": max(|x| 2^-4, 2^(e-4)) with 2^e <
    amax/3.75), the mean of p such errors by at most A/16, the second encode by at most (A + A/16)/16"""
    x = np.stack([a.astype(np.float64) for a in xs])
    mean = x.mean(axis=0)
    nb = R.blocks(cs)
    a = np.zeros((p, nb * 32))
    a[:, :cs] = np.abs(x).max(axis=0).reshape(p, cs)
    A = np.repeat(a.reshape(p, nb, 32).max(axis=2), 32, axis=1)[:, :cs].ravel()
    err = np.abs(out.astype(np.float64) - mean)
    bad = np.nonzero(err > 33.0 / 256.0 * A * (1 + 2.0 ** -20))[0]
    assert bad.size == 0, f"{what}: {bad.size} elements off the mean, first {bad[:4]}: {err[bad[:4]]} against A {A[bad[:4]]}"


@pytest.mark.parametrize("average", [1, 0])
@pytest.mark.parametrize("cls", E.CLASSES)
def test_nan_share_of_the_hostile_cases(composed, cls, average):
    p, cs = HOSTILE_P, HOSTILE_CS
    planted = E.planted_chunks(p)
    for dtype in DTYPES:
        xs = E.build(cls, p, cs, dtype, E.case_rng("mxfp6", cls, dtype))
        with np.errstate(over="ignore", invalid="ignore"):
            outs = composed.centralized(xs, dtype, bool(average))
        what = f"{cls} dtype={dtype} average={average}"
        ranks_agree(outs, what)
        nan = E.is_nan(outs[0], dtype)
        if cls == "all_nan_chunk":    # the two planted chunks of four, whole
            want = np.zeros(p * cs, bool)
            for c in planted:
                want[c * cs:(c + 1) * cs] = True
            assert np.array_equal(nan, want) and 2 * int(nan.sum()) == nan.size, what
        elif cls == "one_nan":        # the block of 32 around element cs // 2 of each planted chunk
            want = np.zeros(p * cs, bool)
            for c in planted:
                b = c * cs + cs // 2 // 32 * 32
                want[b:b + 32] = True
            assert np.array_equal(nan, want) and round(nan.mean(), 4) == 0.0019, what
        else:
            assert not nan.any(), f"{what}: {int(nan.sum())} NaN"
        assert 2 * int(nan.sum()) <= nan.size
        if cls == "benign" and dtype == F32 and average:
            within_codec_error(xs, outs[0], p, cs, what)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cls", E.EF_CLASSES)
def test_error_feedback_cases_recover(cls, dtype):
    """the class on step 1, benign on step 2: the second result has no NaN and every residual stays finite"""
    p, cs = EF_P, EF_CS
    rng = E.case_rng("mxfp6ef", cls, dtype)
    steps = [E.build(cls, p, cs, dtype, rng), E.build("benign", p, cs, dtype, rng)]
    for average in (True, False):
        states = [REF.OpState(p * cs, p) for _ in range(p)]
        for step, xs in enumerate(steps):
            with np.errstate(over="ignore", invalid="ignore"):
                outs, _ = REF.centralized_step(NP, xs, dtype, states, average)
            ranks_agree(outs, f"{cls} dtype={dtype} step {step}")
            for s in states:
                assert np.isfinite(s.worker).all() and np.isfinite(s.server).all(), (cls, dtype, step)
            nans = int(E.is_nan(outs[0], dtype).sum())
            if step == 0:
                assert nans == (32 if cls == "one_nan" else 0), (cls, dtype, nans)   # p = 3: one planted chunk
            else:
                assert nans == 0, (cls, dtype, nans)


@pytest.mark.parametrize("p", [1, 2, 3, 8, 16])
def test_benign_result_within_the_codec_error_of_the_mean(composed, p):
    """the shapes of the piece-count tests; a reference that reduced the wrong chunk would leave the bound"""
    rng = np.random.default_rng(77 + p)
    for cs in (CS, CS_VEC):
        xs = [grads(rng, p * cs, F32) for _ in range(p)]
        outs = composed.centralized(xs, F32, True)
        ranks_agree(outs, f"p={p} cs={cs}")
        assert not np.isnan(outs[0]).any()
        within_codec_error(xs, outs[0], p, cs, f"p={p} cs={cs}")


def test_seventeen_ranks(composed):
    """p = 17, cs = 1536: plain, partly valid (3e38 past num_elem counts as +0 and decodes to +0) and two
    error-feedback steps"""
    p, cs = 17, 1536
    rng = np.random.default_rng(1700)
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    outs = composed.centralized(xs, F32, True)
    ranks_agree(outs, "plain")
    within_codec_error(xs, outs[0], p, cs, "plain")
    num_elem = p * cs - cs // 2 - 3
    ys = [x.copy() for x in xs]
    for y in ys:
        y[num_elem:] = 3e38
    part = composed.centralized(ys, F32, True, num_elem=num_elem)
    ranks_agree(part, "partly valid")
    assert not part[0][num_elem:].view(np.uint32).any() and np.isfinite(part[0]).all()
    within_codec_error([np.where(np.arange(p * cs) < num_elem, y, 0).astype(np.float32) for y in ys], part[0], p, cs,
                       "partly valid")
    assert same(part[0][:(p - 1) * cs], outs[0][:(p - 1) * cs]), "the chunks before the last are fully valid"
    states = [REF.OpState(p * cs, p) for _ in range(p)]
    for step in range(2):
        outs, sent = REF.centralized_step(NP, xs, F32, states, True)
        ranks_agree(outs, f"error feedback step {step}")
        assert np.isfinite(outs[0]).all() and all(s.worker.any() and s.server.any() for s in states)
        if step == 0:   # zero state: the plain op's wire bytes
            assert all(same(sent[r], R.compress(xs[r], F32, p)) for r in range(p))


def test_the_references_tell_a_wrong_op_apart(composed):
    """what the GPU tests compare against changes when the op's composition does: the mode, the valid
    length, and which residual the error-feedback middle step compensates with"""
    p, cs = EF_P, EF_CS
    rng = np.random.default_rng(31)
    xs = [grads(rng, p * cs, F32) for _ in range(p)]
    mean = composed.centralized(xs, F32, True)[0]
    assert not same(mean, composed.centralized(xs, F32, False)[0])
    num_elem = p * cs - cs // 2 - 3
    ys = [x.copy() for x in xs]
    for y in ys:
        y[num_elem:] = 3e38
    with np.errstate(over="ignore"):
        counted = composed.centralized(ys, F32, True)[0]
    assert not same(composed.centralized(ys, F32, True, num_elem=num_elem)[0], counted)
    right = [REF.OpState(p * cs, p) for _ in range(p)]
    out, _ = REF.centralized_step(NP, xs, F32, right, True)

    class WorkerAsServer:   # the middle step handed the own chunk's slice of the worker residual
        def __init__(self, r):
            self.worker = np.zeros(p * cs, np.float32)
            self.server = self.worker[r * cs:(r + 1) * cs]

    wrong, _ = REF.centralized_step(NP, xs, F32, [WorkerAsServer(r) for r in range(p)], True)
    assert not same(out[0], wrong[0])
    first = [REF.OpState(p * cs, p) for _ in range(p)]   # and a second step depends on both residuals of the first
    REF.centralized_step(NP, xs, F32, first, True)
    for s in first:
        s.server[:] = 0
    assert not same(REF.centralized_step(NP, xs, F32, right, True)[0][0], REF.centralized_step(NP, xs, F32, first, True)[0][0])


def exchanged(cs, pieces, block_bytes):
    """one segment through the pieced schedule, every buffer 0xFF at first.  Piece by piece: the encode writes
    the piece's bytes into `send`, the exchange moves the scale bytes [b, e) and the payload bytes [sbytes +
    block_bytes b, sbytes + block_bytes e) to `recv` (to the end of both regions on the piece that ends the
    chunk: schedule.cpp mx_block_pieces), and the piece's consumer reads its bytes from `recv`.  A kernel's
    own ranges are the codec's, 24 bytes per block."""
    rng = np.random.default_rng(cs)
    seg = R.compress(grads(rng, cs, F32), F32, 1)
    nb, sb, co = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    send, recv, got = (np.full(co, 0xFF, np.uint8) for _ in range(3))

    def ranges(b, e, bytes_per_block):
        return ((b, sb if e == nb else e), (sb + bytes_per_block * b, co if e == nb else sb + bytes_per_block * e))

    filled = 0
    for q in range(pieces):
        b, e = R.piece_range(cs, pieces, q)
        if b >= e:
            continue
        filled += 1
        for lo, hi in ranges(b, e, R.BLOCK_BYTES):
            send[lo:hi] = seg[lo:hi]
        for lo, hi in ranges(b, e, block_bytes):
            recv[lo:hi] = send[lo:hi]
        for lo, hi in ranges(b, e, R.BLOCK_BYTES):
            got[lo:hi] = recv[lo:hi]
    return got, seg, filled


@pytest.mark.parametrize("cs", SLACK_SIZES)
def test_piece_byte_ranges_cover_the_segment_at_every_slack(cs):
    """nb mod 4 = 1, 2, 3, 0 (and a ragged block of 8 elements at 2): 24 bytes per block give the whole
    segment, slack included; with MXFP4's 16 a piece is read before it has arrived, with MXFP8's 32 bytes
    move before they are encoded and the second piece's range runs past the segment"""
    nb = R.blocks(cs)
    assert R.payload_bytes(cs) - 24 * nb == {1: 8, 2: 16, 3: 24, 0: 0}[nb % 4]
    got, seg, filled = exchanged(cs, 3, R.BLOCK_BYTES)
    assert filled == 3 and same(got, seg)
    for wrong in (16, 32):
        got, seg, _ = exchanged(cs, 3, wrong)
        assert not same(got, seg), wrong
    assert R.scale_bytes(cs) + 32 * R.piece_range(cs, 3, 1)[1] > R.segment_bytes(cs)
