"""GPU tests of MXFP8 stochastic rounding (MXFP8.md): the stochastic kernels under both conversions, their C entries,
the op, the bucket op and the Python surface, byte for byte against tests/mxfp8_sr_reference.py.  Launch geometry as in
tests/test_gpu_mxfp8.py: an encode workgroup covers 8192 f32 / 16384 16-bit elements, a middle-step one 8192."""
import ctypes

import numpy as np
import pytest
import torch

import bagua_core as bc
import mxfp8_boundary_cases as B
import mxfp8_reference as R
import mxfp8_sr_reference as SR
from bagua_core.communicator import loopback_communicators
from test_gpu_multirank import host, run_ranks
from test_gpu_mxfp8 import (BF16, DTYPES, F16, F32, INVALID_ARG, OK, UNSUPPORTED, dev_at, grads, piece_ranges,
                            received, same_bytes, u8)

pytestmark = pytest.mark.gpu

KEY = SR.key(0xB0A8, 3, 1, 0)
FILL = 0xA5


@pytest.fixture(autouse=True, params=["1", "0"])
def hw(request, monkeypatch):
    """every test under both conversions; the grid and schedule knobs at their defaults"""
    for k in ("BAGUA_TUNE_MX8_ENCODE_BLOCKS", "BAGUA_TUNE_MX8_MIDDLE_BLOCKS", "BAGUA_PIPELINE_PIECES", "BAGUA_CHECK_SCHEDULE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BAGUA_MXFP8_HWCVT", request.param)


def launch(entry, ranges, head, S, target, key):
    """the whole-chunk entry, or its _range form over every non-empty [b, e) of `ranges`, into S bytes of FILL"""
    K, out = bc._native.K, torch.full((S,), FILL, dtype=torch.uint8, device="cuda")
    if ranges is None:
        assert getattr(K, entry)(*head, out.data_ptr(), S, target, key, None) == OK
    for b, e in [r for r in ranges or () if r[0] < r[1]]:
        mid = (out.data_ptr(), S) if "compress" in entry else (out.data_ptr(), S, target)
        assert getattr(K, entry + "_range")(*head, *mid, b, e, key, None) == OK
    return u8(out)


def encode(x, dtype, cs, p, key, target=-1, num_elem=None, offset=0, ranges=None):
    xt = dev_at(x, dtype, offset)
    head = (dtype, xt.data_ptr(), x.size if num_elem is None else num_elem, cs, p)
    return launch("bagua_mxfp8_compress_sr", ranges, head, R.compressed_bytes(cs, p), target, key)


def check_middle(recv, dtype, cs, p, target, average, key, what, ranges=None):
    """the middle step's bytes, whole or over `ranges`, against decode + reduce + compress_sr(target) of the reference"""
    rt = torch.from_numpy(recv).cuda()
    head = (dtype, rt.data_ptr(), recv.size, cs, p, average)
    want = SR.reduce_requantize_sr(recv, p, cs, dtype, target, bool(average), key, out=np.full(recv.size, FILL, np.uint8))
    same_bytes(launch("bagua_mxfp8_reduce_requantize_sr", ranges, head, recv.size, target, key), want, what)


@pytest.mark.parametrize("one_workgroup", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_against_the_reference(dtype, one_workgroup, monkeypatch):
    """cs = 37031: two whole workgroup tiles of the 16-bit encode, a partial tile, a ragged last block, the slack; odd, so
    chunks 1 and 2 start at an odd and an even index on the guarded path; cs = 32768: the vector path.  Then one target
    chunk, a partly valid tensor, a tensor offset by one element; 1, 2 and 4 chunks of whole blocks; 3 pieces."""
    if one_workgroup:
        monkeypatch.setenv("BAGUA_TUNE_MX8_ENCODE_BLOCKS", "1")  # one workgroup strides over every tile
    cs = 2 * 16384 + 4096 + 5 * 32 + 7
    x = grads(np.random.default_rng(1000 + dtype), 3 * cs, dtype)
    for p, size in ((1, cs), (3, cs), (3, 32768)):
        got = encode(x[:p * size], dtype, size, p, KEY)
        same_bytes(got, SR.compress_sr(x[:p * size], dtype, p, KEY), f"cs={size} p={p}")
    plain, nb = R.compress(x[:p * size], dtype, p), R.blocks(size)
    assert np.array_equal(got[:nb], plain[:nb]) and not np.array_equal(got, plain)  # the plain scale bytes
    want = SR.compress_sr(x, dtype, 3, KEY, 1, out=np.full(R.compressed_bytes(cs, 3), FILL, np.uint8))
    same_bytes(encode(x, dtype, cs, 3, KEY, target=1), want, "target 1")
    same_bytes(encode(x, dtype, cs, 3, KEY, num_elem=cs + 517), SR.compress_sr(x, dtype, 3, KEY, num_elem=cs + 517),
               "partly valid")
    same_bytes(encode(x, dtype, cs, 3, KEY, offset=1), SR.compress_sr(x, dtype, 3, KEY), "offset by one element")
    n = 4 * 4096  # index invariance: the same payload bytes for the same elements however the tensor is cut
    pay = [encode(x[:n], dtype, n // p, p, KEY).reshape(p, -1)[:, R.scale_bytes(n // p):].ravel() for p in (1, 2, 4)]
    same_bytes(pay[0], SR.compress_sr(x[:n], dtype, 1, KEY)[R.scale_bytes(n):], "1 chunk")
    same_bytes(np.concatenate(pay[1:]), np.tile(pay[0], 2), "2 and 4 chunks against 1")
    cs = 3 * 4096 + 100  # compress_sr_range over the 3 pieces reassembles compress_sr's bytes
    same_bytes(encode(x[:3 * cs], dtype, cs, 3, KEY, ranges=piece_ranges(bc._native.K, cs, 3)),
               encode(x[:3 * cs], dtype, cs, 3, KEY), "3 pieces")


@pytest.mark.parametrize("p", [1, 3, 5, 9, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_middle_step_against_the_reference(dtype, p, monkeypatch):
    """BY = 2, 4, 8; cs = 8295 under one workgroup: the grid strides twice and ends ragged; sum and mean; 3 pieces; 17 segments"""
    monkeypatch.setenv("BAGUA_TUNE_MX8_MIDDLE_BLOCKS", "1")
    cs, target = 8192 + 3 * 32 + 7, p // 2
    recv = received(np.random.default_rng(100 * dtype + p), p, cs, dtype)
    for average in (0, 1):
        check_middle(recv, dtype, cs, p, target, average, KEY, f"p={p} average={average}")
    check_middle(recv, dtype, cs, p, target, 1, KEY, "3 pieces", ranges=piece_ranges(bc._native.K, cs, 3))
    K, S = bc._native.K, R.compressed_bytes(64, 17)
    buf = torch.zeros(2 * S, dtype=torch.uint8, device="cuda")
    head = (dtype, buf.data_ptr(), S, 64, 17, 1, buf.data_ptr() + S, S, 0)
    assert K.bagua_mxfp8_reduce_requantize_sr(*head, KEY, None) == UNSUPPORTED
    assert K.bagua_mxfp8_reduce_requantize_sr_range(*head, 0, 2, KEY, None) == UNSUPPORTED


@pytest.mark.parametrize("dtype,step", [(F32, 0), (F16, 11), (BF16, 0)])
def test_boundary_table(dtype, step):
    """every scale byte T can produce, every tie and its neighbours in T, the E4M3 subnormals, through the encode and the
    middle step at p = 1, under a random key and the key of `step`, which draws r = 0 and r = 0xffff on off-grid elements
    (found by a search over steps on the host).  This test decides the hardware arm."""
    t = B.table(dtype)
    edge = SR.key(0xED6E, step)
    off_grid = (SR.floor_code_and_fraction(R.scaled(t.values(), dtype)[1])[1] >= 1).ravel()
    r = SR.rbits(edge, np.arange(t.x.size, dtype=np.uint64))
    assert ((r == 0) & off_grid).any() and ((r == 0xFFFF) & off_grid).any()
    one = R.compress(t.x, dtype, 1)
    for k in (KEY, edge):
        same_bytes(encode(t.x, dtype, t.x.size, 1, k), SR.compress_sr(t.x, dtype, 1, k), f"encode key={k:#x}")
        check_middle(one, dtype, t.x.size, 1, 0, 0, k, f"middle key={k:#x}")


def run_op(comms, xs, dtype, average, pieces, seed, step, num_elem=None, offsets=None):
    """bagua_centralized_mxfp8_stochastic on fresh device copies of xs; every rank's result"""
    N = bc._native
    ts = [dev_at(x, dtype, offsets[r] if offsets else 0) for r, x in enumerate(xs)]

    def rank(r):
        raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
        raw.num_elem = raw.num_elem if num_elem is None else num_elem
        N.check(N.C.bagua_centralized_mxfp8_stochastic(comms[r].handle, ctypes.byref(raw), average, seed, step, pieces),
                f"rank {r}")

    torch.cuda.synchronize()
    run_ranks(rank, len(ts))
    return [host(t, dtype).copy() for t in ts]


@pytest.mark.parametrize("p,dtype,average,offsets,valid", [(1, F16, 1, None, 1.0), (2, F32, 1, None, 1.0),
                                                           (3, BF16, 0, None, 1.0), (17, F32, 1, None, 1.0),
                                                           (3, F16, 1, [0, 1, 0], 1.0), (3, F32, 1, None, 0.8)])
def test_op_on_loopback(p, dtype, average, offsets, valid):
    """pieces 0, 1 and 3: the bytes of the op simulated with the reference under the keys of (seed, step, rank, stage); one
    case with a misaligned rank, one partly valid (huge values past the last valid element)"""
    comms = loopback_communicators(p, 0)
    cs = 3 * 4096 + 1192 if p < 17 else 1024
    rng = np.random.default_rng(40 + p)
    xs = [grads(rng, p * cs, dtype) for _ in range(p)]
    num_elem = None if valid == 1.0 else int(p * cs * valid) + 3
    for x in xs if num_elem else ():
        x[num_elem:] = 3e38
    want = SR.centralized_sr(xs, dtype, bool(average), 0x5EED, 4, num_elem=num_elem)
    assert not np.array_equal(want[0].view(np.uint8), R.centralized(xs, dtype, bool(average), num_elem)[0].view(np.uint8))
    for pieces in (0, 1, 3):
        got = run_op(comms, xs, dtype, average, pieces, 0x5EED, 4, num_elem, offsets)
        for r in range(p):
            same_bytes(got[r], want[r], f"p={p} dtype={dtype} pieces={pieces} rank {r}")


def test_bucket_python_surface_and_refusals():
    """the refusals leave the bucket as it was; three executions use steps 0, 1, 2: the direct op's bytes, all different"""
    comm = loopback_communicators(1, 0)[0]
    n = 3 * 5000 + 8
    x = grads(np.random.default_rng(3), n, F32)
    want = [run_op([comm], [x], F32, 1, 0, 0xABCD, step)[0] for step in (0, 1, 2)]
    same_bytes(want[1], SR.centralized_sr([x], F32, True, 0xABCD, 1)[0], "the direct op at step 1")
    assert not any(np.array_equal(want[a], want[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    t = torch.zeros(n, device="cuda")
    bt = bc.BaguaTensorPy(t, "g")
    bk = bc.BaguaBucketPy("mxfp8_sr_bucket", [bt])
    r4, r8 = bc.MXFP4StochasticRounding(1), bc.MXFP8StochasticRounding(0xABCD)
    for error, kw in [(NotImplementedError, dict(stochastic_rounding=r4)), (NotImplementedError, dict(compression="MXFP4")),
                      (NotImplementedError, dict(communicator_intranode=comm, hierarchical=True)),
                      (NotImplementedError, dict(error_feedback=bc.MXFP8ErrorFeedbackState(n, 1, 0))),
                      (TypeError, dict(stochastic_rounding=1))]:
        with pytest.raises(error):
            bk.append_centralized_synchronous_op(comm, **{"compression": "MXFP8", "stochastic_rounding": r8, **kw})
        assert len(bk.ops()) == 0
    assert bc._native.C.bagua_centralized_mxfp8_stochastic(comm.handle, None, 1, 1, 0, 1) == INVALID_ARG
    bk.append_centralized_synchronous_op(comm, None, hierarchical=False, average=True, compression="MXFP8",
                                         stochastic_rounding=r8)
    assert type(bk.ops()[0]).__name__ == "CentralizedMXFP8Stochastic"
    backend = bc.BaguaCommBackendPy(4, 0)
    backend.register_ordered_buckets([bk])
    for step in (0, 1, 2):
        t.copy_(torch.from_numpy(x))
        ev = torch.cuda.Event()
        ev.record()
        backend.mark_communication_ready(bt, ev.cuda_event)
        assert backend.wait_pending_comm_ops() == 1
        same_bytes(host(t, F32), want[step], f"execution {step}")
    comp = bt.compress_with_stochastic_rounding(4, bc.MXFP8StochasticRounding((1 << 64) + 0xFACE), 1)
    same_bytes(comp.to_numpy_u8(), SR.compress_sr(host(t, F32), F32, 4, SR.key(0xFACE, 1, 0, 0)), "tensor compress")
    with pytest.raises(TypeError):
        bt.compress_with_stochastic_rounding(4, 0xFACE, 0)
