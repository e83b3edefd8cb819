"""GPU parity of the exchange and the ticket of the one-launch MinMax-UInt8 encode
(minmax_resident.hip: draw_ticket / park_tag, publish_partials, sweep_chunk, exchange_minmax).

The exchange is swept by waves 0 and 1 of a workgroup: lane l of wave w polls granules
w * 64 + l + 128 j, j < 4, of its chunk's 2 * bpc (bpc workgroups per chunk, a min and a max
granule each), the four loads in flight together, and folds a granule once, when it first carries
the launch's tag.  The ticket is drawn at kernel entry and becomes the tag in LDS (behind the
first loads in the stack order, at once in the others); every thread reads the tag at the
publish.  With G the CU count, a bucket of p chunks runs bpc = G // p workgroups per chunk and
leaves G - p * bpc idle, so the number of chunks sets how many granules a lane and a wave poll:

  p = 1        2 G granules: all four of every lane of both waves on a 256-CU part
  p = 3, 5     2 bpc no multiple of 64 (a ragged wave; lanes with one or two granules), idle
               workgroups
  p = 8        64 granules on a 256-CU part: one per lane of wave 0, none for wave 1
  p = G // 2   4 granules
  p = G        2 granules, one workgroup per chunk
  target >= 0  every workgroup on one chunk of two

on the f32, bf16 and f16 default rows; the same set with a zero exchange timeout (granules partly
accepted, then fold_missing_slices); 32 back-to-back launches on one slot that alternate two
inputs with their extremes in opposite corner slices and p = 1 / 4 (a granule taken from the
launch before would change the header), then a captured launch replayed 8 times between plain
ones; the minimum in the slice whose granules are polled last (the highest granule index: wave 1,
lanes 62 and 63, the fourth load) with the maximum in slice 0, the reverse, and the extremes
either side of granule G (where the lanes' third loads start), on the f32 default row and on a
row with 256-thread workgroups; with p = 5 an extreme in the last active slice, next to the idle
workgroup; 16 launches on each of two streams at once.

Not covered: sweep_chunk's outer loop takes a second batch of 512 granules only with more than
256 workgroups per chunk, which no 256-CU part launches; "the highest index handled in a second
batch" therefore has no case here.

Every case asserts that the one-launch path is taken (gpu_compress) and compares every byte of
the compressed buffer with the C oracle.  Sizes: the active chunks hold just over 4 Mi elements
(the tests' lowered threshold), so a bucket is 4-5 Mi elements and the target case, whose other
chunk is as large, 8 Mi.  The granule-count cases use chunks that are no whole number of rows per
slice (a partial slice, and empty ones where bpc is large); the planted cases use whole rows, so
that a slice is found by its number.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_codec import BF16, F16, F32, to_dev
from test_gpu_resident import K, env, gpu_compress, make_input, small_threshold  # noqa: F401  (fixtures)
from test_gpu_resident_window import NVEC, check, cu_count, geometry, shared_input

pytestmark = pytest.mark.gpu

MIN_TOTAL = 1 << 22  # the lowered size threshold (small_threshold)
SHORT = 64           # vectors the last slice of a chunk is short: keeps the chunk size a multiple of 128
P_CASES = ["1", "3", "5", "8", "half", "all"]
BLOCK256_ROW = 1     # a row with 256-thread workgroups (four waves, two of them sweeping)


def chunks(case):
    return {"half": cu_count() // 2, "all": cu_count()}.get(case) or int(case)


def layout(K, cfg, dtype, p):
    """(chunk size, vectors per slice) of the smallest bucket of p chunks that takes the
    one-launch path with whole rows per slice, the last one SHORT vectors and the scalar head
    shorter (the planted cases: a slice is found by its number).  The chunk size is a multiple of
    128 elements, which every dtype admits for every chunk (a scalar head of 96, 64, 32 or 0
    elements, by the chunk's payload address)."""
    block = geometry(K, cfg)[0]
    bpc = cu_count() // p
    n = NVEC[dtype]
    rows = 1
    while p * n * (bpc * rows * block - SHORT) < MIN_TOTAL:
        rows += 1
    cs = n * (bpc * rows * block - SHORT)
    assert cs % 128 == 0 and p * cs <= 2 * MIN_TOTAL
    return cs, rows * block


def ragged_chunk(p, nact=None):
    """Chunk size of a bucket of p chunks (nact active) just above the threshold: a multiple of 128
    elements that is no whole number of rows per slice, so that a chunk's slices end in a partial
    one and, where bpc is large, in empty ones."""
    nact = nact or p
    return (MIN_TOTAL // nact + 127) // 128 * 128 + 5 * 128


def default_row(K, dtype):
    return K.bagua_minmax_u8_resident_default_cfg(dtype)


def give_ups(K):
    cnt = ctypes.c_uint64(0)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert K.bagua_minmax_u8_resident_give_ups(sp, ctypes.byref(cnt)) == 0
    return int(cnt.value)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("case", P_CASES)
def test_sweep_granule_counts(K, oracle_c, env, case, dtype):
    env.pop("BAGUA_RESIDENT_CFG", None)
    p = chunks(case)
    check(K, oracle_c, shared_input(p * ragged_chunk(p), dtype, seed=21), dtype, p)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_sweep_every_workgroup_on_the_target_chunk(K, oracle_c, env, dtype):
    env.pop("BAGUA_RESIDENT_CFG", None)
    check(K, oracle_c, shared_input(2 * ragged_chunk(2, nact=1), dtype, seed=21), dtype, 2, target=1)


@pytest.mark.parametrize("case", P_CASES + ["target"])
def test_sweep_give_up_path(K, oracle_c, env, case):
    env.pop("BAGUA_RESIDENT_CFG", None)
    env["BAGUA_RESIDENT_TIMEOUT_US"] = "0"
    p, target = (2, 1) if case == "target" else (chunks(case), -1)
    cs = ragged_chunk(p, nact=1 if target >= 0 else None)
    before = give_ups(K)
    check(K, oracle_c, shared_input(p * cs, F32, seed=21), F32, p, target)
    gave_up = give_ups(K) - before
    print(f"p = {p}, target = {target}: {gave_up} of {cu_count()} workgroups gave up")
    # With every workgroup on one chunk, a workgroup escapes the give-up path only if all the
    # others had published before its first round; the first to finish pass 1 never does, so
    # these two cases are certain to cover it.  (With one workgroup per chunk, p = G, a
    # workgroup needs only its own granules and none gives up; in between it is a matter of
    # timing, so nothing is asserted there.)
    if case in ("1", "target"):
        assert gave_up > 0


def planted(K, cfg, p, plants, seed=22):
    """f32 bucket of p chunks for row cfg with values planted in named slices: plants is a list of
    (chunk, slice, value); a negative slice counts from the chunk's last.  The element lies 133
    elements into the slice's vectors: past any scalar head (< 128 elements, which the chunk's
    last slice owns), inside the slice whatever the head is."""
    cs, per = layout(K, cfg, F32, p)
    bpc = cu_count() // p
    x = shared_input(p * cs, F32, seed).copy()
    assert np.abs(x).max() < 20.0  # make_input's outliers are 3 sigma: the plants below set the range
    for c, b, value in plants:
        b = b % bpc
        i = NVEC[F32] * b * per + 133
        assert i < cs
        x[c * cs + i] = np.float32(value)
    return x


def corner_inputs(K, cfg):
    """Two f32 buckets, run as one chunk and as four, whose minimum and maximum sit in opposite
    corner slices: element 133 is in the first slice of the first chunk (past its scalar head) and
    the fifth element from the end in the last slice of the last chunk, at p = 1 and at p = 4."""
    n = 4 * layout(K, cfg, F32, 4)[0]
    xs = []
    for seed, first, last in ((22, -40.0, 56.0), (23, 48.0, -32.0)):
        x = shared_input(n, F32, seed).copy()
        assert np.abs(x).max() < 20.0
        x[133], x[n - 5] = np.float32(first), np.float32(last)
        xs.append(x)
    return n, xs


def launch(K, xt, p, st, target=-1):
    with torch.cuda.stream(st):  # gpu_compress fills its output buffer on the current stream
        out, keep = gpu_compress(K, xt, F32, p, target, stream=st)
    return out, keep


def test_stale_tags_back_to_back_and_graph_replays(K, oracle_c, env):
    env.pop("BAGUA_RESIDENT_CFG", None)
    cfg = default_row(K, F32)
    n, xs = corner_inputs(K, cfg)
    want = {(i, p): oracle_c.compress_minmax_u8(xs[i], F32, p) for i in (0, 1) for p in (1, 4)}
    assert not np.array_equal(want[0, 1][:32], want[1, 1][:32]), "the two inputs' headers differ"
    st = torch.cuda.Stream()
    xts = [to_dev(x, F32) for x in xs]
    st.wait_stream(torch.cuda.current_stream())
    outs = []
    for k in range(32):
        i, p = k % 2, (1, 4)[(k // 2) % 2]
        out, keep = launch(K, xts[i], p, st)
        outs.append((i, p, out, keep))
    torch.cuda.synchronize()
    for k, (i, p, out, _) in enumerate(outs):
        assert np.array_equal(out.cpu().numpy(), want[i, p]), f"launch {k} (input {i}, p = {p})"

    # one captured launch (p = 1) on the same stream's slot, replayed 8 times on alternating
    # inputs with a plain launch of the other input after each
    sp = ctypes.c_void_p(st.cuda_stream)
    S = K.bagua_minmax_u8_compressed_bytes(F32, n, 1)
    wsb = K.bagua_minmax_u8_workspace_bytes(n, 1)
    with torch.cuda.stream(st):
        xg = xts[0].clone()
        og = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    args = (F32, xg.data_ptr(), n, n, 1, og.data_ptr(), S, ws.data_ptr(), wsb, -1, sp)
    assert K.bagua_minmax_u8_resident_path(F32, xg.data_ptr(), n, n, 1, og.data_ptr(), S, -1, sp) == 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        rc = K.bagua_minmax_u8_compress(*args)
    assert rc == 0
    got = []
    for k in range(8):
        i = k % 2
        with torch.cuda.stream(st):
            xg.copy_(xts[i])
            og.fill_(0xA5)
            g.replay()
            got.append((i, 1, og.clone(), None))
        out, keep = launch(K, xts[1 - i], 4 if k % 4 < 2 else 1, st)
        got.append((1 - i, 4 if k % 4 < 2 else 1, out, keep))
    torch.cuda.synchronize()
    for k, (i, p, out, _) in enumerate(got):
        assert np.array_equal(out.cpu().numpy(), want[i, p]), f"replay phase, launch {k} (input {i}, p = {p})"
    assert K.bagua_minmax_u8_release_stream(sp) == 0


@pytest.mark.parametrize("where", ["min_last_max_first", "max_last_min_first", "min_at_granule_G", "max_at_granule_G"])
@pytest.mark.parametrize("row", ["default", "block256"])
def test_extremes_in_the_corner_granules(K, oracle_c, env, row, where):
    """p = 1: the extremes in the slices whose granules have the lowest and the highest index
    (lanes 0 and 1 of wave 0, first load; lanes 62 and 63 of wave 1, fourth load), and either side
    of granule G (slice G / 2: lanes 0 and 1 of wave 0, third load on a 256-CU part) -- every other
    value is at least a factor 2 inside the range."""
    if row == "block256":
        env["BAGUA_RESIDENT_CFG"] = str(BLOCK256_ROW)
        cfg = BLOCK256_ROW
        assert geometry(K, cfg)[0] == 256
    else:
        env.pop("BAGUA_RESIDENT_CFG", None)
        cfg = default_row(K, F32)
    half = cu_count() // 2  # granules 2 * half, 2 * half + 1: the first of the upper half
    plants = {"min_last_max_first": [(0, -1, -40.0), (0, 0, 56.0)],
              "max_last_min_first": [(0, -1, 56.0), (0, 0, -40.0)],
              "min_at_granule_G": [(0, half, -40.0), (0, half - 1, 56.0)],
              "max_at_granule_G": [(0, -1, -40.0), (0, half, 56.0)]}[where]
    check(K, oracle_c, planted(K, cfg, 1, plants), F32, 1)


@pytest.mark.parametrize("value", [-40.0, 56.0])
def test_extreme_next_to_the_idle_workgroup(K, oracle_c, env, value):
    """p = 5: the last active slice (the last chunk's last) holds the bucket's extreme; the
    workgroups after it are idle (none where the CU count is a multiple of 5)."""
    env.pop("BAGUA_RESIDENT_CFG", None)
    cfg = default_row(K, F32)
    check(K, oracle_c, planted(K, cfg, 5, [(4, -1, value), (4, 0, -value / 2), (0, -1, value / 4)]), F32, 5)


def test_two_streams_sixteen_launches_each(K, oracle_c, env):
    """Each stream has its own slot; the two streams' launches overlap (both want every CU, so a
    launch may also take the bounded-wait path)."""
    env.pop("BAGUA_RESIDENT_CFG", None)
    cfg = default_row(K, F32)
    n, xs = corner_inputs(K, cfg)
    want = {(i, p): oracle_c.compress_minmax_u8(xs[i], F32, p) for i in (0, 1) for p in (1, 4)}
    xts = [to_dev(x, F32) for x in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    outs = []
    for k in range(16):
        for j, st in enumerate(streams):
            i, p = (k + j) % 2, (1, 4)[((k // 2) + j) % 2]
            out, keep = launch(K, xts[i], p, st)
            outs.append((i, p, out, keep))
    torch.cuda.synchronize()
    for k, (i, p, out, _) in enumerate(outs):
        assert np.array_equal(out.cpu().numpy(), want[i, p]), f"launch {k} (input {i}, p = {p})"
    for st in streams:
        assert K.bagua_minmax_u8_release_stream(ctypes.c_void_p(st.cuda_stream)) == 0
