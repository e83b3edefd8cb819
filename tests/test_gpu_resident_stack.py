"""GPU parity of the stack-order rows of the one-launch MinMax-UInt8 encode
(minmax_resident.hip, minmax_resident_encode_kernel_stack).

A slice of a chunk is rows of BLOCK vectors: rows [0, R) are held in VGPRs,
rows [R, R + H) parked in LDS, the rest streamed in tiles of SB rows with a
ragged top tile.  The shapes here are derived from the row's R, H, BLOCK and SB
(bagua_minmax_u8_resident_cfg_geometry) and the CU count G, so that every
region edge is crossed; every case compares every byte of the compressed
buffer with the C oracle.

  a  slices shorter than R rows (2^22 elements, p = 1)
  b  slices of exactly R + H rows: no streamed part
  c  R + H rows, one full streamed tile and a ragged tile of 3 rows, the last
     slice a few vectors short: the smallest bucket that runs all three regions
     and the ragged top
  d  c split into p = 8 chunks (all), p = 4 chunks (target 2) and p = 3 chunks,
     with scalar heads and tails
  e  c with NaN, +-0 and denormal inputs
  f  c with a zero exchange timeout (the give-up path)
  g  back-to-back launches on one stream, and one launch on each of two streams
  h  no default row uses scratch (bagua_minmax_u8_resident_cfg_info)
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_codec import BF16, F16, F32, to_dev
from test_gpu_resident import K, env, gpu_compress, make_input, small_threshold  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NVEC = {F32: 4, F16: 8, BF16: 8}  # elements per 16-byte vector
# the stack-order row a dtype's tests select when its default row is not one
FALLBACK_ROW = {F32: 24, F16: 29, BF16: 18}


def geometry(K, cfg):
    v = [ctypes.c_int(0) for _ in range(5)]
    assert K.bagua_minmax_u8_resident_cfg_geometry(cfg, *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)  # block, r, h, sb, stack


def stack_row(K, dtype):
    """(cfg, block, r, h, sb) of the stack-order row under test: the dtype's default row."""
    cfg = K.bagua_minmax_u8_resident_default_cfg(dtype)
    if geometry(K, cfg)[4] == 0:
        cfg = FALLBACK_ROW[dtype]
    block, r, h, sb, stack = geometry(K, cfg)
    assert stack != 0, cfg
    return cfg, block, r, h, sb


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


_inputs = {}


def shared_input(n, dtype, seed, specials=False):
    """One host array per (dtype, seed, specials), generated once at the largest size asked for
    so far; shorter cases take a prefix.  Never written to."""
    key = (dtype, seed, specials)
    if key not in _inputs or _inputs[key].size < n:
        _inputs[key] = make_input(n, dtype, seed, specials)
    return _inputs[key][:n]


def chunk_elements(K, dtype, bpc, rows, short_vectors=0, extra=0):
    """Elements of a chunk whose bpc slices have `rows` rows each, the last one
    `short_vectors` (+ the chunk's scalar head) vectors short, plus `extra` elements."""
    block = stack_row(K, dtype)[1]
    return NVEC[dtype] * (bpc * rows * block - short_vectors) + extra


def check(K, oracle_c, x, dtype, p, target=-1):
    xt = to_dev(x, dtype)
    got_t, _ = gpu_compress(K, xt, dtype, p, target)
    torch.cuda.synchronize()
    got = got_t.cpu().numpy()
    want = oracle_c.compress_minmax_u8(x, dtype, p, target)
    if target >= 0:
        co = got.size // p
        got, want = got[target * co:(target + 1) * co], want[target * co:(target + 1) * co]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"


def case_c_elements(K, dtype, p=1, extra=3):
    """Case c for p chunks: per slice R + H + SB + 3 rows; the head of a chunk (< 128 elements + one
    vector) and 40 vectors come off the last slice, which stays inside the ragged top tile."""
    _, block, r, h, sb = stack_row(K, dtype)
    bpc = cu_count() // p
    return chunk_elements(K, dtype, bpc, r + h + sb + 3, short_vectors=40, extra=extra)


@pytest.fixture
def row(K, env, request):
    dtype = request.node.callspec.params["dtype"]
    cfg = stack_row(K, dtype)[0]
    env["BAGUA_RESIDENT_CFG"] = str(cfg)
    return cfg


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_stack_slices_shorter_than_held_rows(K, oracle_c, row, dtype):
    _, block, r, h, sb = stack_row(K, dtype)
    n = 1 << 22
    assert n // NVEC[dtype] // cu_count() < r * block
    check(K, oracle_c, shared_input(n, dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_stack_slices_of_exactly_the_on_chip_rows(K, oracle_c, row, dtype):
    """Every slice is R + H whole rows (the 96-element head of the chunk is scalar): nothing is streamed."""
    _, block, r, h, sb = stack_row(K, dtype)
    n = 96 + chunk_elements(K, dtype, cu_count(), r + h)
    check(K, oracle_c, shared_input(n, dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_stack_all_regions_and_ragged_top(K, oracle_c, row, dtype):
    check(K, oracle_c, shared_input(case_c_elements(K, dtype), dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("p,target,extra", [(8, -1, 76), (4, 2, 76), (3, -1, 77)])
def test_stack_chunks_with_scalar_heads_and_tails(K, oracle_c, row, dtype, p, target, extra):
    """Case c per chunk.  The one-launch encode needs the input and the payload of every
    active chunk to share a vector alignment; the segment stride is chunk_size + 32 + padding
    / p, which for p = 8 and p = 4 rules out every odd chunk size (the two-kernel encode takes
    those), so these two add 76 elements: every chunk has a scalar head, and the 16-bit chunks
    of even index a scalar tail.  With p = 3 (one idle workgroup) + 77 is admissible, and every
    chunk of either dtype has a scalar head and tail."""
    cs = case_c_elements(K, dtype, p, extra=extra)
    check(K, oracle_c, shared_input(p * cs, dtype, seed=11), dtype, p, target)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_stack_specials(K, oracle_c, row, dtype):
    check(K, oracle_c, shared_input(case_c_elements(K, dtype), dtype, seed=12, specials=True), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_stack_give_up_path(K, oracle_c, env, row, dtype):
    env["BAGUA_RESIDENT_TIMEOUT_US"] = "0"
    check(K, oracle_c, shared_input(case_c_elements(K, dtype), dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_stack_back_to_back_and_two_streams(K, oracle_c, row, dtype):
    n = case_c_elements(K, dtype)
    xs = [shared_input(n, dtype, seed=11), shared_input(n, dtype, seed=13)]
    xts = [to_dev(x, dtype) for x in xs]
    s1, s2 = torch.cuda.current_stream(), torch.cuda.Stream()
    s2.wait_stream(s1)  # the inputs were copied on s1
    outs = []
    # two launches back to back on s1 (tags advance on its slot), then one launch on each
    # of two streams (separate slots); gpu_compress fills its output buffer on the current
    # stream, so each launch is issued with its own stream current
    for i, st in ((0, s1), (1, s1), (0, s1), (1, s2)):
        with torch.cuda.stream(st):
            out, keep = gpu_compress(K, xts[i], dtype, 1, -1, stream=st)
        outs.append((i, out, keep))
    torch.cuda.synchronize()
    want = [oracle_c.compress_minmax_u8(x, dtype, 1) for x in xs]
    for i, out, _ in outs:
        assert np.array_equal(out.cpu().numpy(), want[i])


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_default_rows_use_no_scratch(K, dtype):
    regs, scratch = ctypes.c_int(-1), ctypes.c_int(-1)
    for cfg in (-1, K.bagua_minmax_u8_resident_default_cfg(dtype), stack_row(K, dtype)[0]):
        assert K.bagua_minmax_u8_resident_cfg_info(dtype, cfg, ctypes.byref(regs), ctypes.byref(scratch)) == 0
        print(f"dtype {dtype} cfg {cfg}: {regs.value} registers, {scratch.value} scratch bytes")
        assert 0 < regs.value <= 512
        assert scratch.value == 0, (cfg, scratch.value)
