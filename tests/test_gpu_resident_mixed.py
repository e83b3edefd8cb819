"""GPU parity of the mixed pass 2 of the window-order one-launch MinMax-UInt8 encode
(minmax_resident.hip, quant_mixed): rows 31 and 32 store their on-chip rows (parked in LDS,
held early in VGPRs) in groups of GROUP_ROWS between the turns of the streamed re-read, two
tiles per turn, when a slice holds its whole on-chip part and at least one full streamed tile.

The shapes are derived from the row's geometry and the CU count, as in
test_gpu_resident_window.py: every slice of a chunk but the last has the same whole number of
rows, RE + H + RL on chip, then `nfull` full tiles of SB rows, then a ragged top of one row or
none; the last slice is `short` vectors shorter.  The first LEAD_TURNS turns go before the
first of the NG on-chip groups, the remaining ones are spread over the groups, so

  nfull = 1, 2, 3        one turn of one tile, one of two, two turns (the second of one tile);
                         no turn is left to mix: every on-chip group follows the last tile
  nfull = 2 LEAD_TURNS   as many turns as the lead: still none to mix
  nfull = 2 LEAD_TURNS + 1   one turn (of one tile) past the lead, after the last group
  nfull = NG + 1         8 or 9 turns: the lead in one gap, then a turn every third or fourth
                         group, and one after the last group
  nfull = 2 NG + 1       16 or 17 turns: all but three gaps hold a turn, one follows the last group

each with and without a ragged top, and each with the last slice whole and one vector short
(without a ragged top, the short last slice then has one full tile fewer -- with nfull = 1 none,
which is the unmixed path -- and a ragged top one vector short of a tile).  Every case compares
every byte of the compressed buffer with the C oracle.

Chunks: the one-launch path takes p = 2 only when the chunk size is a multiple of the vector
length (each chunk's payload starts 16-byte aligned, so a chunk that began off a vector
boundary has no common alignment), which leaves every chunk its 96-element scalar head and no
tail; scalar tails come with p = 8 and 76 extra elements, the admissible combination the
window tests use.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_codec import BF16, F32, to_dev
from test_gpu_resident import K, env, gpu_compress, small_threshold  # noqa: F401  (fixtures)
from test_gpu_resident_window import HEAD, NVEC, check, cu_count, elements, geometry, row, shared_input  # noqa: F401

pytestmark = pytest.mark.gpu

MIXED_ROWS = [31, 32]  # the bf16 and the f32 default
GROUP_ROWS = 4         # kMixGroupRows
LEAD_TURNS = 4         # kMixLeadTurns (the shapes below lie on both sides of it)


def groups(K, cfg):
    block, re, h, rl, sb, order = geometry(K, cfg)
    assert order == 2
    return -(-(re + h) // GROUP_ROWS)


def slice_rows(K, cfg, nfull, ragged):
    block, re, h, rl, sb, _ = geometry(K, cfg)
    return re + h + rl + nfull * sb + (1 if ragged else 0)


def nfull_of(K, cfg, name):
    return {"1": 1, "2": 2, "3": 3, "2lead": 2 * LEAD_TURNS, "2lead+1": 2 * LEAD_TURNS + 1,
            "groups+1": groups(K, cfg) + 1, "2groups+1": 2 * groups(K, cfg) + 1}[name]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("tiles", ["1", "2", "3", "2lead", "2lead+1", "groups+1", "2groups+1"])
@pytest.mark.parametrize("cfg", MIXED_ROWS)
def test_mixed_tile_counts(K, oracle_c, row, cfg, tiles, ragged, short, dtype):
    rows = slice_rows(K, cfg, nfull_of(K, cfg, tiles), ragged)
    n = HEAD + elements(K, cfg, dtype, rows, short)
    check(K, oracle_c, shared_input(n, dtype, seed=21), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("target", [-1, 1])
@pytest.mark.parametrize("tiles", ["1", "groups+1"])
@pytest.mark.parametrize("cfg", MIXED_ROWS)
def test_mixed_two_chunks(K, oracle_c, row, cfg, tiles, target, dtype):
    """p = 2, every chunk with a 96-element scalar head (see the module docstring for tails)."""
    p = 2
    rows = slice_rows(K, cfg, nfull_of(K, cfg, tiles), ragged=True)
    cs = elements(K, cfg, dtype, rows, short=1, p=p, extra=HEAD)
    assert cs % NVEC[dtype] == 0
    check(K, oracle_c, shared_input(p * cs, dtype, seed=21), dtype, p, target)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("target", [-1, 1])
@pytest.mark.parametrize("tiles", ["1", "groups+1"])
@pytest.mark.parametrize("cfg", MIXED_ROWS)
def test_mixed_chunks_with_scalar_heads_and_tails(K, oracle_c, row, cfg, tiles, target, dtype):
    p = 8
    rows = slice_rows(K, cfg, nfull_of(K, cfg, tiles), ragged=True)
    cs = elements(K, cfg, dtype, rows, short=1, p=p, extra=76)
    check(K, oracle_c, shared_input(p * cs, dtype, seed=21), dtype, p, target)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cfg", MIXED_ROWS)
def test_mixed_give_up_path(K, oracle_c, env, row, cfg, dtype):
    env["BAGUA_RESIDENT_TIMEOUT_US"] = "0"
    n = HEAD + elements(K, cfg, dtype, slice_rows(K, cfg, 3, ragged=True), short=1)
    check(K, oracle_c, shared_input(n, dtype, seed=21), dtype, 1)


def planted(K, cfg, dtype, infinities):
    """Three full tiles and a ragged top per slice; in slice 1, the first and the last lane of
    an early row, two parked rows and two streamed rows hold NaN, -0 and denormals, and +-inf
    when asked for (they make the chunk's range infinite, so they get a case of their own)."""
    block, re, h, rl, sb, _ = geometry(K, cfg)
    nv = NVEC[dtype]
    rows = slice_rows(K, cfg, 3, ragged=True)
    n = HEAD + elements(K, cfg, dtype, rows, short=1)
    x = shared_input(n, dtype, seed=22).copy()
    if infinities:
        values = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-40, -np.inf, np.inf], np.float32)
    else:
        values = np.array([np.nan, -0.0, 0.0, 1e-40, -1e-40, np.nan, -0.0, 1e-40], np.float32)
    if dtype == BF16:
        values = (values.view(np.uint32) >> 16).astype(np.uint16)
    # an early row, the first and the last parked row, the middle tile's first row and the lowest tile's last row
    for r in (1, re, re + h - 1, re + h + rl + sb, re + h + rl + sb - 1):
        for lane in (0, block - 1):
            first = HEAD + nv * ((1 * rows + r) * block + lane)
            x[first:first + nv] = values[:nv] if lane == 0 else values[-nv:][::-1]
    return x


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("infinities", [False, True])
@pytest.mark.parametrize("cfg", MIXED_ROWS)
def test_mixed_planted_specials(K, oracle_c, row, cfg, infinities, dtype):
    x = planted(K, cfg, dtype, infinities)
    with np.errstate(all="ignore"):
        check(K, oracle_c, x, dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cfg", MIXED_ROWS)
def test_mixed_back_to_back(K, oracle_c, row, cfg, dtype):
    """Two launches on one stream with different inputs (the tag advances on the stream's slot)."""
    n = HEAD + elements(K, cfg, dtype, slice_rows(K, cfg, 3, ragged=True), short=1)
    xs = [shared_input(n, dtype, seed=21), shared_input(n, dtype, seed=22)]
    xts = [to_dev(x, dtype) for x in xs]
    outs = [gpu_compress(K, xt, dtype, 1, -1) for xt in xts]
    torch.cuda.synchronize()
    for x, (out, _) in zip(xs, outs):
        assert np.array_equal(out.cpu().numpy(), oracle_c.compress_minmax_u8(x, dtype, 1))


@pytest.mark.parametrize("dtype,cfg", [(F32, 32), (BF16, 31)])
def test_mixed_default_rows_use_no_scratch(K, dtype, cfg):
    assert K.bagua_minmax_u8_resident_default_cfg(dtype) == cfg
    regs, scratch = ctypes.c_int(-1), ctypes.c_int(-1)
    assert K.bagua_minmax_u8_resident_cfg_info(dtype, cfg, ctypes.byref(regs), ctypes.byref(scratch)) == 0
    print(f"dtype {dtype} row {cfg}: {regs.value} registers, {scratch.value} scratch bytes")
    assert scratch.value == 0, (cfg, scratch.value)
