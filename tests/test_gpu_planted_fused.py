"""Planted extrema through the min/max passes that do not read a tensor the
caller wrote: the fused dequantise+reduce partials with their per-piece slots
and the fold (reduce.hip, minmax_u8.hip), the ring mix's partials and the
one-rank ring op (decentralized.hip), and the 1-bit codec's |x| tile partials
and scale tree (onebit.hip, onebit_ef.hip) with a planted mass.

Fused reduce: benign headers, payload bytes in [64, 191], byte 255 at the
planted maximum and byte 0 at the planted minimum in every segment, so the
reduced extremum is unique for any p; the self-check of tests/planted_cases.py
runs on the reference's reduced chunk (segment_cases.middle_step), which is
also what every entry point is compared with.  A 5-piece schedule with an empty
trailing piece does not exist at cs = segment_cases.CS (5 pieces of 3584
elements leave the last one 2344); 12 pieces have one and are used instead.
"""
import ctypes

import numpy as np
import pytest
import torch

import planted_cases as PC
import segment_cases as SC
from test_gpu_codec import BF16, F16, F32, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401
from test_gpu_reduce_edges import (MODES, PIECED_SEQS, PIECES_TAPERED, oracle_middle, piece_ranges, run_middle,
                                   run_pieced, ws)  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
IDS = ["f32", "f16", "bf16"]
RANKS = [1, 2, 3, 5, 9, 16]  # tree widths 2, 4 and 8


def planted_middle(oracle_c, dtype, base, target, average, names, pos):
    """(receive buffer, oracle's (reduced, segment, final), plants), self-checked"""
    p, cs = base.shape
    plants = [PC.Plant(0, pos[names[0]], "min", names[0]), PC.Plant(0, pos[names[1]], "max", names[1])]
    recv = PC.planted_received(SC.build_received, dtype, base, plants[0].index, plants[1].index)
    want = oracle_middle(oracle_c, recv, dtype, p, cs, target, average)
    return recv, want, plants


def reduced_base(oracle_c, dtype, base, target, average):
    p, cs = base.shape
    recv = PC.planted_received(SC.build_received, dtype, base, -1, -1)
    return SC.middle_step(oracle_c, recv, dtype, p, cs, target, average)[1]


@pytest.mark.parametrize("p", RANKS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_middle_step_sees_every_region(bc, oracle_c, ws, dtype, p):
    """bagua_minmax_u8_reduce_requantize with a tensor and with tensor = NULL, and _final with
    and without a segment, sum and mean"""
    K = bc._native.K
    cs, target = SC.CS, p // 2
    base = PC.received_base(p, cs, seed=100 * p + dtype)
    pos = PC.fused_positions(dtype, p, cs)
    assert sum(n.endswith("_last_element") for n in pos) >= 2 and "sub_tile_remainder_middle" in pos
    for average in (0, 1):
        rb = reduced_base(oracle_c, dtype, base, target, average)
        for names in PC.rotate_pairs(pos):
            recv, want, plants = planted_middle(oracle_c, dtype, base, target, average, names, pos)
            PC.check_plants(want[0], rb, dtype, 1, plants)
            for mode in MODES:
                run_middle(K, dtype, recv, p, cs, target, average, mode, want, ws,
                           f"p={p} average={average} {mode}, planted {plants[0]}, {plants[1]}")


SCHEDULES = [4, 4 | PIECES_TAPERED, 12]


@pytest.mark.parametrize("schedule", SCHEDULES, ids=["4_pieces", "4_tapered", "12_pieces_last_empty"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pieced_middle_step_sees_every_region(bc, oracle_c, dtype, schedule):
    """reduce_piece (storing and NULL) + requantize_pieces / requantize_piece /
    reduce_requantize_piece, with and without the folded partial and the shared tables: the
    header must not depend on the piece that holds the extremum"""
    K = bc._native.K
    cs = SC.CS
    ranges = piece_ranges(K, cs, schedule)
    assert ranges[0][0] == 0 and max(e for _, e in ranges) == cs
    if schedule == 12:
        assert ranges[-1][0] == ranges[-1][1], "the trailing piece is not empty"
    pos = PC.piece_positions(ranges)
    assert len([n for n in pos if n.startswith("piece")]) == 2 * (sum(e > b for b, e in ranges) - 1)
    pairs = PC.rotate_pairs(pos)
    for p in RANKS:
        target = p - 1
        base = PC.received_base(p, cs, seed=7 * p + dtype)
        for average in (0, 1):
            rb = reduced_base(oracle_c, dtype, base, target, average)
            for names in pairs:
                recv, want, plants = planted_middle(oracle_c, dtype, base, target, average, names, pos)
                PC.check_plants(want[0], rb, dtype, 1, plants)
                for seq in PIECED_SEQS:
                    run_pieced(K, dtype, recv, p, cs, target, average, schedule, seq, want,
                               f"p={p} average={average} schedule={schedule:#x} seq={seq}, "
                               f"planted {plants[0]}, {plants[1]}")


# ------------------------------------------------------------ ring mix ----
RING_N = (1 << 18) + 37
MIX_SHAPES = [{"BAGUA_RING_MIX_TILES": "1"}, {"BAGUA_RING_MIX_TILES": "0"}, {"BAGUA_RING_MIX_CONTIG": "1"}]
ONE_RANK_SHAPES = [{"BAGUA_RING_ONE_RANK_MIX_CFG": str(c)} for c in range(5)]


def ring_inputs(dtype, kind, names, pos, seed):
    """l, r, w within 1e-3; t the kind's base with its minimum and maximum planted"""
    from oracle import oracle_np as NP
    rng = np.random.default_rng(seed)
    a = {k: NP.from_f32(rng.uniform(-1e-3, 1e-3, RING_N).astype(np.float32), dtype) for k in "wlr"}
    plants = [PC.Plant(0, pos[names[0]], "min", names[0]), PC.Plant(0, pos[names[1]], "max", names[1])]
    a["t"], tb = PC.build(dtype, kind, 1, RING_N, plants, seed=seed)
    return a, tb, plants


def mixed(oracle_c, t, a, dtype):
    """the oracle's addmul sequence of the op (decentralized_low_precision_synchronous.rs:45-64)"""
    m = t.copy()
    oracle_c.addmul_inplace(m, a["l"], dtype, float(np.float32(1.0 / 3.0)))
    oracle_c.addmul_inplace(m, a["r"], dtype, float(np.float32(1.0 / 3.0)))
    oracle_c.addmul_inplace(m, a["w"], dtype, float(np.float32(-5.0 / 3.0)))
    return m


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ring_mix_sees_every_region(bc, oracle_c, monkeypatch, dtype):
    """bagua_ring_mix_minmax + stage 2, and bagua_ring_one_rank_minmax, in every launch shape:
    the extrema of the MIXED tensor in the first vector, either side of a tile edge, the last
    full vector and every element of the ragged tail"""
    from oracle import simulate
    N, K = bc._native, bc._native.K
    n = RING_N
    pos = PC.ring_positions(dtype, n)
    assert sum(nm.startswith("ragged_tail") for nm in pos) == n % PC.vec_n(dtype) > 0
    wsb = K.bagua_minmax_u8_workspace_bytes(n, 1)
    wsd = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    S = K.bagua_minmax_u8_compressed_bytes(dtype, n, 1)
    for i, names in enumerate(PC.rotate_pairs(pos)):
        a, tb, plants = ring_inputs(dtype, "margin", names, pos, seed=dtype + 1)
        m = mixed(oracle_c, a["t"], a, dtype)
        PC.check_plants(m, mixed(oracle_c, tb, a, dtype), dtype, 1, plants)  # the self-check, on the mixed values
        want_comp = oracle_c.compress_minmax_u8(m, dtype, 1)
        want_op = simulate.decentralized_low_precision(oracle_c, [a["t"]], [a["w"]], [a["l"]], [a["r"]], dtype)
        what = f"{PC.DTYPE_NAME[dtype]} planted {plants[0]}, {plants[1]}"
        for shape in MIX_SHAPES:
            with monkeypatch.context() as mp:
                for k, v in shape.items():
                    mp.setenv(k, v)
                d = {k: to_dev(a[k], dtype) for k in "twlr"}
                out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
                N.check(K.bagua_ring_mix_minmax(dtype, d["t"].data_ptr(), d["l"].data_ptr(), d["r"].data_ptr(),
                                                d["w"].data_ptr(), n, wsd.data_ptr(), wsb, None), "mix")
                N.check(K.bagua_minmax_u8_compress_stage(2, dtype, d["t"].data_ptr(), n, n, 1, out.data_ptr(), S,
                                                         wsd.data_ptr(), wsb, -1, None), "stage 2")
                got = out.cpu().numpy()
                PC.assert_headers(got, want_comp, dtype, 1, plants, f"mix {shape} {what}")
                assert np.array_equal(got, want_comp), f"mix {shape} {what}"
                assert_float_bits_equal(to_host(d["t"], dtype), m, dtype, f"mixed tensor {shape} {what}")
        for shape in ONE_RANK_SHAPES:
            with monkeypatch.context() as mp:
                for k, v in shape.items():
                    mp.setenv(k, v)
                d = {k: to_dev(a[k], dtype) for k in "twlr"}
                N.check(K.bagua_ring_one_rank_minmax(dtype, d["t"].data_ptr(), d["w"].data_ptr(), d["l"].data_ptr(),
                                                     d["r"].data_ptr(), n, wsd.data_ptr(), wsb, None), "one-rank ring op")
                for k, wk in zip("twlr", want_op):
                    assert_float_bits_equal(to_host(d[k], dtype), wk[0], dtype, f"one-rank ring op {k} {shape} {what}")


# -------------------------------------------------- 1-bit planted mass ----
OB_P, OB_CS, OB_PIECES = 3, 1024 * 1030 + 7, 4


def onebit_tile_ranges(K, cs, pieces):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(pieces):
        assert K.bagua_onebit_piece_range(cs, pieces, q, ctypes.byref(b), ctypes.byref(e)) == 0
        out.append((b.value, e.value))
    return out


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_onebit_planted_mass_reaches_the_scale(bc, oracle_c, dtype):
    """Every element +-0 but one 1.0 per chunk: bagua_onebit_compress, encode_range per piece +
    finalize, and compress_ef from a zero state must all carry it to the header's scale."""
    import onebit_ef_reference as EF
    K = bc._native.K
    p, cs = OB_P, OB_CS
    ranges = onebit_tile_ranges(K, cs, OB_PIECES)
    pos = PC.onebit_positions(cs, ranges)
    names = list(pos)
    S = K.bagua_onebit_compressed_bytes(cs, p)
    wsb = K.bagua_onebit_workspace_bytes(cs, p)
    wsd = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for i in range(0, len(names), p):
        mine = [names[(i + c) % len(names)] for c in range(p)]
        x = PC.planted_mass(dtype, p, cs, [pos[nm] for nm in mine], seed=i + dtype)
        want = oracle_c.compress_onebit(x, dtype, p)
        PC.check_mass(want, p, mine)
        what = f"{PC.DTYPE_NAME[dtype]} 1.0 planted at {mine} (chunks 0..{p - 1})"
        xt = to_dev(x, dtype)
        out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
        assert K.bagua_onebit_compress(dtype, xt.data_ptr(), p * cs, cs, p, out.data_ptr(), S, wsd.data_ptr(), wsb, -1,
                                       None) == 0
        got = out.cpu().numpy()
        for c in range(p):  # the headers (scale, count) first
            assert np.array_equal(got[c * (S // p):c * (S // p) + 8], want[c * (S // p):c * (S // p) + 8]), \
                f"compress header of chunk {c}, {what}"
        assert np.array_equal(got, want), f"compress, {what}"
        out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
        for tb, te in reversed(ranges):
            assert K.bagua_onebit_encode_range(dtype, xt.data_ptr(), p * cs, cs, p, out.data_ptr(), S, wsd.data_ptr(),
                                               wsb, tb, te, None) == 0
        assert K.bagua_onebit_finalize(wsd.data_ptr(), wsb, p * cs, cs, p, out.data_ptr(), S, None) == 0
        assert np.array_equal(out.cpu().numpy(), want), f"encode_range + finalize, {what}"
        st = EF.WorkerState(p * cs, p)
        want_ef = EF.compress_ef(oracle_c, x, dtype, p, st)
        PC.check_mass(want_ef, p, mine)
        carry = torch.zeros(p * cs, dtype=torch.float32, device="cuda")
        scales = torch.zeros(p, dtype=torch.float32, device="cuda")
        out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
        assert K.bagua_onebit_compress_ef(dtype, xt.data_ptr(), p * cs, cs, p, out.data_ptr(), S, wsd.data_ptr(), wsb,
                                          -1, carry.data_ptr(), scales.data_ptr(), None) == 0
        assert np.array_equal(out.cpu().numpy(), want_ef), f"compress_ef, {what}"
        assert np.array_equal(scales.cpu().numpy().view(np.uint32), st.scales.view(np.uint32)), f"ef scales, {what}"
        assert np.array_equal(carry.cpu().numpy().view(np.uint32), st.carry.view(np.uint32)), f"ef carry, {what}"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_onebit_one_rank_planted_mass(bc, oracle_c, dtype):
    """bagua_onebit_centralized_one_rank on one chunk of the same shape, the op sequence at
    p = 1 as the expected value (test_onebit_one_rank_op_matches_sequence)"""
    from oracle import simulate
    K = bc._native.K
    n = OB_CS
    pos = PC.onebit_positions(n, onebit_tile_ranges(K, n, OB_PIECES))
    wsb = K.bagua_onebit_one_rank_workspace_bytes(n)
    wsd = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for i, (name, idx) in enumerate(pos.items()):
        x = PC.planted_mass(dtype, 1, n, [idx], seed=i)
        PC.check_mass(oracle_c.compress_onebit(x, dtype, 1), 1, [name])
        average = i & 1
        want = simulate.centralized_low_precision(oracle_c, [x.copy()], dtype, bool(average), method="OneBitSignScale")[0]
        xt = to_dev(x, dtype)
        assert K.bagua_onebit_centralized_one_rank(dtype, xt.data_ptr(), n, average, wsd.data_ptr(), wsb, None) == 0
        assert_float_bits_equal(to_host(xt, dtype), want, dtype, f"1-bit one-rank op, 1.0 planted at {name}")
