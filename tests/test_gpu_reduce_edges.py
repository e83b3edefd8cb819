"""reduce.hip at the C ABI on hostile inputs, bit-exact against the C oracle.

(a) bagua_reduce_chunks on both sides of every tree-width step, both averaging finishes,
    the vector and the scalar kernel, the grid cap, NaN / inf / overflow / underflow;
(b) bagua_minmax_u8_decompress_reduce (its first test);
(c) the fused middle step (bagua_minmax_u8_reduce_requantize, _final) at every p <= 16 and on
    the crafted receive buffers of tests/segment_cases.py -- degenerate headers the p x 256
    tables are built from, reduced values the NaN-aware key fold has to survive;
(d) the pieced forms on the same buffers, bagua_minmax_u8_requantize_pieces included;
(e) the runtime-p kernels behind BAGUA_REDUCE_PF=0, in a child process.

tests/test_reduce_edges_cpu.py checks on the CPU that the two oracles agree on every
crafted buffer and that each class produces what it is named for.  Compressed bytes are
compared exactly, floats bit for bit (NaN as NaN-ness); outputs are pre-filled (0xA5 bytes,
7.0 floats) and everything outside the defined output must keep the fill."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import segment_cases as SC
from test_gpu_codec import BF16, F16, F32, STORAGE, TORCH, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
IDS = ["f32", "f16", "bf16"]
VEC_N = {F32: 4, F16: 8, BF16: 8}
PIECES_TAPERED, PIECES_FOLDED, PIECES_TABLES = 0x10000, 0x40000, 0x80000
UNSUPPORTED, INVALID_ARG = 4, 1
ALL_CLASSES = ["benign"] + SC.CLASSES


def seven(dtype):
    return np.full(1, 7.0, np.float32).astype(STORAGE[dtype]) if dtype != BF16 else np.array([0x40E0], np.uint16)


def assert_fill_kept(got: np.ndarray, dtype: int, what: str):
    assert np.all(got.view(STORAGE[dtype]) == seven(dtype)[0]), f"{what}: written outside the defined output"


def filled(n: int, dtype: int) -> torch.Tensor:
    return torch.full((n,), 7.0, dtype=TORCH[dtype], device="cuda")


# ------------------------------------------------------------- (a) plain ----
REDUCE_PS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40]


def reduce_data(kind: str, dtype: int, p: int, cs: int, seed: int) -> np.ndarray:
    from oracle import oracle_np as NP
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((p, cs)).astype(np.float32)
    if kind == "specials":
        big = {F32: 3e38, F16: 6e4, BF16: 3e38}[dtype]
        den = {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}[dtype]  # smallest denormal of T
        last = p - 1
        for base in (0, cs - 80):  # in the vector body and at the end (the ragged tail included)
            v[0, base:base + 8] = np.nan
            v[last, base + 4:base + 12] = np.nan
            v[0, base + 12:base + 20] = np.inf       # +inf and -inf in different chunks, same element
            v[last, base + 16:base + 24] = -np.inf   # (p = 1: -inf wins)
            v[:, base + 24:base + 32] = big          # the sum overflows T
            v[:, base + 32:base + 40] = -big
            v[:, base + 40:base + 72] = 0.0
            v[last, base + 40:base + 48] = -den      # mean underflows to -0 (p >= 2)
            v[0, base + 48:base + 56] = 3 * den      # mean is a denormal, or underflows to +0
            v[:, base + 56:base + 64] = -0.0         # 0.0f + -0 = +0
            v[:, base + 64:base + 72] = den          # sum of denormals
    return NP.from_f32(v.reshape(-1), dtype)


@pytest.mark.parametrize("p", REDUCE_PS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reduce_chunks_vs_oracle(bc, oracle_c, dtype, p):
    """Vector kernel over several workgroups with a partly filled last one, the scalar kernel
    (cs + 1, and the aligned cs on a base pointer one element off), sum and mean, the target
    first / middle / last; N(0,1) and a mix of NaN, +-inf, overflowing and underflowing values.
    Only the target chunk may change."""
    K = bc._native.K
    n = VEC_N[dtype]
    aligned = 2 * 256 * n + 3 * n
    for cs, offset in ((aligned, 0), (aligned + 1, 0), (aligned, 1)):
        for kind in ("normal", "specials"):
            x = reduce_data(kind, dtype, p, cs, seed=1000 * p + cs + dtype)
            for average in (0, 1):
                for target in sorted({0, p // 2, p - 1}):
                    want = oracle_c.reduce_chunks(x.copy(), dtype, p, target, bool(average))
                    xd = to_dev(x, dtype, offset)
                    assert K.bagua_reduce_chunks(dtype, xd.data_ptr(), cs, p, target, average, None) == 0
                    assert_float_bits_equal(to_host(xd, dtype), want, dtype,
                                            f"p={p} cs={cs} offset={offset} {kind} average={average} target={target}")


def test_reduce_chunks_grid_cap(bc, oracle_c):
    """More vectors than 2048 workgroups x 256 lanes: the grid-strided loop sweeps twice."""
    K = bc._native.K
    p, cs = 2, 2048 * 256 * 4 + 4 * 300
    x = reduce_data("normal", F32, p, cs, seed=77)
    x[5], x[cs + 5], x[cs - 1], x[2 * cs - 1] = np.inf, -np.inf, np.nan, 1.0
    for average in (1, 0):
        want = oracle_c.reduce_chunks(x.copy(), F32, p, 1, bool(average))
        xd = to_dev(x, F32)
        assert K.bagua_reduce_chunks(F32, xd.data_ptr(), cs, p, 1, average, None) == 0
        assert_float_bits_equal(to_host(xd, F32), want, F32, f"grid cap average={average}")


# -------------------------------------------- crafted and benign buffers ----
def benign_from_compressor(oracle_c, dtype: int, p: int, cs: int, r: int, seed: int) -> np.ndarray:
    """The alltoall receive buffer of rank r as p compressors produce it, in this module's layout."""
    from oracle import oracle_np as NP
    rng = np.random.default_rng(seed)
    segs = []
    for _ in range(p):
        x = NP.from_f32((rng.standard_normal(p * cs) * 1e-3).astype(np.float32), dtype)
        comp = oracle_c.compress_minmax_u8(x, dtype, p, r)
        cof = comp.size // p
        segs.append(comp[r * cof:r * cof + 32 + cs])
    co = SC.stride(cs)
    buf = np.zeros(p * co, np.uint8)
    for c, s in enumerate(segs):
        buf[c * co:c * co + 32 + cs] = s
    return buf


def hostile_position(p: int) -> int:
    return SC.positions(p)[-2] if len(SC.positions(p)) == 3 else p - 1


# ---------------------------------------------- (b) decompress + reduce ----
@pytest.mark.parametrize("cls", ALL_CLASSES + ["compressor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_decompress_reduce_vs_oracle(bc, oracle_c, dtype, cls):
    K = bc._native.K
    cs = SC.CS
    for p in (2, 5, 9):
        for k in SC.positions(p):
            if cls == "compressor":
                recv = benign_from_compressor(oracle_c, dtype, p, cs, k, seed=p + k)
            else:
                recv = SC.crafted(cls, dtype, p, cs, k)
            recv_d = torch.from_numpy(recv).cuda()
            for average in (0, 1):
                _, red, _ = SC.middle_step(oracle_c, recv, dtype, p, cs, 0, average)
                out = filled(cs + 64, dtype)
                assert K.bagua_minmax_u8_decompress_reduce(dtype, recv_d.data_ptr(), recv.size, cs, p, out.data_ptr(),
                                                           average, None) == 0
                got = to_host(out, dtype)
                what = f"{cls} p={p} k={k} average={average}"
                assert_float_bits_equal(got[:cs], red, dtype, what)
                assert_fill_kept(got[cs:], dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_decompress_reduce_return_codes(bc, dtype):
    K = bc._native.K
    cs = SC.CS
    co = SC.stride(cs)
    recv = torch.zeros(17 * co + 16, dtype=torch.uint8, device="cuda")
    out = filled(cs + 8, dtype)
    f = K.bagua_minmax_u8_decompress_reduce
    assert f(dtype, recv.data_ptr(), 17 * co, cs, 17, out.data_ptr(), 1, None) == UNSUPPORTED  # p > 16
    assert f(dtype, recv.data_ptr(), 2 * co, cs, 2, out[1:].data_ptr(), 1, None) == UNSUPPORTED  # output off 16 B
    assert f(dtype, recv[1:].data_ptr(), 2 * co, cs, 2, out.data_ptr(), 1, None) == UNSUPPORTED  # payloads off N
    assert f(dtype, recv.data_ptr(), 2 * (cs + 31), cs, 2, out.data_ptr(), 1, None) == INVALID_ARG  # input too small
    assert_fill_kept(to_host(out, dtype), dtype, "refused calls")


# ------------------------------------------------- (c) fused middle step ----
MODES = ["store", "none", "final", "final_noseg"]


def run_middle(K, dtype, recv, p, cs, target, average, mode, want, ws, what):
    """One fused middle step in `mode` against want = (reduced chunk, segment, final chunk)."""
    red, seg, final = want
    co = SC.stride(cs)
    S = p * co
    assert recv.size == S and S % p == 0
    recv_d = torch.from_numpy(recv).cuda()
    t_d = filled(p * cs, dtype)
    send_d = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
    if mode.startswith("final"):
        with_seg = mode == "final"
        rc = K.bagua_minmax_u8_reduce_requantize_final(dtype, recv_d.data_ptr(), S, cs, p, t_d.data_ptr(), average,
                                                       send_d.data_ptr() if with_seg else None, S if with_seg else 0,
                                                       target, ws.data_ptr(), ws.numel(), None)
    else:
        rc = K.bagua_minmax_u8_reduce_requantize(dtype, recv_d.data_ptr(), S, cs, p,
                                                 t_d.data_ptr() if mode == "store" else None, average,
                                                 send_d.data_ptr(), S, target, ws.data_ptr(), ws.numel(), None)
    assert rc == 0, f"{what}: status {rc}"
    check_middle_outputs(dtype, p, cs, target, mode, want, to_host(t_d, dtype), send_d.cpu().numpy(), what)
    assert np.array_equal(recv_d.cpu().numpy(), recv), f"{what}: the receive buffer changed"


def check_middle_outputs(dtype, p, cs, target, mode, want, got_t, got_s, what):
    red, seg, final = want
    co = SC.stride(cs)
    own = slice(target * cs, (target + 1) * cs)
    if mode == "store":
        assert_float_bits_equal(got_t[own], red, dtype, f"{what}: reduced chunk")
    elif mode.startswith("final"):
        assert_float_bits_equal(got_t[own], final, dtype, f"{what}: final chunk")
    else:
        assert_fill_kept(got_t[own], dtype, what)
    assert_fill_kept(np.delete(got_t, own), dtype, what)
    if mode == "final_noseg":
        assert np.all(got_s == 0xA5), f"{what}: segment bytes written without an output buffer"
        return
    mine = slice(target * co, (target + 1) * co)
    bad = np.nonzero(got_s[mine] != seg)[0]
    assert bad.size == 0, (f"{what}: {bad.size} segment bytes differ, first at {bad[:5]}: "
                           f"{got_s[mine][bad[:5]]} vs {seg[bad[:5]]}")
    assert np.all(np.delete(got_s, mine) == 0xA5), f"{what}: bytes outside the target segment written"


def oracle_middle(oracle_c, recv, dtype, p, cs, target, average):
    _, red, seg = SC.middle_step(oracle_c, recv, dtype, p, cs, target, average)
    return red, seg, SC.decode_segment(oracle_c, seg, dtype, cs)


@pytest.fixture(scope="module")
def ws(bc):
    return torch.empty(1 << 20, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("p", list(range(1, 17)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_middle_step_every_rank_count(bc, oracle_c, ws, dtype, p):
    """Every p <= 16: the last round of the segment loop is partial whenever p is not a
    multiple of the tree width (clamped duplicate loads on full tiles, the `break`)."""
    K = bc._native.K
    cs = SC.CS
    target = p // 2
    recv = benign_from_compressor(oracle_c, dtype, p, cs, target, seed=31 * p + dtype)
    for average in (0, 1):
        want = oracle_middle(oracle_c, recv, dtype, p, cs, target, average)
        for mode in MODES:
            run_middle(K, dtype, recv, p, cs, target, average, mode, want, ws, f"p={p} average={average} {mode}")


@pytest.mark.parametrize("cls", SC.CLASSES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_middle_step_crafted(bc, oracle_c, ws, dtype, cls):
    K = bc._native.K
    cs = SC.CS
    for p in (2, 3, 5, 8, 9, 16):
        for k in SC.positions(p):
            recv = SC.crafted(cls, dtype, p, cs, k)
            target = (k + 1) % p
            for average in (0, 1):
                want = oracle_middle(oracle_c, recv, dtype, p, cs, target, average)
                for mode in MODES:
                    run_middle(K, dtype, recv, p, cs, target, average, mode, want, ws,
                               f"{cls} p={p} k={k} average={average} {mode}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_middle_step_ragged_tail(bc, oracle_c, ws, dtype):
    """cs + 3: a tail of fewer elements than a 16-B vector, reduced and quantised by workgroup 0's
    scalar path.  The recompute pair takes any chunk size; a stored or final chunk must start
    16-B aligned, which cs + 3 grants the first chunk only: elsewhere BAGUA_ERR_UNSUPPORTED
    (callers run the unfused ops)."""
    K = bc._native.K
    cs, p = SC.CS + 3, 3
    for target in (0, 1):
        recv = benign_from_compressor(oracle_c, dtype, p, cs, target, seed=5 + dtype)
        recv[SC.stride(cs) + 32 + cs - 2] = 255  # the extremes of one segment inside the tail
        recv[SC.stride(cs) + 32 + cs - 1] = 0
        for average in (0, 1):
            want = oracle_middle(oracle_c, recv, dtype, p, cs, target, average)
            for mode in MODES:
                what = f"ragged target={target} average={average} {mode}"
                if mode == "none" or (target * cs * np.dtype(STORAGE[dtype]).itemsize) % 16 == 0:
                    run_middle(K, dtype, recv, p, cs, target, average, mode, want, ws, what)
                    continue
                S = recv.size
                recv_d = torch.from_numpy(recv).cuda()
                t_d = filled(p * cs, dtype)
                send_d = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
                f = (K.bagua_minmax_u8_reduce_requantize if mode == "store"
                     else K.bagua_minmax_u8_reduce_requantize_final)
                assert f(dtype, recv_d.data_ptr(), S, cs, p, t_d.data_ptr(), average, send_d.data_ptr(), S, target,
                         ws.data_ptr(), ws.numel(), None) == UNSUPPORTED, what
                assert_fill_kept(to_host(t_d, dtype), dtype, what)


def test_fused_middle_step_grid_cap(bc, oracle_c, ws):
    """bf16, p = 9 (tree width 8: one vector per lane and tile): more tiles than the 2048
    workgroups, so reduce_tiles sweeps twice; a negative-scale segment in the second round."""
    K = bc._native.K
    dtype, p, cs, target = BF16, 9, 2048 * 256 * 8 + 8 * 300, 4
    recv = SC.crafted("inverted", dtype, p, cs, 8)
    want = oracle_middle(oracle_c, recv, dtype, p, cs, target, 1)
    for mode in ("none", "store", "final"):
        run_middle(K, dtype, recv, p, cs, target, 1, mode, want, ws, f"grid cap {mode}")


# --------------------------------------------------- (d) the pieced forms ----
def piece_ranges(K, cs, schedule):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & 0xFFFF):
        assert K.bagua_minmax_u8_piece_range(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == 0
        out.append((b.value, e.value))
    return out


def run_pieced(K, dtype, recv, p, cs, target, average, schedule, seq, want, what):
    """One pieced sequence: `seq` is "piece" / "pieces" (storing reduce pieces, then
    requantize_piece per piece in reverse order / one requantize_pieces call) or a tuple of
    schedule bits for the recompute pair (reduce_piece(NULL) + reduce_requantize_piece)."""
    co = SC.stride(cs)
    S = p * co
    n = schedule & 0xFFFF
    wsb = K.bagua_minmax_u8_pipeline_workspace_bytes(cs, schedule)
    assert wsb > 0
    pw = torch.full((wsb,), 0xEE, dtype=torch.uint8, device="cuda")
    recv_d = torch.from_numpy(recv).cuda()
    t_d = filled(p * cs, dtype)
    send_d = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
    if seq in ("piece", "pieces"):
        for q in range(n):
            assert K.bagua_minmax_u8_reduce_piece(dtype, recv_d.data_ptr(), S, cs, p, t_d.data_ptr(), average, target,
                                                  schedule, q, pw.data_ptr(), wsb, None) == 0, what
        if seq == "pieces":
            assert K.bagua_minmax_u8_requantize_pieces(dtype, t_d.data_ptr(), cs, p, send_d.data_ptr(), S, target,
                                                       schedule, pw.data_ptr(), wsb, None) == 0, what
        else:
            for q in reversed(range(n)):
                assert K.bagua_minmax_u8_requantize_piece(dtype, t_d.data_ptr(), cs, p, send_d.data_ptr(), S, target,
                                                          schedule, q, pw.data_ptr(), wsb, None) == 0, what
        mode = "store"
    else:
        bits = 0
        for b in seq:
            bits |= b
        red_sched = schedule | (bits & PIECES_TABLES)
        for q in range(n):
            assert K.bagua_minmax_u8_reduce_piece(dtype, recv_d.data_ptr(), S, cs, p, None, average, target, red_sched,
                                                  q, pw.data_ptr(), wsb, None) == 0, what
        if bits & PIECES_FOLDED:
            assert K.bagua_minmax_u8_fold_piece_partials(dtype, cs, schedule, pw.data_ptr(), wsb, None) == 0, what
        for q in reversed(range(n)):
            assert K.bagua_minmax_u8_reduce_requantize_piece(dtype, recv_d.data_ptr(), S, cs, p, average,
                                                             send_d.data_ptr(), S, target, schedule | bits, q,
                                                             pw.data_ptr(), wsb, None) == 0, what
        mode = "none"
    check_middle_outputs(dtype, p, cs, target, mode, want, to_host(t_d, dtype), send_d.cpu().numpy(), what)


PIECED_SEQS = ["piece", "pieces", (), (PIECES_TABLES,), (PIECES_FOLDED,), (PIECES_TABLES, PIECES_FOLDED)]
SCHEDULES = [1, 3, 4, 3 | PIECES_TAPERED, 4 | PIECES_TAPERED]


@pytest.mark.parametrize("cls", ALL_CLASSES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pieced_middle_step_crafted(bc, oracle_c, dtype, cls):
    """TABLES copies piece 0's float tables (NaN entries included) into the later launches;
    FOLDED folds keys that may all be NaN; requantize_pieces must equal the per-piece form."""
    K = bc._native.K
    cs = SC.CS
    for p, average in ((2, 1), (5, 1), (9, 0), (9, 1)):
        k = hostile_position(p)
        recv = SC.crafted(cls, dtype, p, cs, k)
        target = (k + 1) % p
        want = oracle_middle(oracle_c, recv, dtype, p, cs, target, average)
        for schedule in SCHEDULES:
            ranges = piece_ranges(K, cs, schedule)
            assert ranges[0][0] == 0 and ranges[-1][1] == cs
            for seq in PIECED_SEQS:
                run_pieced(K, dtype, recv, p, cs, target, average, schedule, seq, want,
                           f"{cls} p={p} average={average} schedule={schedule:#x} seq={seq}")


# ------------------------------------------------ (e) BAGUA_REDUCE_PF=0 ----
def pf_cases(oracle_c):
    """The p = 2 NULL-tensor cases of (c) and (d) (the only ones the switch reroutes)."""
    cs, p = SC.CS, 2
    for dtype in DTYPES:
        for cls in ALL_CLASSES:
            for k in SC.positions(p):
                recv = SC.crafted(cls, dtype, p, cs, k)
                target = (k + 1) % p
                for average in (0, 1):
                    yield dtype, cls, k, recv, target, average, oracle_middle(oracle_c, recv, dtype, p, cs, target,
                                                                              average)


def run_pf_cases():
    """Body of the child process (tests/reduce_pf_child.py)."""
    import bagua_core
    from oracle import oracle_c
    K = bagua_core._native.K
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    n = 0
    for dtype, cls, k, recv, target, average, want in pf_cases(oracle_c):
        what = f"PF=0 {cls} {SC.NAMES[dtype]} k={k} average={average}"
        run_middle(K, dtype, recv, 2, SC.CS, target, average, "none", want, ws, what)
        for schedule in (1, 3, 4 | PIECES_TAPERED):
            for seq in ((), (PIECES_TABLES, PIECES_FOLDED)):
                run_pieced(K, dtype, recv, 2, SC.CS, target, average, schedule, seq, want,
                           f"{what} {schedule:#x} {seq}")
        n += 1
    return n


def test_runtime_p_kernels_in_child_process(bc):
    """BAGUA_REDUCE_PF is read once per process, so a fresh interpreter runs the p = 2
    recompute cases with the compile-time-p kernels switched off: same bytes as the oracle."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reduce_pf_child.py")
    env = dict(os.environ, BAGUA_REDUCE_PF="0")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime-p cases ok" in r.stdout, r.stdout[-2000:]
