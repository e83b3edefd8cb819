"""decentralized.hip at the C ABI: the ring mix and apply passes against the oracle's
elementwise restatement of the reference op (decentralized_low_precision_synchronous.rs:45-64,
126-151), written out per step:
    mix:   t += L * 1/3;  t += R * 1/3;  t += W * -5/3;  compress(t)
    apply: L += dq(from_left);  R += dq(from_right);  t = dq(mine) + W;  W = t
`mine`, `from_left` and `from_right` are three different segments with different (and
degenerate) headers, so a kernel that swaps two of them cannot pass; every
BAGUA_RING_APPLY_CFG row runs, and the range form is checked piece by piece."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import segment_cases as SC
from test_gpu_codec import BF16, F16, F32, STORAGE, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401
from test_gpu_ring_one_rank import CASES, inputs

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
IDS = ["f32", "f16", "bf16"]
VEC_N = {F32: 4, F16: 8, BF16: 8}
N_RAGGED = (1 << 18) + 37
N_CAP = 1024 * 256 * 8 * 2 + 8 * 11 + 3  # bf16: more vectors than 1024 workgroups x 256 lanes x 4
UNSUPPORTED, INVALID_ARG = 4, 1
APPLY_ROWS = 23
SEGMENT_CLASSES = ["nan_both", "both_inf", "empty_init", "constant", "inverted", "benign"]
# (mine, from_left, from_right): every class in every role
TRIPLES = [tuple(SEGMENT_CLASSES[(i + j) % 6] for j in range(3)) for i in range(6)]


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k in self.kv:
            del os.environ[k]


def one_segment_buffer(cls: str, dtype: int, n: int, seed: int) -> np.ndarray:
    """A one-chunk MinMax buffer (32 + n bytes, zero slack to a multiple of 32)."""
    rng = np.random.default_rng([seed, SEGMENT_CLASSES.index(cls), dtype])
    return SC.build_received(dtype, n, [SC.one_segment(cls, dtype, n, rng)])


def tensors(dtype: int, n: int, seed: int) -> dict:
    from oracle import oracle_np as NP
    rng = np.random.default_rng(seed)
    a = {k: NP.from_f32((rng.standard_normal(n) * 1e-3).astype(np.float32), dtype) for k in "twlr"}
    a["w"][:8] = NP.from_f32(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 6e4, -6e4, 1.0], np.float32), dtype)
    a["l"][8:12] = NP.from_f32(np.array([np.inf, -np.inf, np.nan, -0.0], np.float32), dtype)
    return a


def oracle_apply(oracle_c, dtype, bufs, a):
    """-> (t, w, l, r) after the apply step; bufs = (mine, from_left, from_right)."""
    n = a["t"].size
    dq = [oracle_c.decompress_minmax_u8(b, 1, np.zeros(n, STORAGE[dtype]), dtype) for b in bufs]
    left = oracle_c.add_inplace(a["l"].copy(), dq[1], dtype)
    right = oracle_c.add_inplace(a["r"].copy(), dq[2], dtype)
    t = oracle_c.add_inplace(dq[0].copy(), a["w"], dtype)
    return {"t": t, "w": t.copy(), "l": left, "r": right}


@functools.lru_cache(maxsize=None)
def apply_case(dtype: int, triple: tuple, n: int):
    from oracle import oracle_c
    bufs = tuple(one_segment_buffer(c, dtype, n, seed=i) for i, c in enumerate(triple))
    a = tensors(dtype, n, seed=n + dtype)
    return bufs, a, oracle_apply(oracle_c, dtype, bufs, a)


def run_apply(K, dtype, bufs, a, n, e0=None, e1=None):
    bd = [torch.from_numpy(b).cuda() for b in bufs]
    d = {k: to_dev(a[k], dtype) for k in "twlr"}
    args = (dtype, bd[0].data_ptr(), bd[1].data_ptr(), bd[2].data_ptr(), bufs[0].size, n)
    tail = (d["t"].data_ptr(), d["w"].data_ptr(), d["l"].data_ptr(), d["r"].data_ptr(), None)
    if e0 is None:
        rc = K.bagua_ring_apply_minmax(*args, *tail)
    else:
        rc = K.bagua_ring_apply_minmax_range(*args, e0, e1, *tail)
    return rc, d, bd


def check_apply(dtype, d, bd, bufs, want, what):
    for k in "twlr":
        assert_float_bits_equal(to_host(d[k], dtype), want[k], dtype, f"{what}: {k}")
    for b, h, name in zip(bd, bufs, ("mine", "from_left", "from_right")):
        assert np.array_equal(b.cpu().numpy(), h), f"{what}: {name} changed"


# ------------------------------------------------------------------ mix ----
MIX_SHAPES = [{}, {"BAGUA_RING_MIX_TILES": "0"}, {"BAGUA_RING_MIX_NTS": "1"},
              {"BAGUA_RING_MIX_TILES": "0", "BAGUA_RING_MIX_CONTIG": "1"}]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ring_mix_then_quantise_vs_oracle(bc, oracle_c, dtype, case):
    """bagua_ring_mix_minmax + stage 2 of bagua_minmax_u8_compress_stage (n_chunks = 1) == the three
    addmuls + compress: the mixed tensor, every compressed byte, L / R / W unchanged."""
    K = bc._native.K
    f13, f53 = float(np.float32(1.0 / 3.0)), float(np.float32(-5.0 / 3.0))
    for n in (5, N_RAGGED):
        a = inputs(case, n, dtype, seed=n + 5 * dtype + len(case))
        mixed = a["t"].copy()
        oracle_c.addmul_inplace(mixed, a["l"], dtype, f13)
        oracle_c.addmul_inplace(mixed, a["r"], dtype, f13)
        oracle_c.addmul_inplace(mixed, a["w"], dtype, f53)
        comp = oracle_c.compress_minmax_u8(mixed, dtype, 1)
        S = K.bagua_minmax_u8_compressed_bytes(dtype, n, 1)
        assert S == comp.size
        wsb = K.bagua_minmax_u8_workspace_bytes(n, 1)
        for shape in MIX_SHAPES:
            what = f"{case} n={n} {shape}"
            d = {k: to_dev(a[k], dtype) for k in "twlr"}
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
            with env(**shape):
                assert K.bagua_ring_mix_minmax(dtype, d["t"].data_ptr(), d["l"].data_ptr(), d["r"].data_ptr(),
                                               d["w"].data_ptr(), n, ws.data_ptr(), wsb, None) == 0, what
            assert K.bagua_minmax_u8_compress_stage(2, dtype, d["t"].data_ptr(), n, n, 1, out.data_ptr(), S,
                                                    ws.data_ptr(), wsb, -1, None) == 0, what
            assert_float_bits_equal(to_host(d["t"], dtype), mixed, dtype, f"{what}: mixed t")
            assert np.array_equal(out.cpu().numpy(), comp), f"{what}: compressed bytes"
            for k in "wlr":
                assert np.array_equal(to_host(d[k], dtype).view(np.uint8), a[k].view(np.uint8)), f"{what}: {k} changed"


# ---------------------------------------------------------------- apply ----
@pytest.mark.parametrize("row", list(range(APPLY_ROWS)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ring_apply_every_row_vs_oracle(bc, oracle_c, dtype, row):
    K = bc._native.K
    for triple in TRIPLES:
        bufs, a, want = apply_case(dtype, triple, N_RAGGED)
        with env(BAGUA_RING_APPLY_CFG=str(row)):
            rc, d, bd = run_apply(K, dtype, bufs, a, N_RAGGED)
        assert rc == 0
        check_apply(dtype, d, bd, bufs, want, f"row {row} {triple}")


@pytest.mark.parametrize("row", [8, 9, 20])
def test_ring_apply_grid_cap(bc, oracle_c, row):
    """Rows 8 and 9 cap the grid at 1024 workgroups: at this size every workgroup sweeps more
    than one batch (contiguous ranges and grid-strided), the last one partly, plus a ragged
    tail; row 20 (the default) for comparison at the same size."""
    K = bc._native.K
    bufs, a, want = apply_case(BF16, ("inverted", "constant", "benign"), N_CAP)
    with env(BAGUA_RING_APPLY_CFG=str(row)):
        rc, d, bd = run_apply(K, BF16, bufs, a, N_CAP)
    assert rc == 0
    check_apply(BF16, d, bd, bufs, want, f"cap row {row}")


# ---------------------------------------------------------- apply range ----
def piece_ranges(K, n, schedule):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & 0xFFFF):
        assert K.bagua_minmax_u8_piece_range(n, schedule, q, ctypes.byref(b), ctypes.byref(e)) == 0
        out.append((b.value, e.value))
    return out


@pytest.mark.parametrize("schedule", [3, 4 | 0x10000])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ring_apply_range_pieces_equal_whole(bc, oracle_c, dtype, schedule):
    """The pieces of bagua_minmax_u8_piece_range applied in reverse order == the whole apply
    (the last piece ends at a ragged n); a middle range alone leaves everything outside it
    untouched; an empty range writes nothing."""
    K = bc._native.K
    n = N_RAGGED
    bufs, a, want = apply_case(dtype, ("both_inf", "inverted", "constant"), n)
    ranges = piece_ranges(K, n, schedule)
    assert ranges[0][0] == 0 and ranges[-1][1] == n and n % VEC_N[dtype]
    bd = [torch.from_numpy(b).cuda() for b in bufs]
    d = {k: to_dev(a[k], dtype) for k in "twlr"}
    for e0, e1 in reversed(ranges):
        assert K.bagua_ring_apply_minmax_range(dtype, bd[0].data_ptr(), bd[1].data_ptr(), bd[2].data_ptr(),
                                               bufs[0].size, n, e0, e1, d["t"].data_ptr(), d["w"].data_ptr(),
                                               d["l"].data_ptr(), d["r"].data_ptr(), None) == 0
    check_apply(dtype, d, bd, bufs, want, f"pieces {schedule:#x}")
    # a middle range only
    e0, e1 = ranges[1]
    rc, d, bd = run_apply(K, dtype, bufs, a, n, e0, e1)
    assert rc == 0
    part = {k: np.concatenate([a[k][:e0], want[k][e0:e1], a[k][e1:]]) for k in "twlr"}
    check_apply(dtype, d, bd, bufs, part, f"middle range [{e0}, {e1})")
    # the ragged tail only (e1 == n, e0 the last vector boundary), then an empty range
    last = n // VEC_N[dtype] * VEC_N[dtype]
    rc, d, bd = run_apply(K, dtype, bufs, a, n, last, n)
    assert rc == 0
    part = {k: np.concatenate([a[k][:last], want[k][last:]]) for k in "twlr"}
    check_apply(dtype, d, bd, bufs, part, "tail range")
    rc, d, bd = run_apply(K, dtype, bufs, a, n, e0, e0)
    assert rc == 0
    check_apply(dtype, d, bd, bufs, a, "empty range")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ring_apply_range_return_codes(bc, dtype):
    K = bc._native.K
    n, N = N_RAGGED, VEC_N[dtype]
    bufs, a, _ = apply_case(dtype, ("both_inf", "inverted", "constant"), n)
    assert run_apply(K, dtype, bufs, a, n, N + 1, 4 * N)[0] == INVALID_ARG       # e0 off a vector boundary
    assert run_apply(K, dtype, bufs, a, n, N, 4 * N + 1)[0] == INVALID_ARG       # e1 off one, and not n
    assert run_apply(K, dtype, bufs, a, n, 4 * N, N)[0] == INVALID_ARG           # reversed
    assert run_apply(K, dtype, bufs, a, n, 0, n + 1)[0] == INVALID_ARG           # past the end
    bd = [torch.from_numpy(b).cuda() for b in bufs]
    shifted = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), bufs[0]])).cuda()[1:]  # payload off N bytes
    off = to_dev(a["t"], dtype, 1)  # one element off 16 B
    ok = {k: to_dev(a[k], dtype) for k in "twlr"}
    f = K.bagua_ring_apply_minmax_range
    S = bufs[0].size
    assert f(dtype, bd[0].data_ptr(), bd[1].data_ptr(), bd[2].data_ptr(), S, n, 0, n, off.data_ptr(),
             ok["w"].data_ptr(), ok["l"].data_ptr(), ok["r"].data_ptr(), None) == UNSUPPORTED
    assert f(dtype, shifted.data_ptr(), bd[1].data_ptr(), bd[2].data_ptr(), S, n, 0, n, ok["t"].data_ptr(),
             ok["w"].data_ptr(), ok["l"].data_ptr(), ok["r"].data_ptr(), None) == UNSUPPORTED
    for k in "twlr":  # nothing was launched
        assert np.array_equal(to_host(ok[k], dtype).view(np.uint8), a[k].view(np.uint8)), k
