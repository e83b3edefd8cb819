"""Planted extrema through every form of the two-pass encode's min/max pass
(minmax_partials_kernel) and the one-rank op that shares it.

The base data stays inside a narrow band; each chunk's minimum and maximum are
single elements planted in named regions of the pass (tests/planted_cases.py:
scalar head and tail, first and last lanes, every subtile, the second
grid-stride iteration, the ragged top tile, the load-policy split), a
different pair per chunk, so one launch of p = 64 chunks covers 128 positions.
A pass that never folds one of these regions writes a wrong header; the whole
poisoned buffer is compared with the C oracle, the headers first, naming the
planted regions.  tests/test_planted_cpu.py proves that every plant decides its
header.

Not constructible: a 16-bit input whose element pointer is odd (the all-scalar
branch at minmax_u8.hip:86) -- torch tensors are element-aligned; the branch
stays unreached here.
"""
import ctypes

import numpy as np
import pytest
import torch

import planted_cases as PC
from test_gpu_codec import BF16, F16, F32, STORAGE, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
PIECES_TAPERED = 0x10000  # bagua_kernels.h BAGUA_PIECES_TAPERED
P = PC.SHAPE_A_P


@pytest.fixture(autouse=True)
def two_pass_only(monkeypatch):
    """this file is about the two-pass encode: the one-launch encode stays off"""
    monkeypatch.setenv("BAGUA_RESIDENT", "0")


class Encoder:
    def __init__(self, bc, dtype, x, p, num_elem=None, offset=0):
        self.N, self.K = bc._native, bc._native.K
        self.dtype, self.p, self.cs = dtype, p, x.size // p
        self.n_in = x.size if num_elem is None else num_elem
        self.xd = to_dev(x, dtype, offset)
        assert self.xd.data_ptr() % 128 == offset * PC.esize(dtype)  # the geometry's byte_offset
        self.S = self.K.bagua_minmax_u8_compressed_bytes(dtype, self.cs, p)
        self.wsb = self.K.bagua_minmax_u8_workspace_bytes(self.cs, p)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fresh(self):
        return torch.full((self.S,), 0xA5, dtype=torch.uint8, device="cuda")

    def args(self, out, target):
        return (self.dtype, self.xd.data_ptr(), self.n_in, self.cs, self.p, out.data_ptr(), self.S,
                self.ws.data_ptr(), self.wsb, target)

    def forward(self, target=-1):
        out = self.fresh()
        assert self.K.bagua_minmax_u8_resident_path(self.dtype, self.xd.data_ptr(), self.n_in, self.cs, self.p,
                                                    out.data_ptr(), self.S, target, self.sp) == 0
        self.N.check(self.K.bagua_minmax_u8_compress(*self.args(out, target), self.sp), "compress")
        return out

    def backward(self, target=-1):
        out = self.fresh()
        self.N.check(self.K.bagua_minmax_u8_compress_stage(5, *self.args(out, target), self.sp), "stage 5")
        self.N.check(self.K.bagua_minmax_u8_compress_stage(2, *self.args(out, target), self.sp), "stage 2")
        return out

    def pieced(self, schedule):
        out = self.fresh()
        self.N.check(self.K.bagua_minmax_u8_compress_stage(1, *self.args(out, -1), self.sp), "stage 1")
        b, e = ctypes.c_int(), ctypes.c_int()
        for q in range(schedule & 0xFFFF):
            self.N.check(self.K.bagua_minmax_u8_piece_range(self.cs, schedule, q, ctypes.byref(b), ctypes.byref(e)), "range")
            self.N.check(self.K.bagua_minmax_u8_quantize_range(*self.args(out, -1), b.value, e.value, self.sp),
                         f"piece {q}")
        return out


def check(out, want, dtype, p, plants, what, target=-1):
    got = out.cpu().numpy()
    assert got.size == want.size
    if target >= 0:
        PC.assert_headers(got, want, dtype, p, plants, what, chunks=[target])
        co = got.size // p
        assert np.array_equal(got[target * co:(target + 1) * co], want[target * co:(target + 1) * co]), what
        return
    PC.assert_headers(got, want, dtype, p, plants, what)
    assert np.array_equal(got, want), f"{what}: payload, gap or slack bytes differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
@pytest.mark.parametrize("kind", PC.KINDS)
def test_two_pass_forms_see_every_region(bc, oracle_c, monkeypatch, kind, dtype):
    """forward, backward, both with non-temporal loads (the backward one with the
    kept-tail split inside every chunk), target chunks and the pieced encode, on one
    planted input, plain and with NaN in the plants' vectors"""
    cs = PC.shape_a_cs(dtype)
    plants = PC.shape_a_plants(dtype, keep_mib=1)
    for nan in (False, True):
        x, _ = PC.build(dtype, kind, P, cs, plants, seed=dtype * 7 + len(kind), nan=nan,
                        vector_origin=PC.shape_a_origin(dtype))
        want = oracle_c.compress_minmax_u8(x, dtype, P)
        enc = Encoder(bc, dtype, x, P)
        tag = f"{kind} {PC.DTYPE_NAME[dtype]}{' nan_in_vector' if nan else ''}"
        fwd = enc.forward()
        check(fwd, want, dtype, P, plants, f"{tag} forward")
        check(enc.backward(), want, dtype, P, plants, f"{tag} backward")
        with monkeypatch.context() as m:
            m.setenv("BAGUA_PARTIALS_NT", "1")
            m.setenv("BAGUA_PARTIALS_KEEP_MIB", "1")
            check(enc.forward(), want, dtype, P, plants, f"{tag} non-temporal forward")
            check(enc.backward(), want, dtype, P, plants, f"{tag} non-temporal backward, 1 MiB kept")
        for target in (5, P - 1):  # one workgroup per tile: no second iteration
            check(enc.forward(target), want, dtype, P, plants, f"{tag} forward target {target}", target)
            check(enc.backward(target), want, dtype, P, plants, f"{tag} backward target {target}", target)
        if not nan:
            # the header must not depend on which piece holds the extremum
            check(enc.pieced(4), want, dtype, P, plants, f"{tag} pieced, 4 pieces")
            check(enc.pieced(4 | PIECES_TAPERED), want, dtype, P, plants, f"{tag} pieced, 4 tapered pieces")
            y = torch.empty(P * cs, dtype=enc.xd.dtype, device="cuda")
            enc.N.check(enc.K.bagua_minmax_u8_decompress(dtype, fwd.data_ptr(), enc.S, cs, P, y.data_ptr(), enc.sp),
                        "decode")
            dw = np.empty(P * cs, dtype=STORAGE[dtype])
            oracle_c.decompress_minmax_u8(want, P, dw, dtype)
            assert_float_bits_equal(to_host(y, dtype), dw, dtype, f"{tag} decode")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
@pytest.mark.parametrize("kind", ["margin", "signed_zero"])
def test_two_pass_offset_pointer(bc, oracle_c, kind, dtype):
    """the input pointer one element past a 128-byte line: chunk 0 has a head too, and
    every chunk's head, body and tail move"""
    cs = PC.shape_a_cs(dtype)
    off = PC.esize(dtype)
    plants = PC.shape_a_plants(dtype, byte_offset=off)
    assert PC.two_pass(dtype, cs, 0, P, off).head == 128 // off - 1
    x, _ = PC.build(dtype, kind, P, cs, plants, seed=3, nan=True, vector_origin=PC.shape_a_origin(dtype, byte_offset=off))
    want = oracle_c.compress_minmax_u8(x, dtype, P)
    enc = Encoder(bc, dtype, x, P, offset=1)
    tag = f"{kind} {PC.DTYPE_NAME[dtype]} pointer + 1 element"
    check(enc.forward(), want, dtype, P, plants, f"{tag} forward")
    check(enc.backward(), want, dtype, P, plants, f"{tag} backward")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
def test_two_pass_ragged_tile_reaches_its_last_subtile(bc, oracle_c, dtype):
    """The shape above leaves the ragged tile at 3 subtiles and 5 vectors; here it has 7
    subtiles and about 40 vectors, so the ragged branch runs to its last subtile (p = 3, one
    workgroup per tile)."""
    p, N = 3, PC.vec_n(dtype)
    cs = (PC.TILE + 7 * PC.K_BLOCK + 40) * N + 3
    geo = [PC.two_pass(dtype, cs, c, p) for c in range(p)]
    assert all(g.full_tiles == 1 and g.nvec % PC.TILE > 7 * PC.K_BLOCK for g in geo)
    plants = []
    for c, g in enumerate(geo):
        pos = PC.two_pass_positions(g)
        names = ["ragged_tile_last_vec", "ragged_tile_first_vec", "full_tile_last_vec"]
        plants += [PC.Plant(c, pos[names[c % 3]], "min", names[c % 3]),
                   PC.Plant(c, pos[names[(c + 1) % 3]], "max", names[(c + 1) % 3])]
    x, _ = PC.build(dtype, "margin", p, cs, plants, seed=17, nan=True, vector_origin=lambda c: geo[c].head)
    want = oracle_c.compress_minmax_u8(x, dtype, p)
    enc = Encoder(bc, dtype, x, p)
    check(enc.forward(), want, dtype, p, plants, f"ragged tile of 7 subtiles {PC.DTYPE_NAME[dtype]} forward")
    check(enc.backward(), want, dtype, p, plants, f"ragged tile of 7 subtiles {PC.DTYPE_NAME[dtype]} backward")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
def test_two_pass_partially_valid_bucket(bc, oracle_c, dtype):
    """input_num_element ends inside chunk p-2: its last valid element is planted, the
    first invalid one and the last element of the empty chunk p-1 hold +-INIT_MAX/2,
    which must stay out of every header (the oracle decides their payload bytes)"""
    cs = PC.shape_a_cs(dtype)
    n_in = (P - 2) * cs + 2 * PC.TILE * PC.vec_n(dtype) + 77
    ragged = P - 2
    plants = PC.shape_a_plants(dtype, num_elem=n_in, chunks=range(P - 1))
    plants = [pl for pl in plants if pl.chunk != ragged]
    g = PC.two_pass(dtype, cs, ragged, P, num_elem=n_in)
    plants += [PC.Plant(ragged, g.valid - 1, "max", "last_valid_element"),
               PC.Plant(ragged, g.elem(g.full_tiles * PC.TILE), "min", "ragged_tile_first_vec")]
    x, _ = PC.build(dtype, "margin", P, cs, plants, seed=11, num_elem=n_in)
    PC.plant_negative(x, dtype, n_in, n_in, negative=False)          # first invalid element
    PC.plant_negative(x, dtype, n_in + 1, n_in, negative=True)
    PC.plant_negative(x, dtype, P * cs - 1, n_in, negative=True)     # last element of the empty chunk
    want = oracle_c.compress_minmax_u8(x, dtype, P, num_elem=n_in)
    assert PC.header_bits(want, dtype, P, ragged) == (PC.t_bits(-1.0, dtype), PC.t_bits(1.0, dtype))
    enc = Encoder(bc, dtype, x, P, num_elem=n_in)
    tag = f"partially valid {PC.DTYPE_NAME[dtype]}"
    fwd = enc.forward()
    check(fwd, want, dtype, P, plants, f"{tag} forward")
    check(enc.backward(), want, dtype, P, plants, f"{tag} backward")
    for target in (ragged, P - 1):
        check(enc.forward(target), want, dtype, P, plants, f"{tag} target {target}", target)
    y = torch.empty(P * cs, dtype=enc.xd.dtype, device="cuda")
    enc.N.check(enc.K.bagua_minmax_u8_decompress(dtype, fwd.data_ptr(), enc.S, cs, P, y.data_ptr(), enc.sp), "decode")
    dw = np.empty(P * cs, dtype=STORAGE[dtype])
    oracle_c.decompress_minmax_u8(want, P, dw, dtype)
    assert_float_bits_equal(to_host(y, dtype), dw, dtype, f"{tag} decode")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
@pytest.mark.parametrize("kind", PC.KINDS)
def test_one_rank_op_sees_every_region(bc, oracle_c, monkeypatch, kind, dtype):
    """bagua_minmax_u8_centralized_one_rank on a 3 MiB tensor with the last MiB loaded with
    the default policy: plants either side of the split, in the head and in the tail
    (the tensor starts one element past a line, so all three exist)"""
    from oracle import simulate
    K = bc._native.K
    monkeypatch.setenv("BAGUA_ONE_RANK_KEEP_MIB", "1")
    es = PC.esize(dtype)
    n = (3 << 20) // es + 2 * PC.vec_n(dtype) + 1
    g = PC.two_pass(dtype, n, 0, 1, byte_offset=es)
    pos = PC.two_pass_positions(g)
    pos.update(PC.nt_positions(g, PC.nt_until(n * es, 1 << 20)))
    names = ["head_first", "head_last", "last_nt_tile_last_vec", "straddling_tile_first_vec", "below_nt_until",
             "at_nt_until", "ragged_tile_last_vec", "tail_first", "tail_last"]
    assert all(nm in pos for nm in names), sorted(pos)
    wsb = K.bagua_minmax_u8_workspace_bytes(n, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    base = PC.base_data(dtype, kind, n, 5)
    for i, nm in enumerate(names):  # every region takes both roles over the runs
        other = names[(i + 4) % len(names)]
        plants = [PC.Plant(0, pos[nm], "min", nm), PC.Plant(0, pos[other], "max", other)]
        x, _ = PC.build(dtype, kind, 1, n, plants, base=base, nan=bool(i & 1), vector_origin=lambda c: g.head)
        average = i & 1
        want = simulate.centralized_low_precision(oracle_c, [x.copy()], dtype, bool(average))[0]
        xt = to_dev(x, dtype, 1)
        assert xt.data_ptr() % 128 == es
        assert K.bagua_minmax_u8_centralized_one_rank(dtype, xt.data_ptr(), n, average, ws.data_ptr(), wsb, None) == 0
        assert_float_bits_equal(to_host(xt, dtype), want, dtype,
                                f"one-rank op {kind} {PC.DTYPE_NAME[dtype]}, planted {plants[0]}, {plants[1]}")
