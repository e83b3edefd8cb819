"""The 1-bit codec at the C ABI on hostile received segments and on every launch shape,
against the oracle's decompress_onebit -> reduce_chunks -> compress_onebit(target).

(a) the decoders on the crafted receive buffers of tests/onebit_segment_cases.py: whole and
    by tile range, aligned and one element off, both store policies, one workgroup;
(b) the fused middle step (bagua_onebit_reduce_requantize) on every class at every position,
    both ends of each table width, tensor stored / NULL, at the default launch shape and with
    one workgroup (four waves: the grid-stride loop takes several trips and the two-tile batch
    loses its second tile); every p <= 16 in f16; the U = 1 / 2 / 4 / 8 instantiations; the
    default grid cap; the per-element kernel behind BAGUA_ONEBIT_LUT=0 in a child process;
(c) the error-feedback middle step (bagua_onebit_reduce_requantize_ef) with a hard server
    state, carry and scale compared with tests/onebit_ef_reference.py;
(d) the encoders in f16, with one workgroup, two f32 tiles per iteration, special values;
(e) the return codes: a refused call launches nothing.

tests/test_onebit_edges_cpu.py checks on the CPU that the two oracles agree on every crafted
buffer.  Output buffers are poisoned (0xA5 bytes, 7.0 floats): every defined byte must be
written and nothing else.  Bytes are compared exactly, floats bit for bit; where the oracle's
float is NaN the GPU's must be NaN (x86 and gfx950 generate different default NaNs), which
covers decoded and reduced elements, the carry and the 4 scale bytes of a header."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import onebit_ef_reference as REF
import onebit_segment_cases as OS
from test_gpu_codec import BF16, F16, F32, STORAGE, TORCH, assert_float_bits_equal, bc, to_dev, to_host  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
IDS = ["f32", "f16", "bf16"]
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 2, 4
ALL_CLASSES = ["benign"] + OS.CLASSES
BIG_CS = 8193 * 1024 + 5  # more tiles than the 2048 x 4 waves of the default grid cap
KNOBS = ["BAGUA_TUNE_OB_MIDDLE_BLOCKS", "BAGUA_OB_MIDDLE_U", "BAGUA_TUNE_OB_DECODE_BLOCKS", "BAGUA_OB_DECODE_NT",
         "BAGUA_TUNE_OB_ENCODE_BLOCKS", "BAGUA_TUNE_OB_ENCODE_TPI", "BAGUA_TUNE_OB_EF_ENCODE_BLOCKS",
         "BAGUA_OB_EF_CARRY_NT"]


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    """every test starts from the default launch shapes; monkeypatch restores what it sets"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def set_knobs(monkeypatch, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        assert k in KNOBS
        monkeypatch.setenv(k, str(v))


def filled(n: int, dtype: int) -> torch.Tensor:
    return torch.full((n,), 7.0, dtype=TORCH[dtype], device="cuda")


def fill_kept(t: torch.Tensor) -> bool:
    return bool((t == 7.0).all().item())


def poison(n: int) -> torch.Tensor:
    return torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")


def workspace(K, cs):
    wsb = K.bagua_onebit_workspace_bytes(cs, 1)
    return torch.empty(wsb, dtype=torch.uint8, device="cuda"), wsb


def with_nan_as_nan(f):
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


middle_ref = with_nan_as_nan(OS.middle_step)
ef_ref = with_nan_as_nan(OS.ef_middle_step)


# ------------------------------------------------------------ (a) decode ----
def piece_ranges(K, cs, pieces):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(pieces):
        assert K.bagua_onebit_piece_range(cs, pieces, q, ctypes.byref(b), ctypes.byref(e)) == 0
        out.append((b.value, e.value))
    return out


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_decode_crafted(bc, oracle_c, monkeypatch, dtype, p):
    """bagua_onebit_decompress and _decompress_range (3 pieces) on every class: the decoded value
    is bit ? -scale : +scale stored in T, whatever the scale; tiles outside a range and the
    elements behind the tensor keep the fill."""
    K = bc._native.K
    cs = OS.CS
    ranges = piece_ranges(K, cs, 3)
    assert ranges[0][0] == 0 and ranges[-1][1] == OS.tiles_of(cs) and all(b < e for b, e in ranges)
    shapes = [{}, {"BAGUA_OB_DECODE_NT": 1}, {"BAGUA_OB_DECODE_NT": 0}, {"BAGUA_TUNE_OB_DECODE_BLOCKS": 1},
              {"BAGUA_TUNE_OB_DECODE_BLOCKS": 1, "BAGUA_OB_DECODE_NT": 1}]
    for cls in ALL_CLASSES:
        for k in OS.positions(p):
            recv = OS.crafted(cls, dtype, p, cs, k)
            want = OS.decode(oracle_c, recv, dtype, p, cs)
            rd = torch.from_numpy(recv).cuda()
            for offset in (0, 1):
                for knobs in shapes:
                    set_knobs(monkeypatch, **knobs)
                    what = f"{cls} p={p} k={k} offset={offset} {knobs}"
                    buf = filled(offset + p * cs + 64, dtype)
                    out = buf[offset:]
                    assert out.data_ptr() % 16 == (0 if offset == 0 else OS.NP.esize(dtype)), what
                    assert K.bagua_onebit_decompress(dtype, rd.data_ptr(), recv.size, cs, p, out.data_ptr(), None) == 0
                    got = to_host(buf, dtype)
                    assert_float_bits_equal(got[offset:offset + p * cs], want, dtype, what)
                    assert fill_kept(buf[:offset]) and fill_kept(buf[offset + p * cs:]), what
                    if "BAGUA_OB_DECODE_NT" in knobs and "BAGUA_TUNE_OB_DECODE_BLOCKS" not in knobs:
                        continue  # the ranges: at the default policy and with one workgroup
                    for tb, te in ranges:
                        buf = filled(offset + p * cs + 64, dtype)
                        out = buf[offset:]
                        assert K.bagua_onebit_decompress_range(dtype, rd.data_ptr(), recv.size, cs, p, out.data_ptr(),
                                                               tb, te, None) == 0
                        got = to_host(buf, dtype)[offset:offset + p * cs].reshape(p, cs)
                        lo, hi = tb * OS.TILE, min(te * OS.TILE, cs)
                        w = want.reshape(p, cs)
                        assert_float_bits_equal(np.ascontiguousarray(got[:, lo:hi]), np.ascontiguousarray(w[:, lo:hi]),
                                                dtype, f"{what} tiles [{tb}, {te})")
                        inside = torch.zeros(offset + p * cs + 64, dtype=torch.bool, device="cuda")
                        for c in range(p):
                            inside[offset + c * cs + lo:offset + c * cs + hi] = True
                        assert fill_kept(buf[~inside]), f"{what} tiles [{tb}, {te}): written outside the range"
            assert np.array_equal(rd.cpu().numpy(), recv), f"{cls}: the receive buffer changed"


# ------------------------------------------------- (b) fused middle step ----
def run_middle(K, dtype, rd, recv, p, cs, target, average, store, want, ws, what):
    """One bagua_onebit_reduce_requantize against want = (reduced chunk, segment)."""
    red, seg = want
    S = recv.size
    co = S // p
    t_d = filled(p * cs, dtype)
    out = poison(S)
    rc = K.bagua_onebit_reduce_requantize(dtype, rd.data_ptr(), S, cs, p, t_d.data_ptr() if store else None, average,
                                          out.data_ptr(), S, target, ws[0].data_ptr(), ws[1], None)
    assert rc == 0, f"{what}: status {rc}"
    torch.cuda.synchronize()
    own = slice(target * cs, (target + 1) * cs)
    if store:
        assert_float_bits_equal(to_host(t_d[own], dtype), red, dtype, f"{what}: reduced chunk")
    else:
        assert fill_kept(t_d[own]), f"{what}: tensor written though NULL was passed"
    assert fill_kept(t_d[:target * cs]) and fill_kept(t_d[(target + 1) * cs:]), f"{what}: another chunk written"
    mine = slice(target * co, (target + 1) * co)
    bad = OS.segment_mismatch(out[mine].cpu().numpy(), seg)
    assert not bad, f"{what}: segment: {bad}"
    assert bool((out[:target * co] == 0xA5).all()) and bool((out[(target + 1) * co:] == 0xA5).all()), \
        f"{what}: bytes outside the target segment written"


def middle_cases(dtype, p, cs, classes):
    for cls in classes:
        for k in OS.positions(p):
            yield cls, k, OS.crafted(cls, dtype, p, cs, k), (k + 1) % p


def run_middle_cases(K, oracle_c, monkeypatch, dtype, p, cs, classes, shapes, stores=(True, False)):
    ws = workspace(K, cs)
    n = 0
    for cls, k, recv, target in middle_cases(dtype, p, cs, classes):
        rd = torch.from_numpy(recv).cuda()
        for average in (0, 1):
            _, red, seg = middle_ref(oracle_c, recv, dtype, p, cs, target, average)
            for knobs in shapes:
                if monkeypatch is not None:
                    set_knobs(monkeypatch, **knobs)
                for store in stores:
                    run_middle(K, dtype, rd, recv, p, cs, target, average, store, (red, seg), ws,
                               f"{cls} {OS.NAMES[dtype]} p={p} k={k} average={average} store={store} {knobs}")
                    n += 1
        assert np.array_equal(rd.cpu().numpy(), recv), f"{cls}: the receive buffer changed"
    return n


SHAPES = [{}, {"BAGUA_TUNE_OB_MIDDLE_BLOCKS": 1}]


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_middle_step_crafted(bc, oracle_c, monkeypatch, dtype, p):
    """Every class at every position, both ends of each table width (PMAX = 2, 4, 8, 16), sum and
    mean, tensor stored and NULL (the group table at p <= 2, the pair table at p <= 4), at the
    default launch shape and with one workgroup."""
    run_middle_cases(bc._native.K, oracle_c, monkeypatch, dtype, p, OS.CS, ALL_CLASSES, SHAPES)


@pytest.mark.parametrize("p", list(range(1, 17)))
def test_middle_step_f16_every_p(bc, oracle_c, monkeypatch, p):
    """f16 is the one type where a received scale can be denormal or overflow, and p = 6, 7 and
    9..15 never ran in it: every p on a benign buffer, a NaN scale and a negative one."""
    run_middle_cases(bc._native.K, oracle_c, monkeypatch, F16, p, OS.CS, ["benign", "nan_scale", "neg_scale"], SHAPES)


@pytest.mark.parametrize("u", [1, 2, 4, 8])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_middle_step_u_variants(bc, oracle_c, monkeypatch, p, u):
    """The UT = 1 / 2 / 4 / 8 instantiations BAGUA_OB_MIDDLE_U selects (tensor NULL), four waves:
    with 11, 17 and 33 tiles every u slot is present in some trips and absent in others."""
    K = bc._native.K
    for dtype in DTYPES:
        for tiles in (11, 17, 33):
            run_middle_cases(K, oracle_c, monkeypatch, dtype, p, (tiles - 1) * 1024 + 300,
                             ["benign", "bits_marker", "neg_scale"],
                             [{"BAGUA_OB_MIDDLE_U": u, "BAGUA_TUNE_OB_MIDDLE_BLOCKS": 1}], stores=(False,))


def test_middle_step_default_grid_cap(bc, oracle_c):
    """No knob set: 8194 tiles on the 8192 waves of the default grid, so waves 0 and 1 take a
    second trip; a negative scale in segment 1."""
    K = bc._native.K
    dtype, p, cs, target = F32, 3, BIG_CS, 2
    recv = OS.crafted("neg_scale", dtype, p, cs, 1)
    rd = torch.from_numpy(recv).cuda()
    ws = workspace(K, cs)
    _, red, seg = middle_ref(oracle_c, recv, dtype, p, cs, target, 1)
    for store in (True, False):
        run_middle(K, dtype, rd, recv, p, cs, target, 1, store, (red, seg), ws, f"grid cap store={store}")


LUT_CHILD_PS = [2, 4, 8, 16]


def run_lut_cases():
    """Body of the child process (tests/onebit_lut_child.py): the per-element kernel
    onebit_reduce_encode_kernel, BY = 2, 4, 8."""
    import bagua_core
    from oracle import oracle_c
    oracle_c.build()
    n = 0
    for dtype in (F32, F16):
        for p in LUT_CHILD_PS:
            n += run_middle_cases(bagua_core._native.K, oracle_c, None, dtype, p, OS.CS, ALL_CLASSES, [{}])
    return n


def test_per_element_kernel_in_child_process(bc):
    """BAGUA_ONEBIT_LUT is read once per process, so a fresh interpreter runs the crafted cases
    on the per-element kernel: same bytes as the oracle."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "onebit_lut_child.py")
    env = dict(os.environ, BAGUA_ONEBIT_LUT="0")
    for k in KNOBS:
        env.pop(k, None)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    want = sum(len(OS.positions(p)) for p in LUT_CHILD_PS) * len(ALL_CLASSES) * 2 * 2 * 2
    assert f"per-element cases ok: {want}" in r.stdout, r.stdout[-2000:]


# ---------------------------------------- (c) error-feedback middle step ----
EF_CLASSES = ["nan_scale", "neg_scale", "neg_zero_scale", "inf_cancel", "denormal_16", "overflow_16", "equal_cancel",
              "bits_marker", "padding_bits_set"]


def hard_carry(cs: int, scale: float, seed: int) -> np.ndarray:
    """random normal x 1e-3 with entries at -0, +0, a denormal and +-scale exactly, in the
    first tile, across a tile edge and in the ragged tail"""
    rng = np.random.default_rng(seed)
    carry = (rng.standard_normal(cs) * 1e-3).astype(np.float32)
    specials = np.array([-0.0, 0.0, 1e-40, -1e-40, scale, -scale], np.float32)
    for base in (3, 1024 - 9, cs - 40):
        if 0 <= base and base + 36 <= cs:
            carry[base:base + 36] = np.tile(specials, 6)
    return carry


def run_ef_middle(K, oracle_c, dtype, recv, p, cs, target, average, carry, scale, ws, what):
    S = recv.size
    co = S // p
    seg, v2, s2 = ef_ref(oracle_c, recv, dtype, p, cs, target, average, carry.copy(), scale)
    rd = torch.from_numpy(recv).cuda()
    cd = torch.full((cs + 64,), 7.0, dtype=torch.float32, device="cuda")
    cd[:cs] = torch.from_numpy(carry).cuda()
    sd = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    sd[0] = float(scale)
    out = poison(S)
    assert cd.data_ptr() % 16 == 0 and sd.data_ptr() % 16 == 0
    rc = K.bagua_onebit_reduce_requantize_ef(dtype, rd.data_ptr(), S, cs, p, average, out.data_ptr(), S, target,
                                             ws[0].data_ptr(), ws[1], cd.data_ptr(), sd.data_ptr(), None)
    assert rc == 0, f"{what}: status {rc}"
    torch.cuda.synchronize()
    bad = OS.segment_mismatch(out[target * co:(target + 1) * co].cpu().numpy(), seg)
    assert not bad, f"{what}: segment: {bad}"
    assert bool((out[:target * co] == 0xA5).all()) and bool((out[(target + 1) * co:] == 0xA5).all()), what
    assert_float_bits_equal(cd[:cs].cpu().numpy(), v2, F32, f"{what}: carry")
    assert fill_kept(cd[cs:]), f"{what}: written past the carry"
    got_s = sd.cpu().numpy()
    assert_float_bits_equal(got_s[:1], np.array([s2], np.float32), F32, f"{what}: new scale")
    assert np.all(got_s[1:] == 7.0), what
    assert np.array_equal(rd.cpu().numpy(), recv), f"{what}: the receive buffer changed"


@pytest.mark.parametrize("p", [1, 2, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ef_middle_step_crafted(bc, oracle_c, dtype, p):
    """bagua_onebit_reduce_requantize_ef called directly, with hostile segments and a non-zero
    server state: segment, every carry entry and the new scale as centralized_step composes
    them.  One extra case each with a zero and a negative server scale."""
    K = bc._native.K
    cs = OS.CS
    ws = workspace(K, cs)
    for cls in EF_CLASSES:
        for k in OS.positions(p):
            recv = OS.crafted(cls, dtype, p, cs, k)
            target = (k + 1) % p
            for average in (0, 1):
                run_ef_middle(K, oracle_c, dtype, recv, p, cs, target, average, hard_carry(cs, 7e-4, p + k), 7e-4, ws,
                              f"ef {cls} p={p} k={k} average={average}")
    recv = OS.crafted("bits_marker", dtype, p, cs, 0)
    for scale in (0.0, -7e-4):
        for average in (0, 1):
            run_ef_middle(K, oracle_c, dtype, recv, p, cs, p - 1, average, hard_carry(cs, abs(scale), 5), scale, ws,
                          f"ef server scale {scale} p={p} average={average}")


def test_ef_middle_step_grid_stride(bc, oracle_c):
    """8194 tiles: the kernel has no launch knob, so only a chunk this large reaches its
    grid-stride loop"""
    K = bc._native.K
    p, cs = 2, BIG_CS
    recv = OS.crafted("neg_scale", F32, p, cs, 0)
    run_ef_middle(K, oracle_c, F32, recv, p, cs, 1, 1, hard_carry(cs, 7e-4, 1), 7e-4, workspace(K, cs), "ef grid stride")


# ------------------------------------------------------------ (d) encode ----
def oracle_compress(oracle_c, x, dtype, n_in, cs, p, target=-1):
    size = oracle_c.onebit_compressed_size(p, cs)
    out = np.zeros(size, dtype=np.uint8)
    with np.errstate(all="ignore"):
        rc = oracle_c.lib().orc_compress_onebit(oracle_c._ptr(x), dtype, n_in, cs, p, oracle_c._ptr(out), size, target)
    assert rc == 0, rc
    return out


def check_compressed(got, want, p, target, what):
    co = want.size // p
    for c in range(p):
        g = got[c * co:(c + 1) * co]
        if target >= 0 and c != target:
            assert np.all(g == 0xA5), f"{what}: segment {c} written"
            continue
        bad = OS.segment_mismatch(g, want[c * co:(c + 1) * co])
        assert not bad, f"{what}: segment {c}: {bad}"
    assert np.array_equal(got[p * co:], want[p * co:]), what


def gpu_compress(K, xd, dtype, n_in, cs, p, target=-1):
    S = K.bagua_onebit_compressed_bytes(cs, p)
    wsb = K.bagua_onebit_workspace_bytes(cs, p)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = poison(S)
    rc = K.bagua_onebit_compress(dtype, xd.data_ptr(), n_in, cs, p, out.data_ptr(), S, ws.data_ptr(), wsb, target, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def sample(dtype, n, seed, specials=False):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    x[rng.integers(0, n, size=max(1, n // 1000))] *= -1e3
    if specials:
        den = {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}[dtype]
        sp = np.array([0.0, -0.0, den, -den, np.inf, -np.inf, np.nan, -0.0], np.float32)
        x[:6] = sp[:6] if n >= 6 else x[:6]        # chunk 0 stays finite: zeros and denormals only
        if n > 2100:
            x[n - 1030:n - 1022] = sp              # the last chunk: inf and NaN across a tile edge
            x[n // 2:n // 2 + 2] = [np.inf, -np.inf]  # p = 3: the middle chunk's scale is +inf
    return OS.NP.from_f32(x, dtype)


F16_SHAPES = [(1, 3 * 1024 + 517, None, -1), (3, 1024 * 5 + 3, None, -1), (2, 700, None, -1),
              (4, 1024 * 9, 1024 * 9 * 2 + 1024 * 3 + 77, -1), (3, 1024 * 6 + 1, None, 1)]


@pytest.mark.parametrize("p,cs,n_in,target", F16_SHAPES)
def test_encode_f16_vs_oracle(bc, oracle_c, p, cs, n_in, target):
    """bagua_onebit_compress in f16 (the two-tiles-per-iteration kernel): ragged chunks, a chunk
    below one tile, a valid count that ends inside chunk 2, a target chunk; plain and special
    values."""
    K = bc._native.K
    n_in = p * cs if n_in is None else n_in
    for specials in (False, True):
        x = sample(F16, p * cs, cs + p, specials)
        want = oracle_compress(oracle_c, x, F16, n_in, cs, p, target)
        got = gpu_compress(K, to_dev(x, F16), F16, n_in, cs, p, target)
        check_compressed(got, want, p, target, f"f16 p={p} cs={cs} n_in={n_in} target={target} specials={specials}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_encode_launch_shapes(bc, oracle_c, monkeypatch, dtype):
    """One workgroup (four waves stride over the tiles; the 16-bit kernels take two tiles per
    iteration, so an odd tile count leaves the second one absent), and for f32 the TPI = 2
    instantiation; inputs hold NaN, +-inf, +-0 and denormals."""
    K = bc._native.K
    shapes = [{"BAGUA_TUNE_OB_ENCODE_BLOCKS": 1}]
    if dtype == F32:
        shapes += [{"BAGUA_TUNE_OB_ENCODE_TPI": 2}, {"BAGUA_TUNE_OB_ENCODE_TPI": 2, "BAGUA_TUNE_OB_ENCODE_BLOCKS": 1}]
    for p, cs, offset in ((1, 1024 * 22 + 5, 0), (2, 1024 * 21 + 700, 0), (3, 1024 * 9, 0), (2, 1024 * 12 + 1, 1)):
        x = sample(dtype, p * cs, 3 * cs + p, specials=True)
        want = oracle_compress(oracle_c, x, dtype, p * cs, cs, p)
        xd = to_dev(x, dtype, offset)
        for knobs in shapes:
            set_knobs(monkeypatch, **knobs)
            check_compressed(gpu_compress(K, xd, dtype, p * cs, cs, p), want, p, -1,
                             f"{OS.NAMES[dtype]} p={p} cs={cs} offset={offset} {knobs}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_encode_ef_launch_shapes(bc, oracle_c, monkeypatch, dtype):
    """bagua_onebit_compress_ef with one workgroup and with either carry policy forced, two steps
    each: payload, carry and scales as onebit_ef_reference.compress_ef."""
    K = bc._native.K
    p, cs = 3, 1024 * 9 + 300
    n = p * cs
    S = K.bagua_onebit_compressed_bytes(cs, p)
    wsb = K.bagua_onebit_workspace_bytes(cs, p)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for knobs in ({"BAGUA_TUNE_OB_EF_ENCODE_BLOCKS": 1}, {"BAGUA_OB_EF_CARRY_NT": 0}, {"BAGUA_OB_EF_CARRY_NT": 1}):
        set_knobs(monkeypatch, **knobs)
        carry = torch.zeros(n + 64, dtype=torch.float32, device="cuda")
        carry[n:] = 7.0
        scales = torch.zeros(4, dtype=torch.float32, device="cuda")
        ref = REF.WorkerState(n, p)
        for step in range(2):
            x = sample(dtype, n, 10 * step + dtype)
            xd = to_dev(x, dtype)
            out = poison(S)
            rc = K.bagua_onebit_compress_ef(dtype, xd.data_ptr(), n, cs, p, out.data_ptr(), S, ws.data_ptr(), wsb, -1,
                                            carry.data_ptr(), scales.data_ptr(), None)
            assert rc == 0, rc
            torch.cuda.synchronize()
            want = REF.compress_ef(oracle_c, x, dtype, p, ref)
            what = f"{OS.NAMES[dtype]} {knobs} step {step}"
            assert np.array_equal(out.cpu().numpy(), want), f"{what}: payload"
            assert_float_bits_equal(carry[:n].cpu().numpy(), ref.carry, F32, f"{what}: carry")
            assert fill_kept(carry[n:]), what
            assert np.array_equal(scales.cpu().numpy()[:p].view(np.uint32), ref.scales.view(np.uint32)), what
            assert scales[3].item() == 0.0, what


# ------------------------------------------------------ (e) return codes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_middle_step_return_codes(bc, dtype):
    K = bc._native.K
    cs = OS.CS
    tiles = OS.tiles_of(cs)
    co = 32 + tiles * 128
    recv = torch.zeros(17 * co + 16, dtype=torch.uint8, device="cuda")
    out = poison(17 * co + 16)
    t_d = filled(2 * cs, dtype)
    ws, wsb = workspace(K, cs)
    ws.fill_(0xA5)
    carry = filled(cs, F32)
    scale = filled(4, F32)
    need = tiles * 4

    def plain(rp, rbytes, p, target, w, wbytes):
        return K.bagua_onebit_reduce_requantize(dtype, rp, rbytes, cs, p, t_d.data_ptr(), 1, out.data_ptr(), rbytes,
                                                target, w, wbytes, None)

    def ef(rp, rbytes, p, target, w, wbytes):
        return K.bagua_onebit_reduce_requantize_ef(dtype, rp, rbytes, cs, p, 1, out.data_ptr(), rbytes, target, w,
                                                   wbytes, carry.data_ptr(), scale.data_ptr(), None)

    for f in (plain, ef):
        assert f(recv.data_ptr(), 17 * co, 17, 0, ws.data_ptr(), wsb) == UNSUPPORTED    # p > 16
        assert f(recv.data_ptr(), 2 * co, 2, 2, ws.data_ptr(), wsb) == UNSUPPORTED      # target out of range
        assert f(recv.data_ptr(), 2 * co, 2, -1, ws.data_ptr(), wsb) == UNSUPPORTED
        assert f(recv.data_ptr(), 2 * (co - 4), 2, 0, ws.data_ptr(), wsb) == INVALID_ARG  # too small for the tiles
        assert f(recv.data_ptr(), 2 * co, 2, 0, ws.data_ptr(), need - 1) == WORKSPACE   # one byte short
        assert f(recv.data_ptr(), 2 * co, 2, 0, None, wsb) == WORKSPACE
        assert f(recv[1:].data_ptr(), 2 * co, 2, 0, ws.data_ptr(), wsb) == INVALID_ARG  # (ptr + 32) % 4 != 0
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == 0xA5).all()), "a refused call wrote its output"
    assert fill_kept(t_d) and fill_kept(carry) and fill_kept(scale), "a refused call wrote tensor or state"
