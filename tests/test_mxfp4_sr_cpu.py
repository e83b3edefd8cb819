"""CPU tests of the MXFP4 codec's stochastic rounding (MXFP4.md, "Stochastic rounding"): the
kernels' arithmetic compiled for the host against the numpy statement of the rule
(tests/mxfp4_sr_reference.py), the rule's properties on that reference, the host-only C
entries and the op simulated on the CPU.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mxfp4_boundary_cases as B
import mxfp4_reference as R
import mxfp4_sr_reference as SR
import onebit_ef_reference as OB
import op_edge_cases as E
from oracle import oracle_np as NP
from test_abi import LIB, built, declared, exported  # noqa: F401  (built: fixture)
from test_mxfp4_cpu import hostile_blocks, random_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
DTYPES = [F32, F16, BF16]
KEY = SR.key(0xB0A7, 3, 1, 0)

KERNEL_SYMBOLS = ["bagua_mxfp4_sr_key", "bagua_mxfp4_sr_word", "bagua_mxfp4_compress_sr",
                  "bagua_mxfp4_compress_sr_range", "bagua_mxfp4_reduce_requantize_sr",
                  "bagua_mxfp4_reduce_requantize_sr_range"]
CORE_SYMBOLS = ["bagua_tensor_compress_mxfp4_stochastic", "bagua_centralized_mxfp4_stochastic"]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mxfp4_sr") / "mxfp4_host_check")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "bagua-core_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tools", "mxfp4_host_check.cpp"), "-o", exe], check=True)
    return exe


def maxf_hex(dtype):
    return "%08x" % np.float32(R.MAX_FINITE[dtype]).view(np.uint32)


def host_keyed(exe, x, dtype, key, j0):
    """the `sr` mode: consecutive blocks, the first element having index j0"""
    out = subprocess.run([exe, "sr", maxf_hex(dtype), "%016x" % key, str(j0)], input=x.astype(np.float32).tobytes(),
                         capture_output=True, check=True).stdout
    got = np.frombuffer(out, np.uint8).reshape(-1, 17)
    return got[:, 0], got[:, 1:]


def host_explicit(exe, x, dtype, r):
    """the `srr` mode: mx_quant_sr under explicit r values"""
    raw = np.concatenate([x.astype(np.float32).view(np.uint32), np.asarray(r, np.uint32).reshape(x.shape)], axis=1)
    out = subprocess.run([exe, "srr", maxf_hex(dtype)], input=raw.tobytes(), capture_output=True, check=True).stdout
    got = np.frombuffer(out, np.uint8).reshape(-1, 17)
    return got[:, 0], got[:, 1:]


def nibbles(payload):
    nib = np.empty((payload.shape[0], 32), np.uint8)
    nib[:, 0::2] = payload & 15
    nib[:, 1::2] = payload >> 4
    return nib


def edge_blocks(dtype):
    """the hostile classes of the op-edge tests, rank p - 1's gradient as whole blocks"""
    rows = []
    for cls in E.CLASSES:
        x = E.build(cls, 2, 64, dtype, E.case_rng("sr", cls, dtype))[-1]
        rows.append(NP.to_f32(x, dtype).astype(np.float64).reshape(-1, 32))
    return np.concatenate(rows)


def all_inputs(dtype):
    return np.concatenate([random_blocks(dtype, 3000, 131 + dtype), hostile_blocks(dtype), edge_blocks(dtype),
                           B.table(dtype).values()])


# ---- host arithmetic against the reference -------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("j0", [0, 5 * 32 + 7])  # even: one hash per pair; odd: a pair straddles every group of 8
def test_host_arithmetic_matches_the_reference(host_check, dtype, j0):
    x = all_inputs(dtype)
    j = np.uint64(j0) + np.arange(x.size, dtype=np.uint64)
    scale, payload = SR.encode_blocks_sr(x, dtype, SR.rbits(KEY, j).reshape(x.shape))
    g_scale, g_payload = host_keyed(host_check, x, dtype, KEY, j0)
    assert np.array_equal(g_scale, scale)
    bad = np.nonzero((g_payload != payload).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], x[bad[:1]], g_payload[bad[:1]], payload[bad[:1]])
    assert (scale == 0xFF).sum() >= 3 and (scale == 0).sum() >= 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_arithmetic_under_explicit_r(host_check, dtype):
    x = all_inputs(dtype)
    rng = np.random.default_rng(7 + dtype)
    for r in (np.zeros(x.shape, np.uint32), np.full(x.shape, 0xFFFF, np.uint32),
              rng.integers(0, 1 << 16, x.shape).astype(np.uint32)):
        scale, payload = SR.encode_blocks_sr(x, dtype, r)
        g_scale, g_payload = host_explicit(host_check, x, dtype, r)
        assert np.array_equal(g_scale, scale)
        assert np.array_equal(g_payload, payload)


def test_index_wraps_as_uint32(host_check):
    x = random_blocks(F32, 4, 5)
    j0 = (1 << 32) - 64
    j = np.uint64(j0) + np.arange(x.size, dtype=np.uint64)
    scale, payload = SR.encode_blocks_sr(x, F32, SR.rbits(KEY, j).reshape(x.shape))
    g_scale, g_payload = host_keyed(host_check, x, F32, KEY, j0)
    assert np.array_equal(g_scale, scale) and np.array_equal(g_payload, payload)
    assert np.array_equal(SR.rbits(KEY, j[64:]), SR.rbits(KEY, np.arange(64, dtype=np.uint64)))


# ---- the rule's properties on the reference ------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_bytes_and_neighbouring_codes(dtype):
    x = all_inputs(dtype)
    rng = np.random.default_rng(17 + dtype)
    p_scale, p_payload = R.encode_blocks(x, dtype)
    lo_scale, lo_payload = SR.encode_blocks_sr(x, dtype, np.zeros(x.shape, np.uint32))
    hi_scale, hi_payload = SR.encode_blocks_sr(x, dtype, np.full(x.shape, 0xFFFF, np.uint32))
    scale, payload = SR.encode_blocks_sr(x, dtype, rng.integers(0, 1 << 16, x.shape))
    for s in (lo_scale, hi_scale, scale):
        assert np.array_equal(s, p_scale)  # the scale bytes are the plain encode's
    lo, hi, nib, plain = nibbles(lo_payload), nibbles(hi_payload), nibbles(payload), nibbles(p_payload)
    assert np.array_equal(lo & 8, nib & 8) and np.array_equal(hi & 8, nib & 8) and np.array_equal(plain & 8, nib & 8)
    assert ((hi & 7) - (lo & 7) <= 1).all() and ((hi & 7) >= (lo & 7)).all()
    for n in (nib, plain):  # every code is the floor code or the one above it
        assert (((n & 7) == (lo & 7)) | ((n & 7) == (hi & 7))).all()
    assert ((hi & 7) > (lo & 7)).sum() > x.size // 2 and ((nib != lo).any() and (nib != hi).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_table_truncates_and_rounds_up(dtype):
    t = B.table(dtype)
    x = t.values()
    scale, _ = R.encode_blocks(x, dtype)
    y = np.ldexp(np.abs(x), -(scale.astype(np.int64) - 127)[:, None])
    on_grid = np.isin(y, R.GRID)
    floor_code = np.searchsorted(R.GRID, y, side="right") - 1
    lo = nibbles(SR.encode_blocks_sr(x, dtype, np.zeros(x.shape, np.uint32))[1]) & 7
    hi = nibbles(SR.encode_blocks_sr(x, dtype, np.full(x.shape, 0xFFFF, np.uint32))[1]) & 7
    assert np.array_equal(lo, floor_code)                         # r = 0 truncates every row
    assert np.array_equal(hi[on_grid], floor_code[on_grid])       # grid values never move
    # r = 0xffff rounds every off-grid value with F >= 1 up; F = 0 off the grid (a fraction below
    # 2^-16 of a step) is truncated by the rule
    _, F, _ = SR.floor_code_and_fraction(y)
    assert np.array_equal(hi[F >= 1], floor_code[F >= 1] + 1)
    assert np.array_equal(hi[F == 0], floor_code[F == 0])
    # the boundaries themselves are the midpoints (their neighbours in T can be grid values where T is coarse)
    mid = (t.bnd >= 0) & (t.side == 0)
    assert (F[mid] == 32768).all() and mid.sum() > 300 and (F[t.bnd >= 0] >= 1).sum() > 1000


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_follow_the_plain_rules(dtype):
    mx = R.MAX_FINITE[dtype]
    x = np.zeros((4, 32))
    x[0, :] = -0.0
    x[1, 3], x[1, 4:] = np.nan, 2.0
    x[2, :4] = [np.inf, -np.inf, mx, -mx]
    x[2, 4:] = mx / 4
    x[3, :] = 1.0
    for r in (0, 0xFFFF, 0x1234):
        scale, payload = SR.encode_blocks_sr(x, dtype, np.full(x.shape, r, np.uint32))
        nib = nibbles(payload)
        p_scale, p_payload = R.encode_blocks(x, dtype)
        assert np.array_equal(scale, p_scale)
        assert (nib[0] == 8).all()                                   # -0 keeps its sign, code 0
        assert scale[1] == 0xFF and not payload[1].any()              # a NaN block
        # +-inf clamp to the largest finite T (just below 4 * 2^e): they encode as it does under the same r
        assert nib[2, 0] == nib[2, 2] and nib[2, 1] == nib[2, 3] and nib[2, 1] == nib[2, 0] | 8
        assert nib[2, 0] == (5 if r == 0 else 6)
        assert np.array_equal(nib[3], nibbles(p_payload)[3])          # 1.0 is on the grid
    # invalid elements count as +0
    t = NP.from_f32(np.full(96, 0.37, np.float32), dtype)
    buf = SR.compress_sr(t, dtype, 1, KEY, num_elem=40)
    sb = R.scale_bytes(96)
    assert buf[2] == 0 and not buf[sb + 32:sb + 48].any() and not buf[sb + 20:sb + 32].any() and buf[sb:sb + 20].all()


def decode64(scale, payload):
    nib = nibbles(payload)
    mag = R.GRID[nib & 7] * np.ldexp(1.0, scale.astype(np.int64) - 127)[:, None]
    return np.where(nib & 8, -mag, mag)


def steps_of(x, scale):
    y = np.ldexp(np.abs(x), -(scale.astype(np.int64) - 127)[:, None])
    return SR.floor_code_and_fraction(y)[2] * np.ldexp(1.0, scale.astype(np.int64) - 127)[:, None]


@pytest.mark.parametrize("K", [64, 1024])
def test_unbiased(K):
    """4096 f32 elements, K steps of one seed: every element's mean decode is within
    5 * step / (2 sqrt(K)) of x (a rounding has variance at most step^2 / 4); round-to-nearest
    fails the same bound at K = 1024"""
    rng = np.random.default_rng(2024)
    x = (rng.standard_normal(4096) * 1e-3).astype(np.float32).astype(np.float64).reshape(-1, 32)
    j = np.arange(x.size, dtype=np.uint64)
    acc = np.zeros(x.shape)
    for step in range(K):
        scale, payload = SR.encode_blocks_sr(x, F32, SR.rbits(SR.key(0x5EED, step), j).reshape(x.shape))
        acc += decode64(scale, payload)
    bound = 5.0 * steps_of(x, scale) / (2.0 * np.sqrt(K))
    worst = (np.abs(acc / K - x) / bound).max() * 5.0
    print(f"K={K}: worst element {worst:.2f} step / (2 sqrt(K)), bound 5")
    assert (np.abs(acc / K - x) <= bound).all()
    if K == 1024:
        rne = decode64(*R.encode_blocks(x, F32))
        assert (np.abs(rne - x) > bound).mean() > 0.5


def test_words_of_different_keys_do_not_correlate():
    j = np.arange(1 << 16, dtype=np.uint64)
    base = SR.rbits(SR.key(9, 4, 2, 0), j).astype(np.float64)
    assert abs(base.mean() / 65535.0 - 0.5) < 0.01
    others = {"rank": SR.key(9, 4, 3, 0), "stage": SR.key(9, 4, 2, 1), "step": SR.key(9, 5, 2, 0),
              "seed": SR.key(10, 4, 2, 0)}
    for what, k in others.items():
        c = abs(np.corrcoef(base, SR.rbits(k, j).astype(np.float64))[0, 1])
        print(f"{what}: |correlation| {c:.1e}")
        assert c < 0.02, what
    # neighbouring elements and the two halves of a word
    assert abs(np.corrcoef(base[:-1], base[1:])[0, 1]) < 0.02
    assert abs(np.corrcoef(base[0::2], base[1::2])[0, 1]) < 0.02


@pytest.mark.parametrize("p,cs", [(2, 4096), (4, 4096), (8, 2048)])
def test_time_averaged_error_against_the_plain_op(p, cs):
    """constant gradients: the time-averaged result's relative L2 error against the true mean falls
    with the steps and is below the plain op's from 16 steps on"""
    xs = OB.appendix_inputs(p, cs, F32)
    true = np.mean([x.astype(np.float64) for x in xs], axis=0)
    rel = lambda v: np.linalg.norm(v - true) / np.linalg.norm(true)  # noqa: E731
    plain = rel(R.centralized(xs, F32, True)[0].astype(np.float64))
    acc = np.zeros(p * cs)
    curve = {}
    for step in range(64):
        acc += SR.centralized_sr(xs, F32, True, 0xC0FFEE, step)[0].astype(np.float64)
        if step + 1 in (1, 4, 16, 32, 64):
            curve[step + 1] = rel(acc / (step + 1))
    print(f"p={p} cs={cs}: plain {plain:.4f}, stochastic " + ", ".join(f"{k}: {v:.4f}" for k, v in curve.items()))
    assert curve[16] < plain and curve[32] < plain and curve[64] < plain
    assert curve[1] > curve[4] > curve[16] > curve[64]
    assert curve[64] < 0.3 * curve[1]  # 1 / sqrt(64) = 0.125


def test_piece_count_and_chunking_do_not_change_the_words():
    """the payload of one tensor as 1 chunk and as 4 chunks is the same bytes"""
    rng = np.random.default_rng(3)
    n = 4 * 4096
    t = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    one = SR.compress_sr(t, F32, 1, KEY)
    four = SR.compress_sr(t, F32, 4, KEY)
    sb1, sb4, seg4 = R.scale_bytes(n), R.scale_bytes(n // 4), R.segment_bytes(n // 4)
    pay4 = np.concatenate([four[c * seg4 + sb4:(c + 1) * seg4] for c in range(4)])
    assert np.array_equal(one[sb1:], pay4)


# ---- the C-ABI surface ---------------------------------------------------------------------
def test_new_symbols_declared_and_exported(built):
    k_decl, c_decl = declared("bagua_kernels.h"), declared("bagua_core.h")
    k_exp = exported(os.path.join(LIB, "libbagua_kernels.so"))
    c_exp = exported(os.path.join(LIB, "libbagua_core.so"))
    assert not [n for n in KERNEL_SYMBOLS if n not in k_decl or n not in k_exp]
    assert not [n for n in CORE_SYMBOLS if n not in c_decl or n not in c_exp]
    from bagua_core import _native as N
    assert set(KERNEL_SYMBOLS) <= set(N.KERNEL_SIGNATURES) and set(CORE_SYMBOLS) <= set(N.CORE_SIGNATURES)
    assert N.BUCKET_OP_CENTRALIZED_MXFP4_STOCHASTIC == 7
    # appended: the layout of the older kinds is unchanged, the seed follows their last field
    assert [f[0] for f in N.bagua_bucket_op_t._fields_][-1] == "ef_server_scale"
    assert [f[0] for f in N.bagua_bucket_op_sr_t._fields_] == ["sr_seed"]
    assert N.bagua_bucket_op_sr_t.sr_seed.offset == ctypes.sizeof(N.bagua_bucket_op_t)
    assert ctypes.sizeof(N.bagua_bucket_op_sr_t) == ctypes.sizeof(N.bagua_bucket_op_t) + 8
    src = open(os.path.join(ROOT, "include", "bagua_core.h")).read()
    assert src.index("ef_server_scale;") < src.index("uint64_t sr_seed;") < src.index("} bagua_bucket_op_t;")


def test_key_and_word_equal_the_reference(built):
    from bagua_core import _native as N
    rng = np.random.default_rng(11)
    cases = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), ((1 << 64) - 1, (1 << 64) - 1, 16, 1)]
    cases += [(int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 64)),
               int(rng.integers(0, 2))) for _ in range(200)]
    keys = set()
    for seed, step, rank, stage in cases:
        k = N.K.bagua_mxfp4_sr_key(seed, step, rank, stage)
        assert k == SR.key(seed, step, rank, stage), (seed, step, rank, stage)
        keys.add(k)
    assert len(keys) == len(cases)
    pairs = np.concatenate([np.arange(64), rng.integers(0, 1 << 32, 500), [(1 << 32) - 1]]).astype(np.uint64)
    for k in (0, KEY, (1 << 64) - 1):
        want = SR.words(k, pairs)
        got = np.array([N.K.bagua_mxfp4_sr_word(k, int(q)) for q in pairs], np.uint32)
        assert np.array_equal(got, want)


def test_argument_checks(built):
    """refusals decided before any launch (the stand-in addresses are never dereferenced on the host)"""
    from bagua_core import _native as N
    ok = 1 << 20
    S = N.K.bagua_mxfp4_compressed_bytes(8192, 2)
    f, fr = N.K.bagua_mxfp4_compress_sr, N.K.bagua_mxfp4_compress_sr_range
    assert f(F32, None, 16384, 8192, 2, ok, S, -1, KEY, None) == 1          # null input
    assert f(F32, ok, 16384, 8192, 2, None, S, -1, KEY, None) == 1          # null output
    assert f(F32, ok, 16384, 8192, 2, ok, S - 1, -1, KEY, None) == 1        # short buffer
    assert f(F32, ok, 16384, 8192, 2, ok + 8, S, -1, KEY, None) == 1        # misaligned output
    assert f(F32, ok, 16384, 8192, 2, ok, S, 2, KEY, None) == 1             # target past the chunks
    assert fr(F32, ok, 16384, 8192, 2, ok, S, 64, 256, KEY, None) == 1      # a range off the granule
    assert fr(F32, ok, 16384, 8192, 2, ok, S, -1, -1, KEY, None) == 1
    assert fr(F32, ok, 16384, 8192, 2, ok, S, 128, 128, KEY, None) == 0     # an empty range: nothing launched
    g, gr = N.K.bagua_mxfp4_reduce_requantize_sr, N.K.bagua_mxfp4_reduce_requantize_sr_range
    assert g(F32, None, S, 8192, 2, 1, ok, S, 0, KEY, None) == 1
    assert g(F32, ok, S - 1, 8192, 2, 1, ok, S, 0, KEY, None) == 1
    assert g(F32, ok, S, 8192, 2, 1, ok + 8, S, 0, KEY, None) == 1
    assert g(F32, ok, S, 8192, 2, 1, ok, S, 2, KEY, None) == 1
    assert gr(F32, ok, S, 8192, 2, 1, ok, S, 0, 64, 256, KEY, None) == 1
    assert gr(F32, ok, S, 8192, 2, 1, ok, S, 0, 128, 128, KEY, None) == 0
    for dt in (3, 4, 5):                                                    # U8, I64, U64
        assert f(dt, ok, 16384, 8192, 2, ok, S, -1, KEY, None) == 4
        assert g(dt, ok, S, 8192, 2, 1, ok, S, 0, KEY, None) == 4
    S17 = N.K.bagua_mxfp4_compressed_bytes(1024, 17)
    assert g(F32, ok, S17, 1024, 17, 1, ok, S17, 0, KEY, None) == 4        # past 16 segments: composed by the caller
    assert gr(F32, ok, S17, 1024, 17, 1, ok, S17, 0, 0, 32, KEY, None) == 4


def test_python_refusals(built):
    import bagua_core
    r = bagua_core.MXFP4StochasticRounding(5)
    assert r.seed == 5 and bagua_core.MXFP4StochasticRounding((1 << 64) + 5).seed == 5
    with pytest.raises(TypeError):
        bagua_core.MXFP4StochasticRounding("5")
