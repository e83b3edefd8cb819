"""GPU parity of the window-order rows of the one-launch MinMax-UInt8 encode
(minmax_resident.hip, minmax_resident_encode_kernel_window) and of their stream-last
control row.

A slice of a chunk is rows of BLOCK vectors: rows [0, RE) are held early in VGPRs,
rows [RE, RE + H) parked in LDS, rows [RE + H, RE + H + RL) held late in the
registers of the streaming buffers, the rest streamed in tiles of SB rows with a
ragged top tile.  The shapes are derived from the row's geometry
(bagua_minmax_u8_resident_cfg_geometry, bagua_minmax_u8_resident_cfg_order) and the
CU count G: every slice of a chunk but the last has the same whole number of rows,
and the last one is `short` vectors shorter.  Every case compares every byte of the
compressed buffer with the C oracle.

  slice lengths (every window row, f32 and bf16; p = 1, a 96-element scalar head):
     fewer rows than RE (2^22 elements)
     RE + H                       nothing held late, nothing streamed
     RE + H + 1, RE + H + RL - 1  the late rows partly present
     RE + H + RL                  nothing streamed
     ... + SB                     one full tile, no ragged top
     ... + SB + 1, last slice BLOCK - 1 vectors short: its ragged top is one vector
     ... + 2 SB, last slice one vector short: a ragged top of SB * BLOCK - 1 vectors
     ... + SB + 3, last slice 40 vectors short (case c below)
  on the first and the last window row, f32 and bf16:
     case c split into chunks with scalar heads and tails
     NaN, +-inf, -0, denormals, an all-NaN chunk and a constant chunk (three full tiles)
     a zero exchange timeout (the give-up path)
     back-to-back launches on one stream, and one launch on each of two streams
  one graph replay (the first window row)
  every window row is in WINDOW_ROWS; no default row uses scratch
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_codec import BF16, F16, F32, to_dev
from test_gpu_resident import K, env, gpu_compress, make_input, small_threshold  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NVEC = {F32: 4, F16: 8, BF16: 8}  # elements per 16-byte vector
CONTROL_ROW = 30                   # stream-last at the window rows' R and SB
WINDOW_ROWS = [31, 32]
EDGE_ROWS = [WINDOW_ROWS[0], WINDOW_ROWS[-1]]
HEAD = 96  # scalar head of a chunk whose input and output buffers are 128-byte aligned


def geometry(K, cfg):
    """(block, re, h, rl, sb, order) of a row; rl = 0 unless order == 2 (window)."""
    v = [ctypes.c_int(0) for _ in range(5)]
    assert K.bagua_minmax_u8_resident_cfg_geometry(cfg, *[ctypes.byref(x) for x in v]) == 0
    order, rl = ctypes.c_int(-1), ctypes.c_int(-1)
    assert K.bagua_minmax_u8_resident_cfg_order(cfg, ctypes.byref(order), ctypes.byref(rl)) == 0
    block, r, h, sb, _ = (x.value for x in v)
    return block, r, h, rl.value, sb, order.value


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


_inputs = {}


def shared_input(n, dtype, seed):
    """One host array per (dtype, seed), generated once at the largest size asked for so far;
    shorter cases take a prefix.  Never written to."""
    key = (dtype, seed)
    if key not in _inputs or _inputs[key].size < n:
        _inputs[key] = make_input(n, dtype, seed)
    return _inputs[key][:n]


def elements(K, cfg, dtype, rows, short=0, p=1, extra=0):
    """Elements of one of p chunks whose slices have `rows` rows each, the last one `short`
    vectors (and the chunk's scalar head) shorter, plus `extra` elements."""
    block = geometry(K, cfg)[0]
    bpc = cu_count() // p
    assert 0 <= short < block * rows
    return NVEC[dtype] * (bpc * rows * block - short) + extra


def case_c(K, cfg, dtype, p=1, extra=HEAD, tiles=1):
    """Every region and the ragged top: RE + H + RL rows, `tiles` full tiles and 3 ragged rows per
    slice; 40 vectors come off the last slice, which stays inside its ragged top."""
    block, re, h, rl, sb, _ = geometry(K, cfg)
    return elements(K, cfg, dtype, re + h + rl + tiles * sb + 3, short=40, p=p, extra=extra)


def check(K, oracle_c, x, dtype, p, target=-1):
    xt = to_dev(x, dtype)
    assert xt.data_ptr() % 128 == 0
    got_t, _ = gpu_compress(K, xt, dtype, p, target)
    torch.cuda.synchronize()
    got = got_t.cpu().numpy()
    want = oracle_c.compress_minmax_u8(x, dtype, p, target)
    if target >= 0:
        co = got.size // p
        got, want = got[target * co:(target + 1) * co], want[target * co:(target + 1) * co]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"


@pytest.fixture
def row(env, request):
    cfg = request.node.callspec.params["cfg"]
    env["BAGUA_RESIDENT_CFG"] = str(cfg)
    return cfg


def slice_rows(name, re, h, rl, sb, block):
    """(rows per slice, vectors the last slice is short) of the named slice-length case."""
    on_chip = re + h + rl
    return {
        "on_chip_without_late": (re + h, 0),
        "one_late_row": (re + h + 1, 0),
        "all_but_one_late_row": (re + h + rl - 1, 0),
        "nothing_streamed": (on_chip, 0),
        "one_full_tile": (on_chip + sb, 0),
        "ragged_top_of_one_vector": (on_chip + sb + 1, block - 1),
        "ragged_top_one_vector_short_of_a_tile": (on_chip + 2 * sb, 1),
        "ragged_top_of_three_rows": (on_chip + sb + 3, 40),
    }[name]


SLICE_CASES = ["on_chip_without_late", "one_late_row", "all_but_one_late_row", "nothing_streamed", "one_full_tile",
               "ragged_top_of_one_vector", "ragged_top_one_vector_short_of_a_tile", "ragged_top_of_three_rows"]


def test_window_rows_are_the_listed_ones(K):
    """Every committed window row is in WINDOW_ROWS (so it runs below); the control row is
    stream-last with the first window row's SB."""
    found, cfg = [], 0
    order, rl = ctypes.c_int(-1), ctypes.c_int(-1)
    while K.bagua_minmax_u8_resident_cfg_order(cfg, ctypes.byref(order), ctypes.byref(rl)) == 0:
        if order.value == 2:
            assert rl.value > 0
            found.append(cfg)
        else:
            assert rl.value == 0
        cfg += 1
    assert found == WINDOW_ROWS
    assert geometry(K, CONTROL_ROW)[5] == 0
    assert geometry(K, CONTROL_ROW)[4] == geometry(K, WINDOW_ROWS[0])[4]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cfg", WINDOW_ROWS + [CONTROL_ROW])
def test_window_slices_shorter_than_early_rows(K, oracle_c, row, cfg, dtype):
    block, re, h, rl, sb, _ = geometry(K, cfg)
    n = 1 << 22
    assert n // NVEC[dtype] // cu_count() < re * block
    check(K, oracle_c, shared_input(n, dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", SLICE_CASES)
@pytest.mark.parametrize("cfg", WINDOW_ROWS)
def test_window_slice_lengths(K, oracle_c, row, cfg, case, dtype):
    block, re, h, rl, sb, order = geometry(K, cfg)
    assert order == 2
    rows, short = slice_rows(case, re, h, rl, sb, block)
    n = HEAD + elements(K, cfg, dtype, rows, short)
    check(K, oracle_c, shared_input(n, dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_control_row_all_regions_and_ragged_top(K, oracle_c, env, dtype):
    env["BAGUA_RESIDENT_CFG"] = str(CONTROL_ROW)
    block, r, h, _, sb, _ = geometry(K, CONTROL_ROW)
    n = HEAD + elements(K, CONTROL_ROW, dtype, r + h + sb + 3, short=40)
    check(K, oracle_c, shared_input(n, dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("p,target,extra", [(8, -1, 76), (4, 2, 76), (3, -1, 77)])
@pytest.mark.parametrize("cfg", EDGE_ROWS)
def test_window_chunks_with_scalar_heads_and_tails(K, oracle_c, row, cfg, dtype, p, target, extra):
    """Case c per chunk, with the (p, target, extra) triples of the stack-order tests: every chunk
    has a scalar head, and a scalar tail where the chunk size allows one (see
    test_stack_chunks_with_scalar_heads_and_tails)."""
    cs = case_c(K, cfg, dtype, p, extra=extra)
    check(K, oracle_c, shared_input(p * cs, dtype, seed=11), dtype, p, target)


def special_input(K, cfg, dtype):
    """Eight chunks of case c with three full tiles: NaN, +-inf, -0, +0 and denormals spread over every
    region of chunk 0; chunk 1 all NaN; chunk 2 constant; chunk 3 finite with -0; the rest plain.
    (p = 8 with + 76 elements is admissible for both dtypes with every chunk active; p = 4 is not
    for the 16-bit ones.)"""
    p = 8
    cs = case_c(K, cfg, dtype, p, extra=76, tiles=3)
    x = shared_input(p * cs, dtype, seed=12).copy()
    f = x if dtype != BF16 else None

    def put(idx, value):
        if dtype == BF16:
            x[idx] = (np.array(value, np.float32).reshape(-1).view(np.uint32) >> 16).astype(np.uint16)
        else:
            f[idx] = value

    rng = np.random.default_rng(5)
    idx = rng.integers(0, cs, 4096)
    put(idx[0::6], np.float32(np.nan))
    put(idx[1::6], np.float32(np.inf))
    put(idx[2::6], np.float32(-np.inf))
    put(idx[3::6], np.float32(-0.0))
    put(idx[4::6], np.float32(0.0))
    put(idx[5::6], np.float32(1e-40))
    put(slice(cs, 2 * cs), np.float32(np.nan))
    put(slice(2 * cs, 3 * cs), np.float32(0.37))
    put(3 * cs + idx[:64], np.float32(-0.0))
    return x, p


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cfg", EDGE_ROWS)
def test_window_specials(K, oracle_c, row, cfg, dtype):
    x, p = special_input(K, cfg, dtype)
    with np.errstate(all="ignore"):
        check(K, oracle_c, x, dtype, p)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cfg", EDGE_ROWS)
def test_window_give_up_path(K, oracle_c, env, row, cfg, dtype):
    env["BAGUA_RESIDENT_TIMEOUT_US"] = "0"
    check(K, oracle_c, shared_input(case_c(K, cfg, dtype), dtype, seed=11), dtype, 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cfg", EDGE_ROWS)
def test_window_back_to_back_and_two_streams(K, oracle_c, row, cfg, dtype):
    n = case_c(K, cfg, dtype)
    xs = [shared_input(n, dtype, seed=11), shared_input(n, dtype, seed=13)]
    xts = [to_dev(x, dtype) for x in xs]
    s1, s2 = torch.cuda.current_stream(), torch.cuda.Stream()
    s2.wait_stream(s1)  # the inputs were copied on s1
    outs = []
    # two launches back to back on s1 (tags advance on its slot), then one launch on each of two
    # streams (separate slots); gpu_compress fills its output buffer on the current stream, so
    # each launch is issued with its own stream current
    for i, st in ((0, s1), (1, s1), (0, s1), (1, s2)):
        with torch.cuda.stream(st):
            out, keep = gpu_compress(K, xts[i], dtype, 1, -1, stream=st)
        outs.append((i, out, keep))
    torch.cuda.synchronize()
    want = [oracle_c.compress_minmax_u8(x, dtype, 1) for x in xs]
    for i, out, _ in outs:
        assert np.array_equal(out.cpu().numpy(), want[i])
    assert K.bagua_minmax_u8_release_stream(ctypes.c_void_p(s2.cuda_stream)) == 0


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_window_graph_replay(K, oracle_c, env, dtype):
    """One captured launch of the first window row, replayed once on new input."""
    cfg = WINDOW_ROWS[0]
    env["BAGUA_RESIDENT_CFG"] = str(cfg)
    n = case_c(K, cfg, dtype)
    xs = [shared_input(n, dtype, seed=11), shared_input(n, dtype, seed=13)]
    xt = to_dev(xs[0], dtype)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    sp = ctypes.c_void_p(st.cuda_stream)
    S = K.bagua_minmax_u8_compressed_bytes(dtype, n, 1)
    out = torch.full((S,), 0xA5, dtype=torch.uint8, device="cuda")
    wsb = K.bagua_minmax_u8_workspace_bytes(n, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    args = (dtype, xt.data_ptr(), n, n, 1, out.data_ptr(), S, ws.data_ptr(), wsb, -1, sp)
    assert K.bagua_minmax_u8_resident_path(dtype, xt.data_ptr(), n, n, 1, out.data_ptr(), S, -1, sp) == 1
    torch.cuda.synchronize()
    assert K.bagua_minmax_u8_compress(*args) == 0  # outside capture: one-time attribute / occupancy setup
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        rc = K.bagua_minmax_u8_compress(*args)
    assert rc == 0
    xt.copy_(to_dev(xs[1], dtype))
    out.fill_(0xA5)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), oracle_c.compress_minmax_u8(xs[1], dtype, 1))
    assert K.bagua_minmax_u8_release_stream(sp) == 0


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_default_rows_use_no_scratch_and_report_their_order(K, dtype):
    cfg = K.bagua_minmax_u8_resident_default_cfg(dtype)
    regs, scratch = ctypes.c_int(-1), ctypes.c_int(-1)
    assert K.bagua_minmax_u8_resident_cfg_info(dtype, cfg, ctypes.byref(regs), ctypes.byref(scratch)) == 0
    order = geometry(K, cfg)[5]
    print(f"dtype {dtype} default row {cfg}: order {order}, {regs.value} registers, {scratch.value} scratch bytes")
    assert order in (0, 1, 2)
    assert 0 < regs.value <= 512
    assert scratch.value == 0, (cfg, scratch.value)
