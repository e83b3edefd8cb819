"""Planted extrema through pass 1 of the one-launch MinMax-UInt8 encode
(minmax_resident.hip): every region of a slice -- rows held early in VGPRs,
rows parked in LDS, rows held late, the streamed tiles and their ragged top
-- in the first, a middle and the last slice of a chunk, and the scalar head,
scalar tail and last vector that the last slice owns (it is 40 vectors short,
so its clamped duplicate loads are in play).  The minimum and the maximum of a
chunk always sit in different slices, so a header is right only if both the
fold and the exchange of the slices' partials are.  The input stays on the
device and only the planted elements are rewritten between launches; every
launch asserts that it takes the one-launch path and compares the whole
poisoned buffer with the C oracle, the header first, naming the planted
regions (tests/planted_cases.py).

Rows: each dtype's default row, the stream-last control row, one stack-order
row and both window-order rows; p = 1 and p = 8; the give-up path (exchange
timeout 0) and two launches back to back on one stream.
"""
import numpy as np
import pytest
import torch

import planted_cases as PC
from test_gpu_codec import BF16, F16, F32, to_dev
from test_gpu_resident import K, env, gpu_compress, small_threshold  # noqa: F401  (fixtures)
from test_gpu_resident_window import CONTROL_ROW, HEAD, WINDOW_ROWS, case_c, cu_count, geometry

pytestmark = pytest.mark.gpu

STACK_ROW = 24
SIGNED = {F32: np.int32, F16: np.int16, BF16: np.int16}
TORCH_INT = {F32: torch.int32, F16: torch.int16, BF16: torch.int16}

_base = {}


def shared_base(dtype, kind, n):
    """the latest (dtype, kind)'s base data at the largest size asked for so far; read-only"""
    key = (dtype, kind)
    if key not in _base or _base[key].size < n:
        _base.clear()
        _base[key] = np.resize(PC.base_data(dtype, kind, 1 << 22, 23), n)  # 4 Mi values, repeated
        _base[key].setflags(write=False)
    return _base[key][:n]


class Bucket:
    """p chunks of "case c" with two full streamed tiles on the device, at row `cfg`"""

    def __init__(self, K, cfg, dtype, kind, p):
        self.K, self.cfg, self.dtype, self.kind, self.p = K, cfg, dtype, kind, p
        # p = 1: a 96-element head and a 3-element tail; p = 8: + 76 elements keeps every
        # chunk eligible for both element sizes (test_gpu_resident_window.py special_input)
        self.cs = case_c(K, cfg, dtype, p, extra=HEAD + 3 if p == 1 else 76, tiles=2)
        self.base = shared_base(dtype, kind, p * self.cs)
        self.x = self.base.copy()
        self.xd = to_dev(self.base, dtype)
        assert self.xd.data_ptr() % 128 == 0
        S = K.bagua_minmax_u8_compressed_bytes(dtype, self.cs, p)
        block, re, h, rl, sb, _ = geometry(K, cfg)
        self.geom = [PC.resident(dtype, self.cs, c, cu_count() // p, (block, re, h, rl, sb), 0, 0, S // p)
                     for c in range(p)]
        self.pos = [PC.resident_positions(g) for g in self.geom]
        self.ref = None

    def plants(self, chunk, min_name, max_name):
        pos = self.pos[chunk]
        return [PC.Plant(chunk, pos[min_name][1], "min", min_name), PC.Plant(chunk, pos[max_name][1], "max", max_name)]

    def apply(self, plants, nan):
        """plants into the host copy and the device buffer; returns what to undo"""
        ed = PC.edits(self.dtype, self.kind, self.p, self.cs, plants, nan, lambda c: self.geom[c].j0)
        idx = np.array(sorted(ed), np.int64)
        bits = np.array([ed[i] for i in idx], PC.BITS[self.dtype])
        self.x.view(PC.BITS[self.dtype])[idx] = bits
        PC.check_plants(self.x, self.base, self.dtype, self.p, plants, changed=idx)
        self.write(idx, bits)
        return idx

    def write(self, idx, bits):
        self.xd.view(TORCH_INT[self.dtype])[torch.from_numpy(idx).cuda()] = torch.from_numpy(
            bits.view(SIGNED[self.dtype]).copy()).cuda()

    def undo(self, idx):
        self.x[idx] = self.base[idx]
        self.write(idx, self.base.view(PC.BITS[self.dtype])[idx])

    def launch(self, stream=None):
        out, keep = gpu_compress(self.K, self.xd, self.dtype, self.p, -1, stream=stream)  # asserts the path
        assert out.data_ptr() % 128 == 0  # the geometry's payload alignment
        return out, keep

    def expected(self, oracle_c, idx):
        """The C oracle's bytes for the current input.  The first call compresses the whole
        input.  A payload byte depends on its element and the chunk's header alone, so a later
        call compresses, per chunk, only the elements that differ from that first input (the
        plants among them): when the small chunk's header is the first input's, the oracle's
        bytes for those elements replace the first input's; otherwise the whole input again."""
        if self.ref is None:
            self.ref = (oracle_c.compress_minmax_u8(self.x, self.dtype, self.p), idx)
            return self.ref[0].copy()
        ref, ref_idx = self.ref
        want, co = ref.copy(), ref.size // self.p
        both = np.union1d(idx, ref_idx)
        for c in range(self.p):
            mine = both[(both >= c * self.cs) & (both < (c + 1) * self.cs)]
            if mine.size == 0:
                continue
            small = oracle_c.compress_minmax_u8(np.ascontiguousarray(self.x[mine]), self.dtype, 1)
            if not np.array_equal(small[:32], ref[c * co:c * co + 32]):
                return oracle_c.compress_minmax_u8(self.x, self.dtype, self.p)
            want[c * co + 32 + (mine - c * self.cs)] = small[32:32 + mine.size]
        return want

    def run(self, oracle_c, plants, nan, what):
        idx = self.apply(plants, nan)
        want = self.expected(oracle_c, idx)
        out, _ = self.launch()
        torch.cuda.synchronize()
        self.undo(idx)
        compare(out, want, self.dtype, self.p, plants, what)


def compare(out, want, dtype, p, plants, what):
    got = out.cpu().numpy()
    assert got.size == want.size
    PC.assert_headers(got, want, dtype, p, plants, what)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} payload, gap or slack bytes differ, first at {bad[:8]}"


def row_of(K, row, dtype):
    return K.bagua_minmax_u8_resident_default_cfg(dtype) if row == "default" else row


def row_cases():
    """(row, dtype, kind): each dtype's default row with every plant kind; the control row, a
    stack row and both window rows with f32 (margin) and bf16 (margin, ulp: the packed 16-bit
    halves); grouped so that cases share base data"""
    out = []
    for dtype in (F32, F16, BF16):
        for kind in PC.KINDS:
            out.append(("default", dtype, kind))
            if (dtype, kind) in ((F32, "margin"), (BF16, "margin"), (BF16, "ulp")):
                out += [(r, dtype, kind) for r in (CONTROL_ROW, STACK_ROW, *WINDOW_ROWS)]
    return out


def case_id(c):
    return f"row_{c[0]}-{PC.DTYPE_NAME[c[1]]}-{c[2]}"


@pytest.fixture
def case(K, env, request):
    row, dtype, kind = request.param
    cfg = row_of(K, row, dtype)
    env["BAGUA_RESIDENT_CFG"] = str(cfg)
    return cfg, dtype, kind


@pytest.mark.parametrize("case", row_cases(), indirect=True, ids=case_id)
def test_resident_eight_chunks_see_every_region(K, oracle_c, case):
    """p = 8, one plant pair per chunk and launch: every region takes both roles"""
    cfg, dtype, kind = case
    b = Bucket(K, cfg, dtype, kind, 8)
    every = {}  # the chunks' heads differ, so some have no scalar head or tail
    for pos in b.pos:
        every.update({n: v for n, v in pos.items() if n not in every})
    todo = PC.cross_slice_pairs(every)
    assert {n for n, _ in todo} == {n for _, n in todo} == set(every)
    launch = 0
    while todo:
        plants = []
        for c in range(8):  # the next pair that this chunk has both regions of
            pair = next((pr for pr in todo if pr[0] in b.pos[c] and pr[1] in b.pos[c]), None)
            if pair:
                todo.remove(pair)
                plants += b.plants(c, *pair)
        assert plants, f"no chunk has both regions of {todo[0]}"
        b.run(oracle_c, plants, nan=bool(launch & 1), what=f"row {cfg} {PC.DTYPE_NAME[dtype]} {kind} p=8 launch {launch}")
        launch += 1


P1_CASES = [("default", F32, "margin"), ("default", F16, "margin"), ("default", BF16, "margin"),
            (CONTROL_ROW, F32, "margin"), (STACK_ROW, F32, "margin"), (WINDOW_ROWS[0], BF16, "margin")]


@pytest.mark.parametrize("case", P1_CASES, indirect=True, ids=case_id)
def test_resident_one_chunk_sees_every_region(K, oracle_c, case):
    """p = 1: all workgroups on one chunk, a scalar head and a scalar tail; one pair per launch,
    every region in at least one role (in both with p = 8)"""
    cfg, dtype, kind = case
    b = Bucket(K, cfg, dtype, kind, 1)
    assert {"scalar_head_first", "scalar_head_last", "scalar_tail_first", "scalar_tail_last"} <= set(b.pos[0])
    pairs = PC.cross_slice_pairs(b.pos[0])
    seen, n = set(), 0
    for mn, mx in pairs:
        if mn in seen and mx in seen:
            continue
        seen |= {mn, mx}
        b.run(oracle_c, b.plants(0, mn, mx), nan=bool(n & 1), what=f"row {cfg} {PC.DTYPE_NAME[dtype]} {kind} p=1")
        n += 1
    assert seen == set(b.pos[0])


GIVE_UP_CASES = [("default", F32, "margin"), ("default", F16, "margin"), ("default", BF16, "margin"),
                 (CONTROL_ROW, BF16, "margin"), (STACK_ROW, F32, "margin"), (WINDOW_ROWS[0], F32, "margin")]


@pytest.mark.parametrize("case", GIVE_UP_CASES, indirect=True, ids=case_id)
def test_resident_give_up_path_sees_every_slice(K, oracle_c, env, case):
    """exchange timeout 0: whichever slices a workgroup re-reads instead of taking their
    published partials, the bytes are the oracle's.  The extrema sit in the first, a middle
    and the last slice, and in the scalars the last slice owns."""
    cfg, dtype, kind = case
    env["BAGUA_RESIDENT_TIMEOUT_US"] = "0"
    b = Bucket(K, cfg, dtype, kind, 8)
    names = ["slice_first_parked_last_row", "slice_last_streamed_tile1_last_lane", "slice_middle_early_first_row",
             "scalar_head_first", "slice_first_streamed_tile0_lane0", "slice_last_ragged_top_lane0",
             "slice_middle_ragged_top_last_lane", "chunk_last_vector"]  # neighbours lie in different slices

    def have(c, name):  # a chunk that starts on a line has no scalar head
        return name if name in b.pos[c] else "slice_last_early_last_row"
    plants = [pl for c in range(8) for pl in b.plants(c, have(c, names[c]), have(c, names[(c + 1) % 8]))]
    b.run(oracle_c, plants, nan=True, what=f"row {cfg} {PC.DTYPE_NAME[dtype]} give-up path")


@pytest.mark.parametrize("case", [("default", F32, "margin"), ("default", BF16, "ulp")], indirect=True, ids=case_id)
def test_resident_back_to_back_launches_do_not_share_partials(K, oracle_c, case):
    """Two launches on one stream, the second queued behind the first, with the extrema in
    different slices: the second must not take the first one's partials.  Two inputs, so
    that nothing is rewritten between the launches."""
    cfg, dtype, kind = case
    b1 = Bucket(K, cfg, dtype, kind, 1)
    b2 = Bucket(K, cfg, dtype, kind, 1)
    pl1 = b1.plants(0, "slice_first_early_first_row", "slice_last_streamed_tile1_last_lane")
    pl2 = b2.plants(0, "slice_middle_parked_first_row", "slice_first_ragged_top_last_lane")
    i1, i2 = b1.apply(pl1, False), b2.apply(pl2, False)
    torch.cuda.synchronize()
    (o1, k1), (o2, k2) = b1.launch(), b2.launch()
    torch.cuda.synchronize()
    w1 = oracle_c.compress_minmax_u8(b1.x, dtype, 1)
    w2 = oracle_c.compress_minmax_u8(b2.x, dtype, 1)
    assert PC.header_bits(w1, dtype, 1, 0) == PC.header_bits(w2, dtype, 1, 0)  # same values, other slices
    compare(o1, w1, dtype, 1, pl1, "first launch")
    compare(o2, w2, dtype, 1, pl2, "second launch")
    # and with the second input's extrema gone, a stale partial of either launch would show
    b2.undo(i2)
    o3, _ = b2.launch()
    torch.cuda.synchronize()
    compare(o3, oracle_c.compress_minmax_u8(b2.x, dtype, 1), dtype, 1, [], "third launch, nothing planted")
