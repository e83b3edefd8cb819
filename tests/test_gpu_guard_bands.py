"""Guard-band tests of every MX entry of the kernel ABI (include/bagua_kernels.h): MXFP4, MXFP6 and MXFP8,
their error-feedback, stochastic-rounding, block-range and ring kernels, called through bc._native.K with raw
pointers into an arena (tests/guard_arena.py) whose every buffer ends exactly where the next byte is poison.

Every call runs under both poisons and asserts (a) status OK and the arena clean: no byte outside a writable
buffer changed, no input changed; (b) every output equals the numpy reference the codec's own tests use,
segments with their slack, tensors and residuals by bits; (c) the outputs of the "hash" and the "ones" run are
identical, so no result depends on a byte outside a buffer (under "ones" such a byte is a NaN or the NaN
scale byte).  A stray access that only reads and does not change the result is not seen.

Placement.  Tensors (gradient, decode output, the middle step's stored chunk, the ring's t / W / L / R) lie
16 B past a multiple of 256 (the vector path, not 32-B aligned) and one element further (the guarded path; the
ring entries refuse such a tensor, which is asserted together with nothing having been written).  Segments lie
at exactly the alignment the header asks for: encode and middle-step buffers 16 B, decode and ring-apply inputs
8 B (MXFP6, MXFP8) or 4 B (MXFP4), residuals 4 B and 16 B.

Shapes are the smallest with a tail: chunks of 1, 33, 65 and 127 elements (1 to 4 blocks, the MXFP6 payload
slacks 8, 16, 24 and 0 B) and one encode wave tile plus a block plus 5, as 1 and 3 chunks (with an odd size
chunks 2 and 3 start misaligned); TABLE lists the entries and the test that drives each."""
import collections
import contextlib
import types

import numpy as np
import pytest
import torch

import mxfp4_ef_reference as EF4
import mxfp4_reference as R4
import mxfp4_sr_reference as SR4
import mxfp6_ef_reference as EF6
import mxfp6_reference as R6
import mxfp8_ef_reference as EF8
import mxfp8_reference as R8
import mxfp8_sr_reference as SR8
from guard_arena import POISONS, Arena
from oracle import oracle_np as NP
from test_gpu_codec import assert_float_bits_equal
from test_gpu_mxfp8 import grads, hostile_inputs, same_bytes
from test_mxfp4_ring_cpu import mixed_reference

pytestmark = pytest.mark.gpu

F32, F16, BF16 = DTYPES = [0, 1, 2]
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
ESIZE = {F32: 4, F16: 2, BF16: 2}
FILL = 0xA5
DEVICE = "cuda"
ENCODE_WAVE = {F32: 2048, F16: 4096, BF16: 4096}    # elements of an encode wave's tile (8 KiB of input)
DECODE_GROUP = {F32: 4096, F16: 8192, BF16: 8192}   # elements of a decode workgroup's iteration
RING_WAVE = {F32: 512, F16: 1024, BF16: 1024}       # elements of a ring kernel's wave tile
MIDDLE_GROUP = 8192                                 # elements of a middle-step workgroup's iteration
EF_TILE = 2048                                      # elements of the worker step's wave tile, every dtype

Codec = collections.namedtuple("Codec", "bits R EF SR knob block_bytes decode_align")
CODECS = {4: Codec(4, R4, EF4, SR4, "MX", 16, 4), 6: Codec(6, R6, EF6, None, "MX6", 24, 8),
          8: Codec(8, R8, EF8, SR8, "MX8", 32, 8)}
SR_CODECS = [4, 8]

# ------------------------------------------------------------------ table ----
Row = collections.namedtuple("Row", "entry test")


def _table():
    rows = []
    for c in CODECS.values():
        m = f"bagua_mxfp{c.bits}_"
        rows += [Row(m + "compress", "test_compress_and_decompress"), Row(m + "decompress", "test_compress_and_decompress"),
                 Row(m + "compress_ef", "test_compress_ef"),
                 Row(m + "reduce_requantize", "test_middle_steps"), Row(m + "reduce_requantize_ef", "test_middle_steps"),
                 Row(m + "compress_range", "test_range_entries"), Row(m + "decompress_range", "test_range_entries"),
                 Row(m + "reduce_requantize_range", "test_range_entries")]
        if c.SR:
            rows += [Row(m + "compress_sr", "test_compress_sr"), Row(m + "reduce_requantize_sr", "test_middle_steps"),
                     Row(m + "compress_sr_range", "test_range_entries"),
                     Row(m + "reduce_requantize_sr_range", "test_range_entries")]
        rows += [Row(f"bagua_ring_{k}_mxfp{c.bits}", "test_ring") for k in ("mix", "apply", "one_rank")]
    # host arithmetic behind the stochastic entries: they give the key every _sr row runs under, and run
    # beside a live arena, which must stay clean
    rows += [Row("bagua_mxfp4_sr_key", "test_compress_sr"), Row("bagua_mxfp4_sr_word", "test_compress_sr")]
    return rows


TABLE = _table()


def entry(K, name, test):
    """the C entry of a table row; a row that is not in the table is not run"""
    assert Row(name, test) in TABLE, f"{name}: no row for {test}"
    return getattr(K, name)


# ---------------------------------------------------------------- harness ----
Buf = collections.namedtuple("Buf", "name data align phase readonly")


def ro(name, data, align, phase):
    return Buf(name, data, align, phase, True)


def rw(name, data, align, phase):
    return Buf(name, data, align, phase, False)


def fill(nbytes):
    return np.full(nbytes, FILL, np.uint8)


def tensor_phases(dtype):
    return 16, 16 + ESIZE[dtype]


def guarded(call, bufs, want, what, rc=OK, floats=None):
    """`call` (buffer name -> pointer; returns the status) under both poisons: (a), (b) against `want` (name ->
    expected array; a writable buffer that is not named must keep its bytes; names in `floats`: tensors that may
    hold NaN, compared as the codecs' tests compare them) and (c)"""
    got = {}
    for poison in POISONS:
        arena = Arena(poison, DEVICE)
        placed = {b.name: arena.place(b.name, b.data.nbytes, b.align, b.phase, b.readonly).write(b.data) for b in bufs}
        status = call({k: v.ptr for k, v in placed.items()})
        torch.cuda.synchronize()
        assert status == rc, f"{what} [{poison}]: status {status}"
        arena.check(what)
        got[poison] = {b.name: placed[b.name].read() for b in bufs if not b.readonly}
        for b in bufs:
            if b.readonly:
                continue
            w = np.ascontiguousarray(want.get(b.name, b.data))
            if floats and b.name in floats:
                assert_float_bits_equal(got[poison][b.name].view(w.dtype), w, floats[b.name], f"{what} [{poison}]: {b.name}")
            else:
                same_bytes(got[poison][b.name], w, f"{what} [{poison}]: {b.name}")
    for name in got["hash"]:
        same_bytes(got["hash"][name], got["ones"][name], f"{what}: {name} differs between the two poisons")
    return got["hash"]


@contextlib.contextmanager
def composed(c):
    """the module with the middle step and the composed ring op of codec c: for MXFP6 mxfp8_reference's over
    that codec's compress and decompress, as the fixture of tests/test_gpu_mxfp6.py arranges it"""
    with pytest.MonkeyPatch.context() as m, np.errstate(all="ignore"):
        if c.bits == 6:
            m.setattr(R8, "compress", R6.compress)
            m.setattr(R8, "decompress", R6.decompress)
        yield R4 if c.bits == 4 else R8


def received(c, rng, p, cs, dtype):
    """the hostile segments of the codec's own middle-step tests (a NaN block; on f16 a sum past the range)"""
    import test_gpu_mxfp4
    import test_gpu_mxfp6
    import test_gpu_mxfp8
    return {4: test_gpu_mxfp4, 6: test_gpu_mxfp6, 8: test_gpu_mxfp8}[c.bits].received(rng, p, cs, dtype)


def step_grads(rng, n, dtype):
    from test_gpu_mxfp8_ef import step_grads as g
    return g(rng, n, dtype)


def state(rng, n):
    """a residual as some earlier step left it"""
    return (rng.standard_normal(n) * 1e-4).astype(np.float32)


def chunk_sizes(dtype):
    return [1, 33, 65, 127, ENCODE_WAVE[dtype] + 37]


def sr_key(K, c, step):
    key = entry(K, "bagua_mxfp4_sr_key", "test_compress_sr")(0xB0A0 + c.bits, step, 1, 0)
    assert key == SR4.key(0xB0A0 + c.bits, step, 1, 0)
    return key


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


def knobs(c):
    return ([f"BAGUA_TUNE_{c.knob}_{k}_BLOCKS" for k in ("ENCODE", "DECODE", "MIDDLE")]
            + [f"BAGUA_TUNE_{c.knob}_RING_{k}_BLOCKS" for k in ("MIX", "APPLY", "ONE_RANK")])


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for c in CODECS.values():
        for k in knobs(c):
            monkeypatch.delenv(k, raising=False)


# ------------------------------------------------- encode and decode ----
def check_compress(K, c, dtype, x, p, what, phase, num_elem=None, target=-1, key=None):
    """bagua_mxfpN_compress, or _compress_sr under `key`; the input buffer holds exactly num_elem elements"""
    cs, n = x.size // p, x.size if num_elem is None else num_elem
    S = c.R.compressed_bytes(cs, p)
    with np.errstate(all="ignore"):
        if key is None:
            fn = entry(K, f"bagua_mxfp{c.bits}_compress", "test_compress_and_decompress")
            want = c.R.compress(x, dtype, p, target, out=fill(S), num_elem=num_elem)
        else:
            fn = entry(K, f"bagua_mxfp{c.bits}_compress_sr", "test_compress_sr")
            want = c.SR.compress_sr(x, dtype, p, key, target, out=fill(S), num_elem=num_elem)
    tail = () if key is None else (key,)
    for ph in phase:
        guarded(lambda q: fn(dtype, q["x"], n, cs, p, q["out"], S, target, *tail, None),
                [ro("x", x[:n], ESIZE[dtype], ph), rw("out", fill(S), 16, 16)], {"out": want}, f"{what} phase {ph}")
    return want


def check_decompress(K, c, dtype, comp, p, cs, what, phase):
    fn = entry(K, f"bagua_mxfp{c.bits}_decompress", "test_compress_and_decompress")
    with np.errstate(all="ignore"):
        want = c.R.decompress(comp, p, np.zeros(p * cs, c.R.STORAGE[dtype]), dtype)
    for ph in phase:
        guarded(lambda q: fn(dtype, q["in"], comp.size, cs, p, q["out"], None),
                [ro("in", comp, c.decode_align, c.decode_align), rw("out", fill(p * cs * ESIZE[dtype]), ESIZE[dtype], ph)],
                {"out": want}, f"{what} phase {ph}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", CODECS)
def test_compress_and_decompress(bc, bits, dtype):
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(10 * bits + dtype)
    both = tensor_phases(dtype)
    for cs in chunk_sizes(dtype):
        for p in (1, 3):
            x, what = grads(rng, p * cs, dtype), f"cs={cs} p={p}"
            comp = check_compress(K, c, dtype, x, p, what + " encode", both)
            check_decompress(K, c, dtype, comp, p, cs, what + " decode", both)
        for target in (0, 2):  # one target chunk: the written segment is the first or the last thing in the buffer
            check_compress(K, c, dtype, x, 3, f"cs={cs} target={target}", both[:1], target=target)
    x = grads(rng, 3 * 1000, dtype)  # partly valid: what lies past the valid count is the band itself
    for num_elem in (1000 + 517, 5, 0):
        check_compress(K, c, dtype, x, 3, f"num_elem={num_elem}", both, num_elem=num_elem)
    cases, p = hostile_inputs(dtype)  # NaN, +-Inf, the largest finite, -0, denormals, a zero chunk, one huge element
    for name, x in cases.items():
        comp = check_compress(K, c, dtype, x, p, name + " encode", both[1:])
        check_decompress(K, c, dtype, comp, p, x.size // p, name + " decode", both[1:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", CODECS)
def test_compress_ef(bc, bits, dtype):
    """every gradient phase under a residual 4 B off a vector and on one"""
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(100 + 10 * bits + dtype)
    fn = entry(K, f"bagua_mxfp{bits}_compress_ef", "test_compress_ef")
    for cs in chunk_sizes(dtype):
        for p in (1, 3):
            n, S = p * cs, c.R.compressed_bytes(cs, p)
            x, res = step_grads(rng, n, dtype), state(rng, n)
            after = res.copy()
            want = c.EF.compress_ef(x, dtype, p, types.SimpleNamespace(residual=after))
            for ph in tensor_phases(dtype):
                for rph in (4, 16):
                    guarded(lambda q: fn(dtype, q["x"], n, cs, p, q["out"], S, -1, q["residual"], None),
                            [ro("x", x, ESIZE[dtype], ph), rw("out", fill(S), 16, 16), rw("residual", res, 4, rph)],
                            {"out": want, "residual": after}, f"cs={cs} p={p} phase {ph} residual phase {rph}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", SR_CODECS)
def test_compress_sr(bc, bits, dtype):
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(200 + 10 * bits + dtype)
    key, both = sr_key(K, c, 3), tensor_phases(dtype)
    pairs = np.array([0, 1, 2, 0x7FFFFFFF, 0xFFFFFFFF], np.uint64)
    word = entry(K, "bagua_mxfp4_sr_word", "test_compress_sr")
    assert [word(key, int(j)) for j in pairs] == SR4.words(key, pairs).tolist()
    for cs in chunk_sizes(dtype):
        for p in (1, 3):
            x = grads(rng, p * cs, dtype)
            check_compress(K, c, dtype, x, p, f"cs={cs} p={p}", both, key=key)
        check_compress(K, c, dtype, x, 3, f"cs={cs} target=2", both[:1], target=2, key=key)
    x = grads(rng, 3 * 1000, dtype)
    for num_elem in (1000 + 517, 5, 0):
        check_compress(K, c, dtype, x, 3, f"num_elem={num_elem}", both, num_elem=num_elem, key=key)


# ------------------------------------------------------------ middle steps ----
def check_middle(K, c, dtype, recv, p, cs, target, average, what, rng, store_phases, residual_phase, key):
    """the plain step storing the reduced chunk (at each phase) and not, the step with error feedback and,
    where the codec has it, the stochastic one, on the same received segments"""
    S, seg, es = recv.size, recv.size // p, ESIZE[dtype]
    head = [ro("in", recv, 16, 16), rw("out", fill(S), 16, 16)]
    with composed(c) as M:
        want, reduced = M.reduce_requantize(recv, p, cs, dtype, target, bool(average), out=fill(S))
    fn = entry(K, f"bagua_mxfp{c.bits}_reduce_requantize", "test_middle_steps")
    before = NP.from_f32(np.full(p * cs, 5.0, np.float32), dtype)
    stored = before.copy()
    stored[target * cs:(target + 1) * cs] = reduced[target * cs:(target + 1) * cs]
    for ph in store_phases:
        guarded(lambda q: fn(dtype, q["in"], S, cs, p, q["tensor"], average, q["out"], S, target, None),
                head + [rw("tensor", before, es, ph)], {"out": want, "tensor": stored}, f"{what} stored at phase {ph}",
                floats={"tensor": dtype})
    guarded(lambda q: fn(dtype, q["in"], S, cs, p, None, average, q["out"], S, target, None), head, {"out": want},
            f"{what} not stored")
    res = state(rng, cs)
    after, want = res.copy(), fill(S)
    with np.errstate(all="ignore"):
        want[target * seg:(target + 1) * seg] = c.EF.middle_ef(NP, recv, p, cs, dtype, target, bool(average), after)
    fn_ef = entry(K, f"bagua_mxfp{c.bits}_reduce_requantize_ef", "test_middle_steps")
    guarded(lambda q: fn_ef(dtype, q["in"], S, cs, p, average, q["out"], S, target, q["residual"], None),
            head + [rw("residual", res, 4, residual_phase)], {"out": want, "residual": after},
            f"{what} error feedback, residual phase {residual_phase}")
    if c.SR:
        with np.errstate(all="ignore"):
            want = c.SR.reduce_requantize_sr(recv, p, cs, dtype, target, bool(average), key, out=fill(S))
        want = want[0] if isinstance(want, tuple) else want
        fn_sr = entry(K, f"bagua_mxfp{c.bits}_reduce_requantize_sr", "test_middle_steps")
        guarded(lambda q: fn_sr(dtype, q["in"], S, cs, p, average, q["out"], S, target, key, None), head, {"out": want},
                f"{what} stochastic")


@pytest.mark.parametrize("p", [2, 5, 16])  # one per BY (2, 4, 8)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", CODECS)
def test_middle_steps(bc, bits, dtype, p):
    """cs = 33: two blocks, the second ragged, a residual that is only 4-B aligned; 8193 + 64: two workgroups, 259
    blocks.  The target is the first and the last segment: the written one is the first or the last thing in `out`"""
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(300 + 100 * bits + 10 * dtype + p)
    key = SR4.key(0xB0A0 + bits, 5, 1, 1)
    for cs in (33, 8193 + 64):
        recv = received(c, rng, p, cs, dtype)
        for target in (0, p - 1):
            for average in (1, 0):
                # both tensor phases where the reduced chunk is stored, once per size
                phases = tensor_phases(dtype) if (target, average) == (p - 1, 1) else tensor_phases(dtype)[:1]
                check_middle(K, c, dtype, recv, p, cs, target, average, f"p={p} cs={cs} target={target} average={average}",
                             rng, phases, 4 if cs == 33 else 16, key)


# ------------------------------------------------------------ block ranges ----
def range_mask(c, cs, bb, be):
    """the bytes of one segment that the range [bb, be) may write: its scale bytes and payload, and both slacks
    where it ends the chunk"""
    nb, sb, seg = c.R.blocks(cs), c.R.scale_bytes(cs), c.R.segment_bytes(cs)
    m = np.zeros(seg, bool)
    m[bb:sb if be == nb else be] = True
    m[sb + c.block_bytes * bb:seg if be == nb else sb + c.block_bytes * be] = True
    return m


def masked(mask, data):
    """`data` where the mask allows a write, the buffer's fill elsewhere"""
    return np.where(mask, data, FILL).astype(np.uint8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", CODECS)
def test_range_entries(bc, bits, dtype):
    """cs = 128 * 32 + 37: the granule's range [0, 128) and the rest [128, 130).  Only the second may touch slack;
    the first writes nothing past block 127's payload.  Two chunks: the second starts misaligned"""
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(400 + 10 * bits + dtype)
    m, test = f"bagua_mxfp{bits}_", "test_range_entries"
    p, cs, es = 2, 128 * 32 + 37, ESIZE[dtype]
    nb, sb, seg, S = c.R.blocks(cs), c.R.scale_bytes(cs), c.R.segment_bytes(cs), c.R.compressed_bytes(cs, p)
    assert nb == 130
    x, recv, key = grads(rng, p * cs, dtype), received(c, rng, p, cs, dtype), SR4.key(0xB0A0 + bits, 7, 0, 0)
    with composed(c) as M:
        comp = c.R.compress(x, dtype, p)
        dec = c.R.decompress(comp, p, np.zeros(p * cs, c.R.STORAGE[dtype]), dtype)
        mid = M.reduce_requantize(recv, p, cs, dtype, 1, True, out=fill(S))[0]
        if c.SR:
            comp_sr = c.SR.compress_sr(x, dtype, p, key)
            mid_sr = c.SR.reduce_requantize_sr(recv, p, cs, dtype, 1, True, key, out=fill(S))
            mid_sr = mid_sr[0] if isinstance(mid_sr, tuple) else mid_sr
    for bb, be in ((0, 128), (128, nb)):
        what = f"blocks [{bb}, {be})"
        own = range_mask(c, cs, bb, be)
        every, last = np.tile(own, p), np.concatenate([np.zeros(seg, bool), own])
        elems = np.zeros(cs, bool)
        elems[32 * bb:min(32 * be, cs)] = True
        want_dec = masked(np.repeat(np.tile(elems, p), es), dec.view(np.uint8))

        def first_range_stops(got):  # on the bytes too: nothing past block 127's payload, in either segment
            if be != nb:
                for s in got.reshape(p, seg):
                    assert (s[be:sb] == FILL).all() and (s[sb + c.block_bytes * be:] == FILL).all(), what

        for ph in tensor_phases(dtype):
            fn = entry(K, m + "compress_range", test)
            got = guarded(lambda q: fn(dtype, q["x"], p * cs, cs, p, q["out"], S, bb, be, None),
                          [ro("x", x, es, ph), rw("out", fill(S), 16, 16)], {"out": masked(every, comp)},
                          f"{what} encode, phase {ph}")
            first_range_stops(got["out"])
            fn = entry(K, m + "decompress_range", test)
            guarded(lambda q: fn(dtype, q["in"], S, cs, p, q["out"], bb, be, None),
                    [ro("in", comp, c.decode_align, c.decode_align), rw("out", fill(p * cs * es), es, ph)], {"out": want_dec},
                    f"{what} decode, phase {ph}")
            if c.SR:
                fn = entry(K, m + "compress_sr_range", test)
                got = guarded(lambda q: fn(dtype, q["x"], p * cs, cs, p, q["out"], S, bb, be, key, None),
                              [ro("x", x, es, ph), rw("out", fill(S), 16, 16)], {"out": masked(every, comp_sr)},
                              f"{what} stochastic encode, phase {ph}")
                first_range_stops(got["out"])
        head = [ro("in", recv, 16, 16), rw("out", fill(S), 16, 16)]
        fn = entry(K, m + "reduce_requantize_range", test)
        got = guarded(lambda q: fn(dtype, q["in"], S, cs, p, 1, q["out"], S, 1, bb, be, None), head,
                      {"out": masked(last, mid)}, f"{what} middle step")
        first_range_stops(got["out"])
        if c.SR:
            fn = entry(K, m + "reduce_requantize_sr_range", test)
            got = guarded(lambda q: fn(dtype, q["in"], S, cs, p, 1, q["out"], S, 1, bb, be, key, None), head,
                          {"out": masked(last, mid_sr)}, f"{what} stochastic middle step")
            first_range_stops(got["out"])


# ------------------------------------------------------------------- ring ----
def reference_apply(c, segs, w, l, r, dtype):
    import test_gpu_mxfp4_ring
    import test_gpu_mxfp8_ring
    with composed(c):
        return (test_gpu_mxfp4_ring if c.bits == 4 else test_gpu_mxfp8_ring).reference_apply(segs, w, l, r, dtype)


def check_ring(K, c, dtype, n, rng, what):
    """the mix, the apply on three segments and on one in all three places, and the one-rank kernel, on the vector
    phase; one element off it every entry refuses the tensors and launches nothing"""
    es, test = ESIZE[dtype], "test_ring"
    mix, app, one = (entry(K, f"bagua_ring_{k}_mxfp{c.bits}", test) for k in ("mix", "apply", "one_rank"))
    t, w, l, r = arrs = [grads(rng, n, dtype) for _ in range(4)]
    with composed(c) as M:
        seg = c.R.compress(mixed_reference(t, w, l, r, dtype), dtype, 1)
        alone = [a[0] for a in M.decentralized([t], [w], [l], [r], dtype)]
        others = [c.R.compress(grads(rng, n, dtype), dtype, 1) for _ in range(2)]
    S = seg.size
    for ph in tensor_phases(dtype):
        rc = OK if ph % 16 == 0 else UNSUPPORTED
        tens = [(name, a, es, ph) for name, a in zip("twlr", arrs)]
        guarded(lambda q: mix(dtype, q["t"], q["l"], q["r"], q["w"], n, q["out"], S, None),
                [ro(*b) for b in tens] + [rw("out", fill(S), 16, 16)], {"out": seg} if rc == OK else {},
                f"{what} mix, phase {ph}", rc)
        ins = [ro(k, s, c.decode_align, c.decode_align) for k, s in zip(("mine", "from_left", "from_right"), [seg] + others)]
        want = dict(zip("twlr", reference_apply(c, [seg] + others, w, l, r, dtype))) if rc == OK else {}
        guarded(lambda q: app(dtype, q["mine"], q["from_left"], q["from_right"], S, n, q["t"], q["w"], q["l"], q["r"], None),
                ins + [rw(*b) for b in tens], want, f"{what} apply, phase {ph}", rc)
        want = dict(zip("twlr", reference_apply(c, [seg] * 3, w, l, r, dtype))) if rc == OK else {}
        guarded(lambda q: app(dtype, q["mine"], q["mine"], q["mine"], S, n, q["t"], q["w"], q["l"], q["r"], None),
                ins[:1] + [rw(*b) for b in tens], want, f"{what} apply on one segment, phase {ph}", rc)
        guarded(lambda q: one(dtype, q["t"], q["w"], q["l"], q["r"], n, None), [rw(*b) for b in tens],
                dict(zip("twlr", alone)) if rc == OK else {}, f"{what} one rank, phase {ph}", rc)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", CODECS)
def test_ring(bc, bits, dtype):
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(500 + 10 * bits + dtype)
    for n in (1, 33, RING_WAVE[dtype] + 37):
        check_ring(K, c, dtype, n, rng, f"n={n}")


# ------------------------------------------------------------ grid-stride ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", CODECS)
def test_second_grid_stride_iteration(bc, bits, dtype, monkeypatch):
    """every kernel family as one workgroup (its BAGUA_TUNE_*_BLOCKS knob at 1) on a size that gives each of its
    four waves a second iteration, the last one ragged: that iteration's tail is guarded too"""
    K, c, rng = bc._native.K, CODECS[bits], np.random.default_rng(600 + 10 * bits + dtype)
    for k in knobs(c):
        monkeypatch.setenv(k, "1")
    ph, key = tensor_phases(dtype)[:1], SR4.key(0xB0A0 + bits, 9, 2, 0)
    cs = 8 * ENCODE_WAVE[dtype] - 27
    x = grads(rng, cs, dtype)
    check_compress(K, c, dtype, x, 1, f"one workgroup, cs={cs}: encode", ph)
    if c.SR:
        check_compress(K, c, dtype, x, 1, f"one workgroup, cs={cs}: stochastic encode", ph, key=key)
    cs = 2 * DECODE_GROUP[dtype] - 27
    check_decompress(K, c, dtype, c.R.compress(grads(rng, cs, dtype), dtype, 1), 1, cs, f"one workgroup, cs={cs}: decode", ph)
    cs = 9 * EF_TILE + 69
    x, res = step_grads(rng, cs, dtype), state(rng, cs)
    after, S = res.copy(), c.R.compressed_bytes(cs, 1)
    want = c.EF.compress_ef(x, dtype, 1, types.SimpleNamespace(residual=after))
    fn = entry(K, f"bagua_mxfp{bits}_compress_ef", "test_compress_ef")
    guarded(lambda q: fn(dtype, q["x"], cs, cs, 1, q["out"], S, -1, q["residual"], None),
            [ro("x", x, ESIZE[dtype], 16), rw("out", fill(S), 16, 16), rw("residual", res, 4, 16)],
            {"out": want, "residual": after}, f"one workgroup, cs={cs}: encode with error feedback")
    cs = 2 * MIDDLE_GROUP - 27
    check_middle(K, c, dtype, received(c, rng, 2, cs, dtype), 2, cs, 1, 1, f"one workgroup, cs={cs}: middle step", rng, ph,
                 16, key)
    n = 8 * RING_WAVE[dtype] - 27
    check_ring(K, c, dtype, n, rng, f"one workgroup, n={n}")
