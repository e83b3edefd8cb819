"""CPU tests of the pieced MXFP4 codec (MXFP4.md, "Pipelined op"): the host-only piece
schedule bagua_mxfp4_piece_range, the refusals of the three range entries (which come
before anything touches a device: null stream, fabricated pointers, no GPU) and, on the
numpy reference's layout, the byte ranges the pieces of a schedule cover in a segment."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mxfp4_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, 1
GRANULE = 128  # blocks between two piece boundaries (4096 elements)
CHUNKS = [0, 1, 31, 32, 4095, 4096, 4097, 3 * 4096 + 37 * 32 + 5, 2 ** 20 + 7]
COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 255]


@pytest.fixture(scope="module")
def N():
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "bagua-core_amd")], check=True)
    from bagua_core import _native
    return _native


def ranges(N, cs, schedule):
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & N.PIECES_COUNT_MASK):
        assert N.K.bagua_mxfp4_piece_range(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == OK
        out.append((b.value, e.value))
    return out


def piece_bytes(cs, bb, be):
    """the two byte ranges of a segment that blocks [bb, be) cover; the range that ends at nb
    runs to the end of both regions (the slack)"""
    nb, sb, seg = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    if bb >= be:
        return []
    last = be == nb
    return [(bb, sb if last else be), (sb + 16 * bb, seg if last else sb + 16 * be)]


@pytest.mark.parametrize("tapered", [False, True])
@pytest.mark.parametrize("cs", CHUNKS)
def test_piece_ranges_partition_the_blocks(N, cs, tapered):
    nb = R.blocks(cs)
    for count in COUNTS:
        rs = ranges(N, cs, count | (N.PIECES_TAPERED if tapered else 0))
        what = f"cs={cs} count={count} tapered={tapered}: {rs}"
        pos = 0
        for b, e in rs:
            assert b == pos and e >= b, what  # in order, no gap, no overlap
            assert e % GRANULE == 0 or e == nb, what
            pos = e
        assert pos == nb, what
        sizes = [e - b for b, e in rs]
        filled = [s for s in sizes if s]
        assert sizes[:len(filled)] == filled, f"{what}: empty ranges only at the tail"
        if tapered and count < 3:
            assert rs == ranges(N, cs, count), what
        if tapered and count >= 3 and nb >= GRANULE * 2 * (count - 1):
            assert len(filled) == count, what
            assert filled[0] <= min(filled[1:-1]) and filled[-1] <= min(filled[1:-1]), what


def test_tapered_edges_follow_the_weights(N):
    """edge weights 0, 1, 3, ..., 2(k - 1): with whole granules per weight unit the first and
    the last piece are exactly half the others"""
    for count in (3, 4, 8):
        unit = 5 * GRANULE
        cs = 32 * unit * 2 * (count - 1)
        sizes = [e - b for b, e in ranges(N, cs, count | N.PIECES_TAPERED)]
        assert sizes == [unit] + [2 * unit] * (count - 2) + [unit], (count, sizes)


def test_piece_range_refusals(N):
    f = N.K.bagua_mxfp4_piece_range
    b, e = ctypes.c_int(), ctypes.c_int()
    rb, re_ = ctypes.byref(b), ctypes.byref(e)
    assert f(4096, 2, 0, rb, re_) == OK
    assert f(4096, 0, 0, rb, re_) == INVALID_ARG                       # no count
    assert f(4096, N.PIECES_TAPERED, 0, rb, re_) == INVALID_ARG        # a flag without a count
    assert f(4096, 2 | (1 << 21), 0, rb, re_) == INVALID_ARG           # unknown schedule bit
    assert f(4096, 2, 2, rb, re_) == INVALID_ARG                       # piece out of range
    assert f(4096, 2, -1, rb, re_) == INVALID_ARG
    assert f(-1, 2, 0, rb, re_) == INVALID_ARG
    assert f(4096, 2, 0, None, re_) == INVALID_ARG
    assert f(4096, 2, 0, rb, None) == INVALID_ARG


@pytest.mark.parametrize("entry", ["compress", "decompress", "reduce_requantize"])
def test_range_entries_refuse_bad_ranges_before_the_device(N, entry):
    """a misaligned block_begin, block_end past nb, below block_begin, or neither nb nor a
    multiple of 128: BAGUA_ERR_INVALID_ARG with nothing launched -- the pointers are
    fabricated (16-B aligned, never dereferenced on the host) and this test has no device.
    Empty ranges return BAGUA_OK the same way."""
    K = N.K
    cs, p = 3 * 4096 + 37 * 32 + 5, 2
    nb, S = R.blocks(cs), R.compressed_bytes(cs, p)
    assert nb == 3 * GRANULE + 38
    a, o = 0x10000, 0x20000

    def call(bb, be, dtype=0):
        if entry == "compress":
            return K.bagua_mxfp4_compress_range(dtype, a, cs * p, cs, p, o, S, bb, be, None)
        if entry == "decompress":
            return K.bagua_mxfp4_decompress_range(dtype, o, S, cs, p, a, bb, be, None)
        return K.bagua_mxfp4_reduce_requantize_range(dtype, a, S, cs, p, 1, o, S, 1, bb, be, None)

    for dtype in (0, 1, 2):
        assert call(64, 128, dtype) == INVALID_ARG         # block_begin not on a granule
        assert call(1, nb, dtype) == INVALID_ARG
        assert call(-128, 128, dtype) == INVALID_ARG
        assert call(-1, -1, dtype) == INVALID_ARG
        assert call(0, nb + 1, dtype) == INVALID_ARG       # block_end past nb
        assert call(4 * GRANULE, 4 * GRANULE, dtype) == INVALID_ARG  # block_begin past nb
        assert call(256, 128, dtype) == INVALID_ARG        # block_end below block_begin
        assert call(0, nb - 1, dtype) == INVALID_ARG       # neither nb nor a multiple of 128
        assert call(128, 200, dtype) == INVALID_ARG
        for bb in (0, 128, 256, 384):                      # empty ranges: nothing to launch
            assert call(bb, bb, dtype) == OK
        assert call(nb, nb, dtype) == INVALID_ARG          # empty, but nb is no multiple of 128 here
    # the whole-chunk entries' refusals hold for the range entries too
    if entry == "compress":
        assert K.bagua_mxfp4_compress_range(0, a, cs * p, cs, p, o, S - 1, 0, 128, None) == INVALID_ARG
        assert K.bagua_mxfp4_compress_range(0, a, cs * p, cs, p, o + 4, S, 0, 128, None) == INVALID_ARG
        assert K.bagua_mxfp4_compress_range(0, None, cs * p, cs, p, o, S, 0, 128, None) == INVALID_ARG
        assert K.bagua_mxfp4_compress_range(3, a, cs * p, cs, p, o, S, 0, 128, None) == 4
    elif entry == "decompress":
        assert K.bagua_mxfp4_decompress_range(0, o, S - 1, cs, p, a, 0, 128, None) == INVALID_ARG
        assert K.bagua_mxfp4_decompress_range(0, o + 2, S, cs, p, a, 0, 128, None) == INVALID_ARG
        assert K.bagua_mxfp4_decompress_range(0, o, S, cs, p, None, 0, 128, None) == INVALID_ARG
    else:
        assert K.bagua_mxfp4_reduce_requantize_range(0, a, S, cs, p, 1, o, S, p, 0, 128, None) == INVALID_ARG
        assert K.bagua_mxfp4_reduce_requantize_range(0, a, S, cs, p, 1, o, S - 1, 0, 0, 128, None) == INVALID_ARG
        S17 = R.compressed_bytes(cs, 17)
        assert K.bagua_mxfp4_reduce_requantize_range(0, a, S17, cs, 17, 1, o, S17, 0, 0, 128, None) == 4  # UNSUPPORTED


@pytest.mark.parametrize("cs", [c for c in CHUNKS if c])
def test_pieces_cover_the_segment_once(N, cs):
    """the two byte ranges of all pieces of a schedule are disjoint and their union is the
    whole segment of the reference's layout; the slack (bytes past the nb scale bytes and
    past the 16 nb payload bytes) belongs to the last non-empty piece only"""
    nb, sb, seg = R.blocks(cs), R.scale_bytes(cs), R.segment_bytes(cs)
    assert seg == R.compressed_bytes(cs, 1)
    slack = np.zeros(seg, bool)
    slack[nb:sb] = True
    slack[sb + 16 * nb:] = True
    for count in COUNTS:
        for schedule in (count, count | N.PIECES_TAPERED):
            rs = ranges(N, cs, schedule)
            owner = np.full(seg, -1, np.int64)
            for q, (bb, be) in enumerate(rs):
                for lo, hi in piece_bytes(cs, bb, be):
                    assert (owner[lo:hi] == -1).all(), (cs, schedule, q)
                    owner[lo:hi] = q
            assert (owner >= 0).all(), (cs, schedule)
            last = max(q for q, (bb, be) in enumerate(rs) if be > bb)
            assert (owner[slack] == last).all(), (cs, schedule)
            for q, (bb, be) in enumerate(rs):  # and nothing but its own blocks otherwise
                mine = np.zeros(seg, bool)
                mine[bb:be] = True
                mine[sb + 16 * bb:sb + 16 * be] = True
                assert ((owner == q) & ~slack == mine & ~slack).all(), (cs, schedule, q)
