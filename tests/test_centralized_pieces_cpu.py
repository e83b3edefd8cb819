"""CPU tests of the pipelined centralized ops' piece tables (bagua_centralized_piece_plan,
host-only): which bytes of a segment each piece's alltoall and allgather move.

The unit range of a piece comes from the kernel library's own bagua_*_piece_range (covered
by test_abi.py and test_mxfp4_pieces_cpu.py).  The bytes expected for it are derived here,
byte by byte, from the segment formats of DESIGN.md §4 and MXFP4.md -- every byte of a
segment gets the piece that owns it -- and compared with the entry.  A wrong range would
otherwise show only as a parity failure on a GPU, a piece that arrives after the kernel that
reads it only as a race."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mxfp4_reference as R
from oracle import oracle_np as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 4
MINMAX, ONEBIT, MXFP4 = 1, 2, 3
F32, F16 = 0, 1
A2A, AG = 0, 1
TAPERED = 0x10000
COUNT_MASK = 0xFFFF
RANKS = [1, 2, 3, 8, 16]
CHUNKS = {MINMAX: [1, 511, 512, 1536, 12345, 40000],
          ONEBIT: [1, 1023, 1024, 1025, 5000, 12288],
          MXFP4: [1, 32, 4095, 4096, 4097, 12288, 40000]}
SCHEDULES = [1, 2, 3, 4, 7, 3 | TAPERED, 5 | TAPERED, 8 | TAPERED]
HEADER = 32     # MinMax and 1-bit: bytes of a segment before its payload
TILE, TILE_BYTES = 1024, 128  # 1-bit: elements and sign-bit bytes per tile


@pytest.fixture(scope="module")
def N():
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "bagua-core_amd")], check=True)
    from bagua_core import _native
    return _native


def segment_bytes(method, p, cs, dtype=F32):
    """S / p from the formats (None: S is no multiple of p, the ops refuse the tensor)"""
    if method == MINMAX:
        S = NP.minmax_compressed_size(p, cs, dtype)
        return S // p if S % p == 0 else None
    if method == ONEBIT:
        return HEADER + (cs + TILE - 1) // TILE * TILE_BYTES
    return R.segment_bytes(cs)


def unit_ranges(N, method, cs, schedule):
    f = {MINMAX: N.K.bagua_minmax_u8_piece_range, ONEBIT: N.K.bagua_onebit_piece_range,
         MXFP4: N.K.bagua_mxfp4_piece_range}[method]
    if method == ONEBIT:
        schedule &= COUNT_MASK  # uniform tile ranges: the 1-bit ops drop the taper flag
    b, e = ctypes.c_int(), ctypes.c_int()
    out = []
    for q in range(schedule & COUNT_MASK):
        assert f(cs, schedule, q, ctypes.byref(b), ctypes.byref(e)) == 0
        out.append((b.value, e.value))
    return out


def plan(N, method, p, cs, schedule, phase, dtype=F32):
    """[(unit_begin, unit_end, [(lo, hi), (lo, hi)])] of every piece, from the entry"""
    b, e = ctypes.c_int(), ctypes.c_int()
    r = (ctypes.c_size_t * 4)()
    out = []
    count = schedule & COUNT_MASK
    for q in range(count):
        n = N.C.bagua_centralized_piece_plan(method, dtype, p, cs, schedule, q, phase, ctypes.byref(b), ctypes.byref(e), r)
        assert n == count, (method, p, cs, hex(schedule), q, phase, n)
        out.append((b.value, e.value, [(r[0], r[1]), (r[2], r[3])]))
    return out


def owners(method, cs, co, units, phase):
    """the piece that moves each byte of a segment in `phase`, from the format"""
    own = np.full(co, -1, np.int64)
    filled = [q for q, (b, e) in enumerate(units) if e > b]
    last = filled[-1]  # the slack travels with the last non-empty piece
    if method == MINMAX:   # [0, 32) header, byte 32 + j element j, then slack
        own[:HEADER] = 0   # the header travels with piece 0 in both phases
        for q, (b, e) in enumerate(units):
            own[HEADER + b:HEADER + e] = q
        own[HEADER + cs:] = last
    elif method == ONEBIT:  # [0, 32) header, tile t at [32 + 128 t, 32 + 128 (t + 1)), no slack
        own[:HEADER] = len(units) - 1 if phase == A2A else 0  # last in the alltoall, first in the allgather
        for q, (b, e) in enumerate(units):
            own[HEADER + TILE_BYTES * b:HEADER + TILE_BYTES * e] = q
    else:  # MXFP4.md: nb scale bytes padded to sb, then 16 bytes per block, padded
        nb, sb = R.blocks(cs), R.scale_bytes(cs)
        for q, (b, e) in enumerate(units):
            own[b:e] = q
            own[sb + 16 * b:sb + 16 * e] = q
        own[nb:sb] = last
        own[sb + 16 * nb:] = last
    assert (own >= 0).all()
    return own


def reads(method, cs, co, b, e):
    """the bytes of a segment that the consumer of units [b, e) reads (the fused reduce or
    middle step in the alltoall phase, the decode in the allgather phase)"""
    m = np.zeros(co, bool)
    if e <= b:
        return m  # nothing is launched for an empty piece
    if method == MINMAX:
        m[:HEADER] = True
        m[HEADER + b:HEADER + e] = True
    elif method == ONEBIT:
        m[:HEADER] = True
        m[HEADER + TILE_BYTES * b:HEADER + TILE_BYTES * e] = True
    else:
        sb = R.scale_bytes(cs)
        m[b:e] = True
        m[sb + 16 * b:sb + 16 * e] = True
    return m


@pytest.mark.parametrize("p", RANKS)
@pytest.mark.parametrize("method", [MINMAX, ONEBIT, MXFP4])
def test_piece_tables(N, method, p):
    for cs in CHUNKS[method]:
        for dtype in ((F32, F16) if method == MINMAX else (F32,)):
            co = segment_bytes(method, p, cs, dtype)
            for schedule in SCHEDULES:
                what = f"method={method} p={p} cs={cs} dtype={dtype} schedule={schedule:#x}"
                if co is None:  # S % p != 0: the ops return INVALID_ARG for this tensor, the entry too
                    assert N.C.bagua_centralized_piece_plan(method, dtype, p, cs, schedule, 0, A2A, None, None,
                                                            None) == -INVALID_ARG, what
                    continue
                units = unit_ranges(N, method, cs, schedule)
                for phase in (A2A, AG):
                    table = plan(N, method, p, cs, schedule, phase, dtype)
                    assert [(b, e) for b, e, _ in table] == units, what
                    want = owners(method, cs, co, units, phase)
                    seen = np.zeros(co, bool)     # union of pieces 0 .. q
                    for q, (b, e, ranges) in enumerate(table):
                        mine = np.zeros(co, bool)
                        for lo, hi in ranges:
                            if hi <= lo:
                                continue
                            assert hi <= co, f"{what} phase={phase} piece={q}: {ranges}"
                            assert not mine[lo:hi].any() and not seen[lo:hi].any(), f"{what} phase={phase}: overlap at {q}"
                            mine[lo:hi] = True
                        assert (mine == (want == q)).all(), f"{what} phase={phase} piece={q}: {ranges}"
                        seen |= mine
                        if e <= b:
                            # an empty piece moves nothing -- unless the header travels with it: the
                            # 1-bit alltoall's last piece, and MinMax's piece 0 when a tapered
                            # schedule's first edge rounds down to 0 (its quantise writes the header)
                            carrier = (method == ONEBIT and phase == A2A and q == len(table) - 1) or \
                                      (method == MINMAX and q == 0)
                            assert mine.sum() == (HEADER if carrier else 0), f"{what} phase={phase} piece={q}"
                            assert not carrier or mine[:HEADER].all()
                        # what the consumer of piece q reads has arrived with pieces 0 .. q (the
                        # 1-bit middle step runs once, after the last piece: the union below)
                        if not (method == ONEBIT and phase == A2A):
                            assert not (reads(method, cs, co, b, e) & ~seen).any(), f"{what} phase={phase} piece={q}"
                    assert seen.all(), f"{what} phase={phase}: bytes no piece moves"


def test_refusals(N):
    f = N.C.bagua_centralized_piece_plan
    b, e = ctypes.c_int(), ctypes.c_int()
    r = (ctypes.c_size_t * 4)()
    out = (ctypes.byref(b), ctypes.byref(e), r)
    for method, cs in ((MINMAX, 1536), (ONEBIT, 5000), (MXFP4, 12288)):
        assert f(method, F32, 2, cs, 4, 3, A2A, *out) == 4
        assert f(method, F32, 2, cs, 4, 0, AG, None, None, None) == 4       # outputs are optional
        assert f(method, F32, 2, cs, 4 | (1 << 21), 0, A2A, *out) == -INVALID_ARG   # unknown schedule bit
        assert f(method, F32, 2, cs, 4 | 0x40000, 0, A2A, *out) == -INVALID_ARG     # a kernel-only flag (FOLDED)
        assert f(method, F32, 2, cs, 0, 0, A2A, *out) == -INVALID_ARG               # no count
        assert f(method, F32, 2, cs, TAPERED, 0, A2A, *out) == -INVALID_ARG
        assert f(method, F32, 2, cs, 4, 4, A2A, *out) == -INVALID_ARG               # piece outside the count
        assert f(method, F32, 2, cs, 4, -1, A2A, *out) == -INVALID_ARG
        assert f(method, F32, 2, cs, 4, 0, 2, *out) == -INVALID_ARG                 # no such phase
        assert f(method, F32, 0, cs, 4, 0, A2A, *out) == -INVALID_ARG               # no ranks
        assert f(method, F32, 2, 1 << 31, 4, 0, A2A, *out) == -INVALID_ARG          # a chunk past INT_MAX
    for method in (0, 4, -1):                                                       # no pieced op
        assert f(method, F32, 2, 4096, 4, 0, A2A, *out) == -UNSUPPORTED
