"""Boundary inputs for the MXFP8 codec (MXFP8.md).  CPU only, shared by
tests/test_mxfp8_boundary_cpu.py and tests/test_gpu_mxfp8_boundaries.py.

Random data never lands on a tie of the E4M3 grid or one ulp beside it, and it reaches few
scale bytes.  `table(dtype)` is a tensor of whole blocks of T values in which every element
is there for a reason, with the code each one must get:

  pinned blocks   For every scale byte a finite T can produce (0..247 for f32 and bf16,
                  95..135 for f16) blocks hold one pin, their amax: 448 * 2^e or 256 * 2^e with
                  e = byte - 127, the first that is a finite T value, and the largest finite T
                  for the top byte.  Beside it stand, for each of the 126 ties between
                  neighbouring E4M3 magnitudes times 2^e and for both signs, three elements:
                  the tie itself, the next T value below it and the next T value above it (in
                  magnitude).  All 126 ties stand under every byte (about 200 K elements for
                  f32), so nothing is rotated.  A (byte, tie, side) triple is left out only if
                  the tie is no finite T value, the element would exceed the block's pin, or
                  T is so coarse there that the neighbour is no longer between the tie's two
                  grid values (`Table.left_out`).  A byte's triples are sorted by magnitude and
                  cut into blocks of 31: in the blocks whose elements are all at most
                  224 * 2^e the pin alone decides the scale byte (`pin_decides`); in the others
                  the pin is the amax but not the only element that holds the byte.  A block
                  is filled up with +0.
  edge blocks     The pin is 1.75 * 2^j, the largest T value with m <= 0.875 in
                  amax = m * 2^k, or the next T value above it: the edge of the scale rule (the
                  `+ 0x1fffff` carry of mx8_scale_byte), at every fourth exponent j across T's
                  range; and the smallest normal and the largest denormal T as amax.
                  Everything else is at most a quarter of the pin.
  planted blocks  32 blocks for each of three scale bytes: the pin 448 * 2^e at position
                  k = 0..31, every other element at most 112 * 2^e, so a pass that misses the
                  pin moves the scale byte by 2.

The element order of a block is rotated by the block's index: the pin visits all 32
positions, and every class reaches every position of a lane's 16-byte vector and every byte
of a payload word.  The block count is a multiple of 3 (three chunks of whole blocks) and no
multiple of a wave tile.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import oracle_np as NP

F32, F16, BF16 = 0, 1, 2
BLOCK = 32
STORAGE = {F32: np.float32, F16: np.float16, BF16: np.uint16}
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
MANT = {F32: 23, F16: 10, BF16: 7}          # explicit significand bits of T
EMIN = {F32: -126, F16: -14, BF16: -126}    # exponent of the smallest normal T
MAX_FINITE = {F32: float(np.finfo(np.float32).max), F16: 65504.0,
              BF16: float(np.uint32(0x7F7F0000).view(np.float32))}
BYTES = {F32: range(0, 248), F16: range(95, 136), BF16: range(0, 248)}


def code_value(c: int) -> float:
    e, m = c >> 3, c & 7
    return m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)


GRID = np.array([code_value(c) for c in range(127)])   # the magnitudes of codes 0 .. 0x7E
TIES = (GRID[:-1] + GRID[1:]) / 2                      # tie i lies between the codes i and i + 1
EVEN_CODE = np.array([i if i % 2 == 0 else i + 1 for i in range(126)])
SIDES = (-1, 0, 1)  # the next T value below, the tie itself, the next T value above

PIN, TIE, FILL = 0, 1, 2                       # Table.kind
PINNED, EDGE, PLANTED = 0, 1, 2                # Table.cls
PLANTED_BYTES = {F32: (2, 127, 246), F16: (100, 120, 134), BF16: (2, 127, 246)}


# --------------------------------------------------------------- T values ----
def is_t(v, dtype: int) -> np.ndarray:
    """v (float64, any shape) is a finite value of T"""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        back = NP.to_f32(NP.from_f32(v.astype(np.float32).ravel(), dtype), dtype).astype(np.float64).reshape(v.shape)
    return (back == v) & (np.abs(v) <= MAX_FINITE[dtype])


def neighbours(v: np.ndarray, dtype: int):
    """(next T value below, next T value above) of positive T values v, as float64; above the
    largest finite T lies inf"""
    b = NP.from_f32(np.asarray(v, np.float64).astype(np.float32).ravel(), dtype).view(BITS[dtype])
    lo = NP.to_f32((b - 1).astype(BITS[dtype]).view(STORAGE[dtype]), dtype).astype(np.float64)
    hi = NP.to_f32((b + 1).astype(BITS[dtype]).view(STORAGE[dtype]), dtype).astype(np.float64)
    return lo.reshape(np.shape(v)), hi.reshape(np.shape(v))


def to_t(v64: np.ndarray, dtype: int) -> np.ndarray:
    """float64 values that are T values -> T storage; raises if one of them is not"""
    v32 = np.asarray(v64, np.float64).astype(np.float32)
    t = NP.from_f32(v32.ravel(), dtype)
    if not np.array_equal(NP.to_f32(t, dtype).astype(np.float64), np.asarray(v64, np.float64).ravel()):
        raise ValueError("a table value is not a value of T")
    if (np.signbit(v64) & (np.asarray(v64) == 0)).any():
        raise ValueError("the table holds no -0")
    return t


def pin_of(byte: int, dtype: int) -> float:
    e = byte - 127
    for c in (448.0, 256.0):
        if bool(is_t(math.ldexp(c, e), dtype)):
            return math.ldexp(c, e)
    assert byte == BYTES[dtype][-1]
    return MAX_FINITE[dtype]


def triples_of(byte: int, dtype: int):
    """(tie index, side, magnitude, code) arrays of the triples present under this byte's pin"""
    e, pin = byte - 127, pin_of(byte, dtype)
    t = np.ldexp(TIES, e)
    ok = is_t(t, dtype) & (t <= pin)
    idx = np.nonzero(ok)[0]
    t = t[idx]
    lo, hi = neighbours(t, dtype)
    glo, ghi = np.ldexp(GRID[idx], e), np.ldexp(GRID[idx + 1], e)
    out = [(idx, np.zeros_like(idx), t, EVEN_CODE[idx])]
    keep = (lo > glo) & (lo > 0)
    out.append((idx[keep], np.full(keep.sum(), -1), lo[keep], idx[keep]))
    keep = (hi < ghi) & (hi <= pin)
    out.append((idx[keep], np.full(keep.sum(), 1), hi[keep], idx[keep] + 1))
    i, s, m, c = (np.concatenate(x) for x in zip(*out))
    order = np.argsort(m, kind="stable")
    return i[order], s[order], m[order], c[order]


# ------------------------------------------------------------------ table ----
@dataclass(frozen=True)
class Table:
    dtype: int
    x: np.ndarray            # (nb * 32,) T storage
    byte: np.ndarray         # (nb,) the scale byte each block was built for
    cls: np.ndarray          # (nb,) PINNED, EDGE or PLANTED
    pin_pos: np.ndarray      # (nb,) position of the pin
    pin_decides: np.ndarray  # (nb,) without the pin the block's scale byte is lower
    kind: np.ndarray         # (nb, 32) PIN, TIE or FILL
    tie: np.ndarray          # (nb, 32) tie index of a TIE element, else -1
    side: np.ndarray         # (nb, 32) its side (-1, 0, 1)
    code: np.ndarray         # (nb, 32) the element byte a TIE element must get (sign included), else -1
    left_out: int            # how many (byte, tie, side, sign) triples T cannot represent under their pin

    @property
    def nb(self) -> int:
        return self.byte.size

    def values(self) -> np.ndarray:
        """(nb, 32) float64"""
        return NP.to_f32(self.x, self.dtype).astype(np.float64).reshape(-1, BLOCK)

    def without_pins(self) -> np.ndarray:
        """values() with every block's pin replaced by +0"""
        v = self.values().copy()
        v[np.arange(self.nb), self.pin_pos] = 0.0
        return v


def edge_pins(dtype: int) -> list:
    """[(pin, scale byte)] of the edge class"""
    out = []
    lo = EMIN[dtype] - MANT[dtype] + 2           # 1.75 * 2^j needs three significand bits
    hi = {F32: 127, F16: 15, BF16: 127}[dtype]
    for j in list(range(lo, hi, 4)) + [hi - 1]:
        a = math.ldexp(1.75, j)                  # m = 0.875, k = j + 1: e = j - 8
        out.append((a, max(j + 119, 0)))
        above = float(neighbours(np.array([a]), dtype)[1][0])
        if above <= MAX_FINITE[dtype]:
            out.append((above, max(j + 120, 0)))  # m just above 0.875: e = j - 7
    normal = math.ldexp(1.0, EMIN[dtype])        # 0.5 * 2^(EMIN + 1): e = EMIN - 8
    out.append((normal, max(EMIN[dtype] + 119, 0)))
    out.append((float(neighbours(np.array([normal]), dtype)[0][0]), max(EMIN[dtype] + 119, 0)))  # m just below 1, k = EMIN
    return out


def _quarter(pin: float, dtype: int, b: int) -> np.ndarray:
    """31 T values of magnitude at most pin / 4 (no -0)"""
    f = np.array([(0.25, -0.125, 0.0625, -0.25, 0.0, 0.125)[(k + b) % 6] for k in range(BLOCK - 1)])
    v = NP.to_f32(NP.from_f32((pin * f).astype(np.float32), dtype), dtype).astype(np.float64)
    v[(np.abs(v) > pin / 4) | (v == 0)] = 0.0
    return v


@functools.lru_cache(maxsize=None)
def table(dtype: int) -> Table:
    vals, kinds, ties, sides, codes, byte_of, cls_of, decides = [], [], [], [], [], [], [], []
    left_out = 0

    def add(v, kind, tie, side, code, byte, cls, roll, pin_decides):
        r = roll % BLOCK   # element 0, the pin, lands on position r
        for dst, src in ((vals, v), (kinds, kind), (ties, tie), (sides, side), (codes, code)):
            dst.append(np.roll(np.asarray(src), r))
        byte_of.append(byte)
        cls_of.append(cls)
        decides.append(pin_decides)

    for byte in BYTES[dtype]:
        e, pin = byte - 127, pin_of(byte, dtype)
        i, s, m, c = triples_of(byte, dtype)
        left_out += 2 * (3 * TIES.size - i.size)
        # both signs, interleaved, ascending in magnitude
        i, s, m = np.repeat(i, 2), np.repeat(s, 2), np.repeat(m, 2)
        c = np.repeat(c, 2)
        neg = np.arange(m.size) % 2 == 1
        m = np.where(neg, -m, m)
        c = np.where(neg, c | 0x80, c)
        for k in range(0, max(m.size, 1), BLOCK - 1):   # a byte whose ties T cannot hold still gets its pin
            n = min(BLOCK - 1, m.size - k)
            b = len(vals)
            flip = b % 2 == 1   # every other block has a negative pin
            v = np.zeros(BLOCK)
            kind = np.full(BLOCK, FILL)
            tie, side, code = np.full(BLOCK, -1), np.zeros(BLOCK, int), np.full(BLOCK, -1)
            v[0], kind[0] = (-pin if flip else pin), PIN
            v[1:1 + n], kind[1:1 + n] = m[k:k + n], TIE
            tie[1:1 + n], side[1:1 + n], code[1:1 + n] = i[k:k + n], s[k:k + n], c[k:k + n]
            add(v, kind, tie, side, code, byte, PINNED, b, bool(byte > 0 and (n == 0 or np.abs(m[k:k + n]).max() <= math.ldexp(224.0, e))))
    for pin, byte in edge_pins(dtype):
        b = len(vals)
        v = np.concatenate([[pin], _quarter(pin, dtype, b)])
        kind = np.array([PIN] + [FILL] * (BLOCK - 1))
        add(v, kind, np.full(BLOCK, -1), np.zeros(BLOCK, int), np.full(BLOCK, -1), byte, EDGE, b, byte > 0)
    others = np.array((112.0, -96.0, 64.0, -48.0, 1.0, -0.25, 0.0, -112.0, 80.0, -2.0 ** -6, 2.0 ** -9, -32.0, 16.0))

    def planted(byte, k, roll):
        e = byte - 127
        v = np.concatenate([[math.ldexp(-448.0 if k % 2 else 448.0, e)],
                            np.ldexp(others[(np.arange(BLOCK - 1) + k) % others.size], e)])
        v[~is_t(v, dtype)] = 0.0
        v[v == 0] = 0.0
        kind = np.array([PIN] + [FILL] * (BLOCK - 1))
        add(v, kind, np.full(BLOCK, -1), np.zeros(BLOCK, int), np.full(BLOCK, -1), byte, PLANTED, roll, True)

    for byte in PLANTED_BYTES[dtype]:
        for k in range(BLOCK):
            planted(byte, k, k)
    k = 0
    while len(vals) % 3 or len(vals) % 128 == 0:  # three chunks of whole blocks, a ragged last wave tile
        planted(PLANTED_BYTES[dtype][1], k, 7 * k + 3)
        k += 1
    v = np.array(vals, np.float64)
    kind = np.array(kinds, np.int8)
    assert ((kind == PIN).sum(axis=1) == 1).all()
    x = to_t(v, dtype)
    x.setflags(write=False)
    return Table(dtype, x, np.array(byte_of, np.int64), np.array(cls_of, np.int8),
                 np.argmax(kind == PIN, axis=1).astype(np.int64), np.array(decides, bool), kind,
                 np.array(ties, np.int16), np.array(sides, np.int8), np.array(codes, np.int16), left_out)
