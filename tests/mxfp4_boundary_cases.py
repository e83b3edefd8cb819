"""Boundary inputs for the MXFP4 codec (MXFP4.md).  CPU only, shared by
tests/test_mxfp4_boundary_cpu.py and tests/test_gpu_mxfp4_boundaries.py.

Random data never lands on a tie of the E2M1 grid or one ulp beside it, and it reaches few
scale bytes.  `table(dtype)` is a tensor of whole blocks of T values in which every element
is there for a reason, with a description of each:

  pinned blocks   For every scale byte a finite T can produce (0..253 for f32 and bf16,
                  101..141 for f16) a block holds one pin, its amax: 6 * 2^e or 4 * 2^e with
                  e = byte - 127, the first that is a finite T value, and the largest finite T
                  for the top byte.  Around it, for each of 0.25, 0.75, 1.25, 1.75, 2.5, 3.5
                  and 5.0 times 2^e and for both signs, three elements: the value itself, the
                  next T value below it and the next T value above it (in magnitude; the
                  neighbour below the smallest T is +0 for both signs, so the table holds
                  no -0).  A (byte, boundary, side) triple is left out only if the boundary
                  is not a finite T value or the element would exceed the block's pin
                  (`Table.left_out`).  42 elements do not fit beside a pin, so a byte's triples
                  are split over a LOW block (0.25 .. 2.5: everything else is at most
                  3 * 2^e, so the pin alone decides the scale byte) and a HIGH block (3.5 and
                  5.0: any element above 3 * 2^e gives the pin's scale byte as well, so there
                  the pin is the amax but not the only element that holds the byte).
                  The rest of a block is filled from exact grid points, +0, the smallest
                  non-zero T and pin * 2^-40.  Every byte has two LOW and two HIGH blocks
                  (the second of each with the element order reversed and a negative pin), and
                  the byte list is walked until the class has about a thousand blocks.
  edge blocks     The pin is 1.5 * 2^j, the largest T value with m <= 0.75 in
                  amax = m * 2^k, or the next T value above it: the edge of the scale rule
                  (the `+ 0x3fffff` carry of mx_scale_byte), at about a dozen exponents j
                  across T's range; and the smallest normal and the largest denormal T as amax.
                  Everything else is at most a quarter of the pin.
  planted blocks  32 blocks for each of three scale bytes: the pin 6 * 2^e at position
                  k = 0..31, every other element at most 1.5 * 2^e, so a pass that misses the
                  pin moves the scale byte by 2.

The element order of a block is rotated by the block's index: the pin visits all 32
positions, and every class reaches every position of a lane's 16-byte vector and every nibble
of a payload word.  The block count is a multiple of 3 (three chunks of whole blocks) and no
multiple of a wave tile.

`middle_exact(dtype)` and `middle_neighbours()` build received segments for the centralized
op's middle step whose decoded values sum, in the summation tree of the reduce, exactly to
the boundaries and to their one-ulp neighbours.
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
SMALLEST = {d: math.ldexp(1.0, EMIN[d] - MANT[d]) for d in (F32, F16, BF16)}
BYTES = {F32: range(0, 254), F16: range(101, 142), BF16: range(0, 254)}

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BOUNDARIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
# boundary i lies between the codes i and i + 1; a tie goes to the even one of the two
LOWER_CODE = (0, 1, 2, 3, 4, 5, 6)
UPPER_CODE = (1, 2, 3, 4, 5, 6, 7)
EVEN_CODE = (0, 2, 2, 4, 4, 6, 6)
SIDES = (-1, 0, 1)  # the next T value below, the boundary itself, the next T value above

PIN, BOUNDARY, FILL = 0, 1, 2                  # Table.kind
LOW, HIGH, EDGE, PLANTED = 0, 1, 2, 3          # Table.cls
LOW_BOUNDARIES, HIGH_BOUNDARIES = (0, 1, 2, 3, 4), (5, 6)
PINNED_BLOCKS = 960                            # whole walks of the byte list until the pinned class has this many blocks
PLANTED_BYTES = {F32: (2, 127, 252), F16: (105, 120, 140), BF16: (2, 127, 252)}
# 1.5 * 2^j: denormal, around the smallest normal, mid-range, up to the last j whose next T is finite
EDGE_EXPONENTS = {F32: (-128, -127, -126, -125, -124, -100, -64, -1, 0, 1, 64, 100, 126, 127),
                  F16: (-23, -22, -16, -15, -14, -13, -8, -1, 0, 1, 8, 14, 15),
                  BF16: (-128, -127, -126, -125, -124, -100, -64, -1, 0, 1, 64, 100, 126, 127)}


# --------------------------------------------------------------- T values ----
def is_t(v: float, dtype: int) -> bool:
    """v is a finite value of T"""
    a = abs(v)
    if a == 0:
        return True
    if not a <= MAX_FINITE[dtype]:
        return False
    _, k = math.frexp(a)
    q = math.ldexp(a, MANT[dtype] - max(k - 1, EMIN[dtype]))
    return q == int(q)


def _bits(v: float, dtype: int) -> int:
    return int(NP.from_f32(np.array([v], np.float32), dtype).view(BITS[dtype])[0])


def _value(bits: int, dtype: int) -> float:
    return float(NP.to_f32(np.array([bits], BITS[dtype]).view(STORAGE[dtype]), dtype)[0])


def neighbours(v: float, dtype: int):
    """(next T value below, next T value above) of a T value v > 0; below the smallest T lies +0,
    above the largest finite T inf"""
    b = _bits(v, dtype)
    return _value(b - 1, dtype), _value(b + 1, dtype)


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
    for c in (6.0, 4.0):
        if is_t(math.ldexp(c, e), dtype):
            return math.ldexp(c, e)
    if byte == BYTES[dtype][-1]:
        return MAX_FINITE[dtype]
    return math.ldexp(3.5, e)


def triples_of(byte: int, dtype: int) -> dict:
    """(boundary index, side) -> magnitude, for the triples present under this byte's pin"""
    e, pin, out = byte - 127, pin_of(byte, dtype), {}
    for i, c in enumerate(BOUNDARIES):
        v = math.ldexp(c, e)
        if not is_t(v, dtype) or v > pin:
            continue
        below, above = neighbours(v, dtype)
        for side, m in zip(SIDES, (below, v, above)):
            if m <= pin:
                out[(i, side)] = m
    return out


# ------------------------------------------------------------------ table ----
@dataclass(frozen=True)
class Table:
    dtype: int
    x: np.ndarray        # (nb * 32,) T storage
    byte: np.ndarray     # (nb,) the scale byte each block was built for
    cls: np.ndarray      # (nb,) LOW, HIGH, EDGE or PLANTED
    pin_pos: np.ndarray  # (nb,) position of the pin
    kind: np.ndarray     # (nb, 32) PIN, BOUNDARY or FILL
    bnd: np.ndarray      # (nb, 32) boundary index of a BOUNDARY element, else -1
    side: np.ndarray     # (nb, 32) its side (-1, 0, 1)
    left_out: frozenset  # the (byte, boundary index, side) triples no block holds

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


def _fill_pool(byte: int, dtype: int, pin: float, cap: float) -> list:
    e = byte - 127
    pool = [math.ldexp(g, e) for g in GRID[1:7]] + [0.0, SMALLEST[dtype], math.ldexp(pin, -40)]
    return [v for v in pool if is_t(v, dtype) and v <= cap and v < pin]


def _pinned_block(b: int, byte: int, q: int, dtype: int):
    """element list (value, kind, boundary, side) of block b: q = 0, 2 LOW, q = 1, 3 HIGH"""
    e = byte - 127
    pin = pin_of(byte, dtype)
    tri = triples_of(byte, dtype)
    high = bool(q & 1)
    elems = []
    for i in (HIGH_BOUNDARIES if high else LOW_BOUNDARIES):
        for sign in (1.0, -1.0):
            for side in SIDES:
                if (i, side) in tri:
                    m = tri[(i, side)]
                    elems.append((sign * m if m else 0.0, BOUNDARY, i, side))
    pool = _fill_pool(byte, dtype, pin, pin if high else math.ldexp(3.0, e))
    k = 0
    while len(elems) < BLOCK - 1:
        v = pool[(k + b) % len(pool)]
        elems.append((-v if v and (k + b) % 2 else v, FILL, -1, 0))
        k += 1
    if q >= 2:
        elems.reverse()
    return [(-pin if q >= 2 else pin, PIN, -1, 0)] + elems


def _quarter(pin: float, dtype: int, b: int) -> list:
    """31 T values of magnitude at most pin / 4 (no -0)"""
    out = []
    for k in range(BLOCK - 1):
        f = (0.25, -0.125, 0.0625, -0.25, 0.0, 0.125)[(k + b) % 6]
        v = float(NP.to_f32(NP.from_f32(np.array([pin * f], np.float32), dtype), dtype)[0])
        if abs(v) > pin / 4 or v == 0:
            v = 0.0
        out.append((v, FILL, -1, 0))
    return out


def edge_pins(dtype: int) -> list:
    """[(pin, scale byte)] of the edge class"""
    out = []
    for j in EDGE_EXPONENTS[dtype]:
        a = math.ldexp(1.5, j)
        out.append((a, max(j + 125, 0)))                      # m = 0.75, k = j + 1: e = j - 2
        out.append((neighbours(a, dtype)[1], max(j + 126, 0)))  # m just above 0.75: e = j - 1
    normal = math.ldexp(1.0, EMIN[dtype])                      # 0.5 * 2^(EMIN + 1): e = EMIN - 2
    out.append((normal, max(EMIN[dtype] + 125, 0)))
    out.append((neighbours(normal, dtype)[0], max(EMIN[dtype] + 125, 0)))  # m just below 1, k = EMIN
    return out


def _planted_block(byte: int, k: int) -> list:
    e = byte - 127
    others = (1.5, -1.25, 1.0, -0.75, 0.5, -0.25, 0.0, -1.5, 1.25, -1.0, 0.75, -0.5, 0.25)
    elems = [(math.ldexp(others[(i + k) % len(others)], e) if i else math.ldexp(1.5, e), FILL, -1, 0)
             for i in range(BLOCK - 1)]
    return [(math.ldexp(-6.0 if k % 2 else 6.0, e), PIN, -1, 0)] + elems


@functools.lru_cache(maxsize=None)
def table(dtype: int) -> Table:
    blocks, byte_of, cls_of = [], [], []

    def add(elems, byte, cls, roll):
        assert len(elems) == BLOCK
        r = roll % BLOCK
        blocks.append(elems[BLOCK - r:] + elems[:BLOCK - r])  # element 0, the pin, lands on position r
        byte_of.append(byte)
        cls_of.append(cls)

    bytes_ = list(BYTES[dtype])
    while len(blocks) < PINNED_BLOCKS:
        for q in range(4):
            for byte in bytes_:
                b = len(blocks)
                add(_pinned_block(b, byte, q, dtype), byte, HIGH if q & 1 else LOW, b)
    for pin, byte in edge_pins(dtype):
        b = len(blocks)
        add([(pin, PIN, -1, 0)] + _quarter(pin, dtype, b), byte, EDGE, b)
    for byte in PLANTED_BYTES[dtype]:
        for k in range(BLOCK):
            add(_planted_block(byte, k), byte, PLANTED, k)
    k = 0
    while len(blocks) % 3 or len(blocks) % 128 == 0:  # three chunks of whole blocks, a ragged last wave tile
        add(_planted_block(PLANTED_BYTES[dtype][1], k), PLANTED_BYTES[dtype][1], PLANTED, 7 * k + 3)
        k += 1
    nb = len(blocks)
    v = np.array([[el[0] for el in blk] for blk in blocks], np.float64)
    kind = np.array([[el[1] for el in blk] for blk in blocks], np.int8)
    bnd = np.array([[el[2] for el in blk] for blk in blocks], np.int8)
    side = np.array([[el[3] for el in blk] for blk in blocks], np.int8)
    pin_pos = np.argmax(kind == PIN, axis=1)
    assert ((kind == PIN).sum(axis=1) == 1).all()
    present = set()
    for byte in bytes_:
        present |= {(byte, i, s) for (i, s) in triples_of(byte, dtype)}
    left_out = frozenset((byte, i, s) for byte in bytes_ for i in range(len(BOUNDARIES)) for s in SIDES) - present
    x = to_t(v, dtype)
    x.setflags(write=False)
    return Table(dtype, x, np.array(byte_of, np.int64), np.array(cls_of, np.int8), pin_pos.astype(np.int64), kind, bnd,
                 side, frozenset(left_out))


# ------------------------------------------------------------ middle step ----
def segment(scales: np.ndarray, nibbles: np.ndarray) -> np.ndarray:
    """one segment (MXFP4.md, "Layout") from (nb,) scale bytes and (nb, 32) nibbles"""
    nb = scales.size
    sb = (nb + 31) // 32 * 32
    pb = (16 * nb + 31) // 32 * 32
    seg = np.zeros(sb + pb, np.uint8)
    seg[:nb] = scales
    nib = np.asarray(nibbles, np.uint8).reshape(nb, BLOCK)
    seg[sb:sb + 16 * nb] = (nib[:, 0::2] | (nib[:, 1::2] << 4)).ravel()
    return seg


def nibble(g: float) -> int:
    """sign << 3 | code of a signed grid value (+0 for 0)"""
    return GRID.index(abs(g)) | (8 if g < 0 else 0)


@dataclass(frozen=True)
class Middle:
    dtype: int
    p: int
    cs: int
    recv: np.ndarray      # the p received segments
    parts: np.ndarray     # (p, nb, 32) float64: what each segment's element decodes to
    want: np.ndarray      # (nb, 32) float64: the reduced value each element is built to have
    byte: np.ndarray      # (nb,) the scale byte of the encoded result
    bnd: np.ndarray       # (nb, 32) boundary index, -1 for the pin and the fillers
    side: np.ndarray      # (nb, 32)


# (segment 0, segment 1) in units of 2^e; segment 1 lies one scale byte lower, so its grid is halved
_EXACT_A = [((3, 3), -1), ((0, .25), 0), ((.5, .25), 1), ((1, .25), 2), ((1, .75), 3), ((2, .5), 4), ((3, .5), 5),
            ((4, 1), 6), ((1, -.25), 1), ((1.5, -.25), 2), ((2, -.25), 3), ((3, -.5), 4), ((4, -.5), 5), ((6, -1), 6),
            ((0, .75), 1)]
# both segments at the output's scale byte
_EXACT_B = [((3, 3), -1), ((2, .5), 4), ((3, .5), 5), ((4, 1), 6), ((1.5, 1), 4), ((2, 1.5), 5), ((3, 2), 6),
            ((1, 1.5), 4), ((.5, 3), 5), ((2, 3), 6), ((3, -.5), 4), ((4, -.5), 5), ((6, -1), 6), ((-.5, 3), 4),
            ((-.5, 4), 5), ((-1, 6), 6)]
MIDDLE_EXACT_BYTES = {F32: (0, 1, 2, 3, 64, 126, 127, 128, 129, 200, 251, 252),
                      F16: (104, 105, 106, 110, 112, 113, 114, 120, 127, 135, 139, 140),
                      BF16: (0, 1, 2, 3, 64, 126, 127, 128, 129, 200, 251, 252)}


def _mirror(elems):
    """the list and, for everything but the pin, its mirror image; padded with zero sums to 32"""
    out = list(elems) + [(tuple(-c for c in cs), i, s) for cs, i, s in elems[1:]]
    width = len(elems[0][0])
    pad = [((1,) + (0,) * (width - 1), -1, 0), ((0,) * width, -1, 0), ((-2,) + (0,) * (width - 1), -1, 0)]
    k = 0
    while len(out) < BLOCK:
        out.append(pad[k % 3])
        k += 1
    assert len(out) == BLOCK
    return out


def _build_middle(dtype: int, specs) -> Middle:
    """specs: [(out byte, (scale byte of each segment), [(grid units per segment, boundary, side)] * 32,
    (unit exponent of each segment relative to e))]"""
    p = len(specs[0][1])
    nb = len(specs)
    scales = np.zeros((p, nb), np.uint8)
    nibs = np.zeros((p, nb, BLOCK), np.uint8)
    parts = np.zeros((p, nb, BLOCK), np.float64)
    bnd = np.full((nb, BLOCK), -1, np.int8)
    side = np.zeros((nb, BLOCK), np.int8)
    want = np.zeros((nb, BLOCK), np.float64)
    byte = np.zeros(nb, np.int64)
    for b, (ob, sbytes, elems, _) in enumerate(specs):
        r = (3 * b) % BLOCK
        elems = elems[BLOCK - r:] + elems[:BLOCK - r]
        byte[b] = ob
        for j, (cs, i, s) in enumerate(elems):
            bnd[b, j], side[b, j] = i, s
            for y in range(p):
                # cs[y] is in units of 2^(ob - 127); segment y's own unit is 2^(sbytes[y] - 127)
                g = cs[y] * 2.0 ** (ob - sbytes[y])
                scales[y, b] = sbytes[y]
                nibs[y, b, j] = nibble(g)
                parts[y, b, j] = math.ldexp(cs[y], ob - 127)
            want[b, j] = math.fsum(parts[:, b, j])
    recv = np.concatenate([segment(scales[y], nibs[y]) for y in range(p)])
    return Middle(dtype, p, nb * BLOCK, recv, parts, want, byte, bnd, side)


@functools.lru_cache(maxsize=None)
def middle_exact(dtype: int) -> Middle:
    """p = 2: under a pin 3 + 3 = 6, sums that are exactly the boundaries (side 0), both signs.  Form A
    (segment 1 one scale byte below segment 0) reaches the odd quarters; form B has both segments at
    the output's byte and reaches the lowest byte."""
    specs = []
    lowest = MIDDLE_EXACT_BYTES[dtype][0]
    for ob in MIDDLE_EXACT_BYTES[dtype]:
        for form in ("A", "B"):
            if form == "A" and ob == lowest:
                continue
            base = [(cs, i, 0) for cs, i in (_EXACT_A if form == "A" else _EXACT_B)]
            for rep in range(2):
                specs.append((ob, (ob, ob - 1) if form == "A" else (ob, ob), _mirror(base), None))
    return _build_middle(dtype, specs)


# p = 3, f32: segment 2 lies d scale bytes below the output's and holds t grid units of 2^(e - d);
# entries (segment 0, segment 1, t), boundary, side.  The tree adds segment 2 to segment 0 first.
_NEAR = {
    24: [((0, .25, .5), 0, 1), ((.5, .25, -1), 1, -1), ((.5, .25, 1), 1, 1), ((0, .75, -1), 1, -1), ((0, .75, 1), 1, 1),
         ((1, .25, -2), 2, -1), ((1, .25, 2), 2, 1), ((1, .75, -2), 3, -1), ((1, .75, 2), 3, 1),
         ((2, .5, -4), 4, -1), ((2, .5, 4), 4, 1), ((3, .5, -4), 5, -1), ((3, .5, 4), 5, 1), ((1, .25, 0), 2, 0),
         ((3, .5, 0), 5, 0)],
    21: [((4, 1, -1), 6, -1), ((4, 1, 1), 6, 1), ((2, 3, -1), 6, -1), ((2, 3, 1), 6, 1), ((2, .5, -.5), 4, -1),
         ((2, .5, .5), 4, 1), ((3, .5, -.5), 5, -1), ((3, .5, .5), 5, 1), ((.5, 3, -.5), 5, -1), ((.5, 3, .5), 5, 1),
         ((4, 1, 0), 6, 0), ((2, .5, 0), 4, 0)],
    26: [((0, .25, -1), 0, -1), ((0, .25, 2), 0, 1), ((0, .75, -4), 1, -1), ((0, .75, 4), 1, 1), ((0, .25, 0), 0, 0),
         ((0, .75, 0), 1, 0)],
}
MIDDLE_NEIGHBOUR_BYTES = (26, 27, 64, 100, 126, 127, 128, 160, 200, 251, 252)


@functools.lru_cache(maxsize=None)
def middle_neighbours() -> Middle:
    """p = 3, f32: the boundaries' one-ulp neighbours.  An f32 ulp of the smallest boundary is
    2^(e - 26), which a third segment can hold only from scale byte 26 up."""
    specs = []
    for ob in MIDDLE_NEIGHBOUR_BYTES:
        for d, elems in _NEAR.items():
            pin = ((3, 3, 0), -1, 0)
            # t counts units of 2^(e - d): in units of 2^e it is t * 2^-d
            base = [pin] + [((c0, c1, t * 2.0 ** -d), i, s) for (c0, c1, t), i, s in elems]
            specs.append((ob, (ob, ob - 1, ob - d), _mirror(base), None))
    return _build_middle(F32, specs)
