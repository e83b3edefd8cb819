"""Planted-extremum inputs for the min/max passes (CPU only, shared by the
planted tests).

A MinMax-UInt8 header depends on exactly two elements of a chunk.  A pass that
never folds some region still passes a random-data test unless one of those
two elements happens to lie in that region.  Here the base data stays inside a
narrow band and one element per role is *planted* outside it, at a position
named after the region of the kernel that has to fold it.  Every positive plant
is self-checked (`build` raises otherwise): without it the chunk's min (max)
is different, so the oracle's header changes when that one element is
restored to its base value -- no case can be vacuous.

Plant kinds (all dtypes):
  margin        base uniform in [-1e-3, 1e-3]; max = +1.0, min = -1.0
  ulp           base = 0.37 rounded to T; max / min = the next T value above /
                below it (a fold at lower precision than T, or on the wrong
                half of a packed 16-bit pair, loses it)
  signed_zero   base {+0, positives}; min = a single -0 (max: +1.0)
  signed_zero_mirror
                base {-0, negatives}; max = a single +0 (min: -1.0)
A fold that compares floats (-0 == +0) fails the last two.

Positions are expressed through the kernels' own geometry, restated below
with the source line each formula comes from.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import oracle_np as NP

F32, F16, BF16 = 0, 1, 2
DTYPE_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
STORAGE = {F32: np.float32, F16: np.float16, BF16: np.uint16}
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
KINDS = ("margin", "ulp", "signed_zero", "signed_zero_mirror")

K_BLOCK = 256            # codec_common.hpp:17 kBlock
K_PARTIALS_SUB = 8       # minmax_u8.hip:40 kPartialsSub
K_PARTIALS_BLOCKS = 1024  # minmax_u8.hip:41 kPartialsBlocks
K_TARGET_BLOCKS = 2048   # launch_util.hpp:15 kTargetBlocks (bagua_minmax_u8_workspace_bytes)
TILE = K_BLOCK * K_PARTIALS_SUB  # vectors per workgroup iteration of minmax_partials_kernel


def esize(dtype: int) -> int:
    return 4 if dtype == F32 else 2


def vec_n(dtype: int) -> int:
    """elements per 16-byte vector (Vec<T>::N)"""
    return 16 // esize(dtype)


# ------------------------------------------------------------ T values ----
def t_bits(v: float, dtype: int) -> int:
    return int(NP.from_f32(np.array([v], np.float32), dtype).view(BITS[dtype])[0])


def t_next(bits: int, dtype: int, up: bool) -> int:
    """bits of the next T value above / below a finite, nonzero T value"""
    sign = bits >> (8 * esize(dtype) - 1)
    away = up != bool(sign)  # larger magnitude
    return bits + 1 if away else bits - 1


def nan_bits(dtype: int) -> int:
    return {F32: 0x7FC00000, F16: 0x7E00, BF16: 0x7FC0}[dtype]


def neg_zero_bits(dtype: int) -> int:
    return 0x80000000 if dtype == F32 else 0x8000


def huge_bits(dtype: int, negative: bool) -> int:
    """+-INIT_MAX / 2 in T (the negative plants)"""
    v = np.float32(NP.INIT_MAX[dtype]) / np.float32(2)
    return t_bits(-v if negative else v, dtype)


# ------------------------------------------------------------ base data ----
@functools.lru_cache(maxsize=4)
def base_data(dtype: int, kind: str, n: int, seed: int) -> np.ndarray:
    """n elements of T (storage dtype) strictly inside the kind's band; shared between
    the cases that ask for the same one, so read-only"""
    rng = np.random.default_rng(seed)
    if kind == "margin":
        v = (rng.random(n, dtype=np.float32) * np.float32(2) - np.float32(1)) * np.float32(1e-3)
    elif kind == "ulp":
        v = np.full(n, 0.37, np.float32)
    elif kind in ("signed_zero", "signed_zero_mirror"):
        v = np.float32(1e-4) + rng.random(n, dtype=np.float32) * np.float32(9e-4)
        v[rng.random(n, dtype=np.float32) < 0.5] = 0.0
        if kind == "signed_zero_mirror":
            v = -v  # {-0, negatives}
    else:
        raise ValueError(f"unknown plant kind {kind!r}")
    x = NP.from_f32(v, dtype)
    x.setflags(write=False)
    return x


def plant_bits(dtype: int, kind: str, role: str) -> int:
    """the planted T value of a kind, as bits"""
    assert role in ("min", "max")
    if kind == "ulp":
        return t_next(t_bits(0.37, dtype), dtype, up=(role == "max"))
    if kind == "signed_zero" and role == "min":
        return neg_zero_bits(dtype)
    if kind == "signed_zero_mirror" and role == "max":
        return 0
    return t_bits(1.0 if role == "max" else -1.0, dtype)


# --------------------------------------------------------------- plants ----
@dataclass(frozen=True)
class Plant:
    chunk: int
    index: int   # element index inside the chunk
    role: str    # "min" or "max"
    name: str    # the region, for assertion messages

    def __str__(self):
        return f"{self.role}@{self.name}[chunk {self.chunk} elem {self.index}]"


def _key(xf: np.ndarray) -> np.ndarray:
    """the total order the reference's min/max uses: -0 < +0 (oracle_np.minmax)"""
    i = np.ascontiguousarray(xf, np.float32).view(np.int32)
    return i ^ ((i >> 31) & 0x7FFFFFFF)


def _extreme_key(xf: np.ndarray, role: str):
    k = _key(xf[~np.isnan(xf)])
    if k.size == 0:
        return None
    return int(k.min() if role == "min" else k.max())


_base_extremes = {}  # (id(base), chunk, valid) -> (base, min key, max key); base kept alive, so the id stays its own


def check_plants(x: np.ndarray, base: np.ndarray, dtype: int, p: int, plants, num_elem: int | None = None,
                 base_extremes: dict | None = None, changed=None):
    """The self-check: every plant lies in its chunk's valid prefix, and the chunk's
    min (max) with the plant differs from its min (max) with that one element
    restored to its base value: the plant lies strictly outside everything else in the
    chunk.  `changed`: the global indices where x differs from base, when the caller knows
    them.  Raises ValueError otherwise."""
    cs = x.size // p
    n_in = x.size if num_elem is None else num_elem
    cache = _base_extremes if base_extremes is None else base_extremes
    if cache is _base_extremes and cache and next(iter(cache.values()))[0] is not base:
        cache.clear()  # the module's cache holds the latest base only
    changed = np.nonzero(x.view(BITS[dtype]) != base.view(BITS[dtype]))[0] if changed is None else np.asarray(changed, np.int64)
    for pl in plants:
        valid = max(0, min(n_in - pl.chunk * cs, cs))
        if not (0 <= pl.chunk < p and 0 <= pl.index < valid):
            raise ValueError(f"plant {pl} is outside the chunk's {valid} valid elements")
        lo = pl.chunk * cs
        # the chunk's extreme with this element at its base value: over the base chunk (once
        # per chunk; it holds the plant's own base value) and every other changed element
        key = (id(base), pl.chunk, valid)
        if key not in cache:
            seg = NP.to_f32(base[lo:lo + valid], dtype)
            cache[key] = (base, _extreme_key(seg, "min"), _extreme_key(seg, "max"))
        others = changed[(changed >= lo) & (changed < lo + valid) & (changed != lo + pl.index)]
        rest = [cache[key][1 if pl.role == "min" else 2], _extreme_key(NP.to_f32(x[others], dtype), pl.role)]
        rest = [k for k in rest if k is not None]
        mine = _extreme_key(NP.to_f32(x[lo + pl.index:lo + pl.index + 1], dtype), pl.role)
        decides = mine is not None and all(mine < k if pl.role == "min" else mine > k for k in rest)
        if not decides:
            raise ValueError(f"plant {pl} does not decide the chunk's {pl.role}: a pass that skips it would go unseen")


def build(dtype: int, kind: str, p: int, cs: int, plants, seed: int = 0, nan: bool = False,
          vector_origin=None, num_elem: int | None = None, base: np.ndarray | None = None):
    """(x, base): p*cs elements of T with the plants applied, self-checked.

    nan: NaN goes into every other element of each plant's 16-byte vector (the
    elements at an odd distance from the plant); `vector_origin(chunk)` is the
    chunk-relative index of an element that starts a vector (the scalar head's
    length), so that the vector is the one the kernel loads."""
    if base is None:
        base = base_data(dtype, kind, p * cs, seed)
    assert base.size == p * cs
    x = base.copy()
    xb = x.view(BITS[dtype])
    ed = edits(dtype, kind, p, cs, plants, nan, vector_origin, num_elem)
    for i, bits in ed.items():
        xb[i] = bits
    check_plants(x, base, dtype, p, plants, num_elem, changed=sorted(ed))
    return x, base


def edits(dtype: int, kind: str, p: int, cs: int, plants, nan: bool = False, vector_origin=None,
          num_elem: int | None = None) -> dict:
    """global element index -> T bits of everything `build` changes in the base data (for a
    test that rewrites only these elements of a buffer it keeps on the device)"""
    taken = {(pl.chunk, pl.index) for pl in plants}
    if len(taken) != len(plants):
        raise ValueError("two plants on one element")
    n_in = p * cs if num_elem is None else num_elem
    N, out = vec_n(dtype), {}
    for pl in plants:
        if not (0 <= pl.chunk < p and 0 <= pl.index < cs):
            raise ValueError(f"plant {pl} is outside the chunk")
        out[pl.chunk * cs + pl.index] = plant_bits(dtype, kind, pl.role)
        if nan:
            valid = max(0, min(n_in - pl.chunk * cs, cs))
            org = vector_origin(pl.chunk) if vector_origin else 0
            v0 = pl.index - ((pl.index - org) % N)
            for j in range(max(v0, 0), min(v0 + N, valid)):
                if (j - pl.index) % 2 and (pl.chunk, j) not in taken:
                    out[pl.chunk * cs + j] = nan_bits(dtype)
    return out


def plant_negative(x: np.ndarray, dtype: int, index: int, num_elem: int, negative: bool):
    """A huge finite value at a global element index at or past input_num_element: it
    must NOT enter any header (the oracle decides its payload byte)."""
    if index < num_elem or index >= x.size:
        raise ValueError(f"negative plant at {index} is inside the valid prefix of {num_elem} (or past the input)")
    x.view(BITS[dtype])[index] = huge_bits(dtype, negative)


def header_bits(buf: np.ndarray, dtype: int, p: int, chunk: int):
    """(min bits, max bits) of a chunk's header in a compressed buffer"""
    co = buf.size // p
    es = esize(dtype)
    h = buf[chunk * co:chunk * co + 2 * es]
    b = h.view(BITS[dtype])
    return int(b[0]), int(b[1])


def plants_of(plants, chunk: int) -> str:
    return ", ".join(str(pl) for pl in plants if pl.chunk == chunk)


def assert_headers(got: np.ndarray, want: np.ndarray, dtype: int, p: int, plants, what: str, chunks=None):
    """the headers first, naming the planted regions of the chunk that differs"""
    for c in (range(p) if chunks is None else chunks):
        g, w = header_bits(got, dtype, p, c), header_bits(want, dtype, p, c)
        assert g == w, (f"{what}: header of chunk {c} is {g[0]:#x}/{g[1]:#x}, the oracle's {w[0]:#x}/{w[1]:#x}; "
                        f"planted: {plants_of(plants, c) or 'nothing'}")


# ------------------------------------------- two-pass encode geometry ----
def partials_blocks(cs: int, dtype: int, nact: int, ws_bytes: int | None = None) -> int:
    """gridDim.x of minmax_partials_kernel: minmax_u8.hip:504-520 (blocks_for with
    sub = kPartialsSub, target = kPartialsBlocks, then the workspace cap)"""
    nvec = cs // vec_n(dtype) + 1
    tiles = (nvec + TILE - 1) // TILE
    per_chunk = (K_PARTIALS_BLOCKS + nact - 1) // nact
    nblk = max(1, min(tiles, per_chunk))
    if ws_bytes is not None:
        cap = (ws_bytes // 8) // max(nact, 1)
        nblk = min(nblk, cap)
    return nblk


@dataclass(frozen=True)
class TwoPass:
    """minmax_partials_kernel's view of one chunk (minmax_u8.hip:81-97): a scalar head up
    to the first 128-byte line, `nvec` 16-byte vectors in tiles of TILE, a scalar tail."""
    dtype: int
    valid: int      # valid elements of the chunk (chunk_valid)
    head: int       # scalar head elements (j0)
    nvec: int
    grid: int       # gridDim.x
    rev: bool = False

    @property
    def N(self):
        return vec_n(self.dtype)

    @property
    def tail(self):
        return self.valid - self.head - self.nvec * self.N

    @property
    def ntile(self):
        return (self.nvec + TILE - 1) // TILE

    @property
    def full_tiles(self):
        return self.nvec // TILE

    def elem(self, vec: int, lane: int = 0) -> int:
        assert 0 <= vec < self.nvec and 0 <= lane < self.N
        return self.head + vec * self.N + lane

    def swept(self, fwd_vec: int) -> int:
        """the vector a workgroup loads at sweep coordinate fwd_vec (minmax_u8.hip:97:
        base = REV ? (ntile - 1) * tile - fwd : fwd)"""
        t, w = divmod(fwd_vec, TILE)
        return ((self.ntile - 1 - t) if self.rev else t) * TILE + w


def two_pass(dtype: int, cs: int, chunk: int, nact: int, byte_offset: int = 0, num_elem: int | None = None,
             p: int | None = None, rev: bool = False, ws_bytes: int | None = None) -> TwoPass:
    """byte_offset: the input pointer's offset from a 128-byte line"""
    es, N = esize(dtype), vec_n(dtype)
    valid = cs if num_elem is None else max(0, min(num_elem - chunk * cs, cs))
    addr = byte_offset + chunk * cs * es
    head = ((128 - addr % 128) % 128) // es      # minmax_u8.hip:85
    if addr % es:
        head = valid                              # minmax_u8.hip:86 (all scalar)
    head = min(head, valid)
    return TwoPass(dtype, valid, head, (valid - head) // N, partials_blocks(cs, dtype, nact, ws_bytes), rev)


def two_pass_positions(g: TwoPass) -> dict:
    """name -> chunk-relative element index of every region of the pass that exists in
    this chunk.  Needs at least one full tile more than the grid has workgroups, and a
    ragged top tile, for all of them to exist."""
    N, pos = g.N, {}
    if g.head:
        pos["head_first"] = 0
        if g.head > 1:
            pos["head_last"] = g.head - 1
    if g.nvec:
        pos["body_vec0_lane0"] = g.elem(0, 0)
        pos["body_vec0_lane_last"] = g.elem(0, N - 1)
    if g.full_tiles >= 1:
        for k in range(1, K_PARTIALS_SUB):  # subtile 0's first vector is body_vec0
            pos[f"tile0_subtile{k}_first_vec"] = g.elem(k * K_BLOCK, k % N)
        for t in (63, 64, 255):
            pos[f"thread{t}_vec"] = g.elem(t, t % N)
        pos["full_tile_last_vec"] = g.elem(TILE - 1, N - 1)
    if g.full_tiles > g.grid:
        # tile index gridDim.x: workgroup 0's second grid-stride iteration
        pos[f"tile{g.grid}_second_iteration"] = g.elem(g.swept(g.grid * TILE + 3 * K_BLOCK + 129), 1)
    if g.nvec % TILE:
        pos["ragged_tile_first_vec"] = g.elem(g.full_tiles * TILE, 0)
        pos["ragged_tile_last_vec"] = g.elem(g.nvec - 1, N - 1)
    if g.tail:
        pos["tail_first"] = g.head + g.nvec * N
        if g.tail > 1:
            pos["tail_last"] = g.valid - 1
    return pos


def nt_positions(g: TwoPass, nt_until: int) -> dict:
    """the vectors either side of the non-temporal / default load split of the sweep
    (minmax_u8.hip:100: full tiles with fwd + tile <= nt_until load non-temporally), and
    one in the tile that straddles nt_until"""
    pos = {}
    N = g.N
    for name, f in (("below_nt_until", nt_until - 1), ("at_nt_until", nt_until),
                    ("straddling_tile_first_vec", nt_until // TILE * TILE),
                    ("last_nt_tile_last_vec", nt_until // TILE * TILE - 1)):
        if 0 <= f < g.ntile * TILE and g.swept(f) < g.nvec:
            pos[name] = g.elem(g.swept(f), f % N)
    return pos


def nt_until(nbytes: int, keep_bytes: int) -> int:
    """sweep coordinate (in vectors) up to which full tiles load non-temporally:
    minmax_u8.hip:577-578 (compress_impl, keep = (KEEP_MIB << 20) / nact > 0) and
    minmax_u8.hip:877 (one_rank_impl, keep < bytes)"""
    return (nbytes - keep_bytes) // 16 if nbytes > keep_bytes else 0


def paired_plants(positions_of_chunk, p: int, shift: int | None = None, skip=()) -> list:
    """One min and one max plant per chunk, in different regions; over the chunks every
    position takes both roles (p >= number of positions)."""
    per_chunk = {c: positions_of_chunk(c) for c in range(p) if c not in skip}
    order = []  # every region any chunk has, in first-seen order
    for pos in per_chunk.values():
        order += [n for n in pos if n not in order]
    L = len(order)
    s = L // 2 if shift is None else shift
    used = {"min": dict.fromkeys(order, 0), "max": dict.fromkeys(order, 0)}

    def pick(pos, start, role, avoid=None):
        # the region of this chunk that has had this role least often so far (ties: the
        # first from `start` on), so regions that few chunks have get both roles too
        best = None
        for k in range(L):
            n = order[(start + k) % L]
            if n in pos and (avoid is None or pos[n] != avoid) and (best is None or used[role][n] < used[role][best]):
                best = n
        if best is None:
            raise ValueError("a chunk has fewer than two plantable regions")
        used[role][best] += 1
        return best
    plants = []
    for c, pos in per_chunk.items():
        a = pick(pos, c, "min")
        b = pick(pos, c + s, "max", avoid=pos[a])
        plants.append(Plant(c, pos[a], "min", a))
        plants.append(Plant(c, pos[b], "max", b))
    return plants


def covered_names(plants) -> dict:
    """position name -> set of roles it was planted with"""
    out = {}
    for pl in plants:
        out.setdefault(pl.name, set()).add(pl.role)
    return out


# ---------------------------------------------- the two-pass test shape ----
SHAPE_A_P = 64  # 1024 / 64 = 16 workgroups per chunk


def shape_a_cs(dtype: int) -> int:
    """17 full tiles + a ragged tile of 3 subtiles and 5 vectors + 3 scalar elements (for a
    chunk that starts on a 128-byte line; cs is odd, so the chunks' heads differ in length)"""
    return (17 * TILE + 3 * K_BLOCK + 5) * vec_n(dtype) + 3


def shape_a_positions(dtype: int, c: int, p: int = SHAPE_A_P, byte_offset: int = 0, num_elem: int | None = None,
                      keep_mib: int | None = None) -> dict:
    """Every region of chunk c, for the forward sweep and (names starting rev_) for the
    backward one: its second grid-stride iteration, and with keep_mib (BAGUA_PARTIALS_KEEP_MIB)
    the vectors around the split between non-temporal and default loads."""
    cs = shape_a_cs(dtype)
    pos = two_pass_positions(two_pass(dtype, cs, c, p, byte_offset, num_elem, p))
    g = two_pass(dtype, cs, c, p, byte_offset, num_elem, p, rev=True)
    pos.update({"rev_" + n: i for n, i in two_pass_positions(g).items() if "second_iteration" in n})
    if keep_mib is not None:
        ntu = nt_until(cs * esize(dtype), (keep_mib << 20) // p)
        pos.update({"rev_" + n: i for n, i in nt_positions(g, ntu).items()})
    taken, out = set(), {}
    for n, i in pos.items():  # one name per element
        if i not in taken:
            out[n] = i
            taken.add(i)
    return out


def shape_a_plants(dtype: int, p: int = SHAPE_A_P, byte_offset: int = 0, num_elem: int | None = None,
                   keep_mib: int | None = None, chunks=None) -> list:
    """the plant pairs of the two-pass shape: chunk c gets one min and one max in different regions"""
    skip = () if chunks is None else [c for c in range(p) if c not in chunks]
    return paired_plants(lambda c: shape_a_positions(dtype, c, p, byte_offset, num_elem, keep_mib), p, skip=skip)


def shape_a_origin(dtype: int, p: int = SHAPE_A_P, byte_offset: int = 0):
    cs = shape_a_cs(dtype)
    return lambda c: two_pass(dtype, cs, c, p, byte_offset).head


# ------------------------------------------- fused reduce and the ring ----
def reduce_by(p: int) -> int:
    """width of the reference's summation tree (segment_cases.reduce_by)"""
    return 2 if p <= 4 else 4 if p <= 8 else 8 if p <= 16 else 16 if p <= 32 else 32


def fused_positions(dtype: int, p: int, cs: int) -> dict:
    """Regions of the fused dequantise+reduce kernels (reduce.hip:196-262 reduce_tiles): a tile
    is kBlock * Q vectors, Q = max(1, 64 / (N * BY)); full tiles, a partial last tile, a
    scalar tail of fewer than N elements."""
    N = vec_n(dtype)
    q = max(1, 64 // (N * reduce_by(p)))
    tile = K_BLOCK * q * N  # elements
    nvec = cs // N
    pos = {"first_vector_lane0": 0, "first_vector_last_lane": N - 1,
           "last_vector_lane0": (nvec - 1) * N, "last_element": cs - 1}
    full = cs // tile
    for t in range(1, full + 1):
        pos[f"tile{t - 1}_last_element"] = t * tile - 1
        if t * tile < cs:
            pos[f"tile{t}_first_element"] = t * tile
    rem = nvec * N - full * tile
    if rem > 2 * N:
        pos["sub_tile_remainder_middle"] = full * tile + rem // (2 * N) * N + 1
    if cs - nvec * N:
        pos["scalar_tail_first"] = nvec * N
    out, taken = {}, set()
    for n, i in pos.items():
        if i not in taken:
            out[n] = i
            taken.add(i)
    return out


def piece_positions(ranges) -> dict:
    """both sides of every piece boundary, and the middle of the shortest non-empty piece
    (its workgroups leave partial slots of the workspace unused)"""
    pos = {}
    live = [(b, e) for b, e in ranges if e > b]
    for q, (b, e) in enumerate(live[:-1]):
        pos[f"piece{q}_last_element"] = e - 1
        pos[f"piece{q + 1}_first_element"] = e
    b, e = min(live, key=lambda r: r[1] - r[0])
    pos.setdefault("shortest_piece_middle", (b + e) // 2)
    pos.setdefault("chunk_first_element", live[0][0])
    pos.setdefault("chunk_last_element", live[-1][1] - 1)
    out, taken = {}, set()
    for n, i in pos.items():
        if i not in taken:
            out[n] = i
            taken.add(i)
    return out


def rotate_pairs(pos: dict) -> list:
    """[(min name, max name)]: every position once in each role"""
    names = list(pos)
    return [(a, names[(i + len(names) // 2) % len(names)]) for i, a in enumerate(names)]


def received_base(p: int, cs: int, seed: int) -> np.ndarray:
    """p payloads of bytes uniform in [64, 191] (p x cs)"""
    return np.random.default_rng(seed).integers(64, 192, (p, cs), dtype=np.uint8)


def planted_received(build_received, dtype: int, base: np.ndarray, min_index: int, max_index: int) -> np.ndarray:
    """The receive buffer (segment_cases.build_received) with benign headers {-1e-3, 1e-3}: byte
    255 at the planted maximum and byte 0 at the planted minimum in EVERY segment, so the
    reduced extremum is unique for any p.  (-1, -1): the base alone."""
    p, cs = base.shape
    pay = base.copy()
    if min_index >= 0:
        if not (0 <= min_index < cs and 0 <= max_index < cs and min_index != max_index):
            raise ValueError("planted position outside the chunk")
        pay[:, max_index] = 255
        pay[:, min_index] = 0
    return build_received(dtype, cs, [(-1e-3, 1e-3, pay[c]) for c in range(p)])


def ring_positions(dtype: int, n: int) -> dict:
    """Regions of ring_mix_kernel (decentralized.hip:111-189): 16-byte vectors in tiles of
    U * kBlock (U = 2, 4 or 8 by launch shape: vector 2048 starts a tile of every shape), the last
    full vector, and every element of the ragged tail, which workgroup 0 mixes one per thread."""
    N = vec_n(dtype)
    nvec = n // N
    pos = {"first_vector_lane0": 0, "tile_edge_last_lane_below": 2048 * N - 1, "tile_edge_lane0_above": 2048 * N,
           "last_full_vector_last_lane": nvec * N - 1}
    for j in range(nvec * N, n):
        pos[f"ragged_tail_element{j - nvec * N}"] = j
    if max(pos.values()) >= n or nvec <= 2048:
        raise ValueError("the tensor is too short for these regions")
    return pos


# ------------------------------------------------- 1-bit planted mass ----
OB_TILE = 1024   # onebit_common.hpp kObTile: elements per |x| tile partial, partials per tree group


def onebit_positions(cs: int, tile_ranges) -> dict:
    """Regions of the 1-bit codec's |x| pass and scale tree: the first tile, the last tile of the
    first level-1 group of 1024 tile partials, the first tile of the next group, the ragged last
    tile, and the tiles either side of every piece boundary (bagua_onebit_piece_range)."""
    tiles = (cs + OB_TILE - 1) // OB_TILE
    if tiles <= OB_TILE or cs % OB_TILE == 0:
        raise ValueError("the chunk needs more than one level-1 group and a ragged last tile")
    pos = {"tile0_first_element": 0, "tile0_last_element": OB_TILE - 1,
           "group0_last_tile_first_element": (OB_TILE - 1) * OB_TILE, "group0_last_tile_last_element": OB_TILE * OB_TILE - 1,
           "group1_first_tile_first_element": OB_TILE * OB_TILE, "group1_first_tile_last_element": (OB_TILE + 1) * OB_TILE - 1,
           "ragged_last_tile_first_element": (tiles - 1) * OB_TILE, "ragged_last_tile_last_element": cs - 1}
    live = [(b, e) for b, e in tile_ranges if e > b]
    for q, (b, e) in enumerate(live[:-1]):
        pos[f"piece{q}_last_element"] = e * OB_TILE - 1
        pos[f"piece{q + 1}_first_element"] = e * OB_TILE
    return pos


def planted_mass(dtype: int, p: int, cs: int, indices, seed: int) -> np.ndarray:
    """p chunks of +-0 with random signs (the sign bits are not trivial) and a single 1.0 at
    indices[c] of chunk c: the chunk's scale is nonzero only if the |x| tile partial that holds
    it reaches the scale tree's root.  Raises for a position outside the chunk."""
    rng = np.random.default_rng(seed)
    bits = np.where(rng.random(p * cs) < 0.5, neg_zero_bits(dtype), 0).astype(BITS[dtype])
    if len(indices) != p:
        raise ValueError("one planted element per chunk")
    for c, i in enumerate(indices):
        if not 0 <= i < cs:
            raise ValueError(f"planted mass at {i} is outside the chunk of {cs}")
        bits[c * cs + i] = t_bits(1.0, dtype)
    return bits.view(STORAGE[dtype])


def check_mass(want: np.ndarray, p: int, names):
    """the self-check of the planted mass: the oracle's scale (the f32 at the start of a
    segment) of every chunk is nonzero with the single 1.0 and would be 0 without it"""
    co = want.size // p
    for c in range(p):
        if want[c * co:c * co + 4].view(np.float32)[0] == 0:
            raise ValueError(f"the planted 1.0 at {names[c]} does not reach the oracle's scale of chunk {c}")


# ------------------------------------------ one-launch encode geometry ----
def common_alignment(dtype: int, t_addr: int, byte_addr: int) -> int:
    """codec_common.hpp:224-232: the scalar head of a (T stream, payload byte stream) pair"""
    N, es = vec_n(dtype), esize(dtype)
    j1 = (128 - byte_addr % 128) % 128
    if (t_addr + j1 * es) % 16 == 0:
        return j1
    for j in range(N):
        if (t_addr + j * es) % 16 == 0 and (byte_addr + j) % N == 0:
            return j
    return -1


@dataclass(frozen=True)
class Resident:
    """One chunk as the one-launch encode cuts it (minmax_resident.hip:137-153 SliceGeom):
    a scalar head j0, nvec body vectors in `bpc` slices of `per` vectors (the last one
    shorter), a scalar tail.  A slice is rows of `block` vectors: rows [0, re) held in
    VGPRs, [re, re + h) parked in LDS, [re + h, re + h + rl) held late, the rest streamed
    in tiles of sb rows (bagua_minmax_u8_resident_cfg_geometry / _cfg_order)."""
    dtype: int
    cs: int
    j0: int
    nvec: int
    bpc: int
    block: int
    re: int
    h: int
    rl: int
    sb: int

    @property
    def per(self):
        return ((self.nvec + self.bpc - 1) // self.bpc + self.block - 1) // self.block * self.block

    def slice_range(self, b: int):
        v0 = min(b * self.per, self.nvec)
        return v0, min(v0 + self.per, self.nvec)

    def elem(self, b: int, row: int, thread: int, lane: int) -> int:
        """element of slice b's vector (row, thread); raises if the slice does not hold it"""
        v0, v1 = self.slice_range(b)
        v = v0 + row * self.block + thread
        if not (0 <= thread < self.block and 0 <= lane < vec_n(self.dtype) and v0 <= v < v1):
            raise ValueError(f"slice {b} has no vector at row {row}, thread {thread}")
        return self.j0 + v * vec_n(self.dtype) + lane


def resident(dtype: int, cs: int, chunk: int, bpc: int, geom, in_addr: int, out_addr: int, chunk_offset: int) -> Resident:
    """geom = (block, re, h, rl, sb) of the row; the addresses are the launch's input and output pointers"""
    block, re, h, rl, sb = geom
    j0 = common_alignment(dtype, in_addr + chunk * cs * esize(dtype), out_addr + chunk * chunk_offset + 32)
    if j0 < 0:
        raise ValueError("the chunk is not eligible for the one-launch encode (no common alignment)")
    j0 = min(j0, cs)
    return Resident(dtype, cs, j0, (cs - j0) // vec_n(dtype), bpc, block, re, h, rl, sb)


def resident_positions(g: Resident) -> dict:
    """name -> (slice, element) for slice 0, a middle slice and the last slice of the chunk: the
    first and last row of each on-chip region, lane 0 and the last lane of the first, the second
    and the ragged top streamed tile; for the last slice also the chunk's scalar head, scalar
    tail and last vector.  Raises when the shape lacks one of the regions (it must have two
    full streamed tiles and a ragged top in every slice)."""
    N, B = vec_n(g.dtype), g.block
    on_chip = g.re + g.h + g.rl
    pos = {}
    for tag, b in (("first", 0), ("middle", g.bpc // 2), ("last", g.bpc - 1)):
        v0, v1 = g.slice_range(b)
        streamed = v1 - v0 - on_chip * B
        if streamed <= 2 * g.sb * B or streamed % (g.sb * B) == 0:
            raise ValueError(f"slice {b} has no ragged top tile above two full streamed tiles")

        def put(name, row, thread, lane):
            pos[f"slice_{tag}_{name}"] = (b, g.elem(b, row, thread, lane))
        put("early_first_row", 0, 0, 0)
        put("early_last_row", g.re - 1, B - 1, N - 1)
        put("parked_first_row", g.re, 1, 0)
        put("parked_last_row", g.re + g.h - 1, B - 2, N - 1)
        if g.rl > 0:
            put("late_first_row", g.re + g.h, 63, 1)
            put("late_last_row", on_chip - 1, 64, N - 2)
        for k, name in ((0, "streamed_tile0"), (1, "streamed_tile1")):
            put(name + "_lane0", on_chip + k * g.sb, 0, 0)
            put(name + "_last_lane", on_chip + (k + 1) * g.sb - 1, B - 1, N - 1)
        put("ragged_top_lane0", on_chip + 2 * g.sb, 0, 0)
        top = v1 - 1 - (1 if tag == "last" else 0)  # the last slice's last vector is chunk_last_vector
        pos[f"slice_{tag}_ragged_top_last_lane"] = (b, g.j0 + top * N + N - 1)
        assert (top - v0) // B >= on_chip + 2 * g.sb
    last = g.bpc - 1
    pos["chunk_last_vector"] = (last, g.j0 + (g.nvec - 1) * N + N - 1)
    if g.j0:
        pos["scalar_head_first"] = (last, 0)
        if g.j0 > 1:
            pos["scalar_head_last"] = (last, g.j0 - 1)
    if g.cs - g.j0 - g.nvec * N:
        pos["scalar_tail_first"] = (last, g.j0 + g.nvec * N)
        if g.cs - g.j0 - g.nvec * N > 1:
            pos["scalar_tail_last"] = (last, g.cs - 1)
    return pos


def cross_slice_pairs(pos: dict) -> list:
    """[(min name, max name)]: every position once as the minimum and once as the maximum, the
    two of a pair always in different slices (a wrong exchange shows as well as a wrong fold)"""
    names = list(pos)
    n = len(names)
    pairs = []
    for i, a in enumerate(names):
        j = (i + n // 3) % n
        while pos[names[j]][0] == pos[a][0] or pos[names[j]][1] == pos[a][1]:
            j = (j + 1) % n
        pairs.append((a, names[j]))
    for b in names:  # whatever the walk above left without the maximum's role
        if all(mx != b for _, mx in pairs):
            a = next(a for a in names if pos[a][0] != pos[b][0])
            pairs.append((a, b))
    return pairs
