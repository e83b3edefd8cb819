"""Hostile gradients and the dispatch-path table of the comm-op edge tests.

The codec, reduce and ring kernels are tested one at a time on hostile data; the layer that
composes them (csrc/runtime/comm_ops.cpp) picks, per call, which of them run and in which
order.  This module holds what both tests/test_op_edges_cpu.py (the reference is sound on
these inputs) and tests/test_gpu_op_edges.py (the op equals the reference, and took the
path the table says) need: no GPU, no torch.

Inputs.  Benign data is standard_normal * 1e-3 + 0.01 * r, rounded to T.  A class plants its
values on rank p - 1 in chunk p - 1 and, from p >= 4, in chunk 0 as well (planted_chunks):
never more than half of the chunks, so a NaN result cannot hide a wrong chunk elsewhere.

  benign              nothing
  one_nan             one NaN in the middle of the chunk
  all_nan_chunk       the whole chunk NaN
  pos_inf             one +inf at element 1
  neg_inf             one -inf at the last element
  inf_cancel          +inf on rank p - 1 and -inf on rank 0 at the same element
  constant            the whole chunk 0.5 on rank p - 1
  all_ranks_constant  the chunk 0.25 on every rank (max == min in the reduced chunk too)
  zero / neg_zero     the chunk +0 / -0
  denormal            integer multiples (-3..3) of the smallest denormal of T
  huge                +-3e38 (f32, bf16) or +-60000 (f16) on the first two elements of the
                      chunk on EVERY rank: the f16 sum overflows

Tail classes (partially valid tensor): num_elem = n - short, the elements past it hold NaN,
+inf, -inf or 3e4 on every rank, the valid part is benign.

Ring classes (decentralized op, values on rank p - 1): one_nan in t, w_nan in weight,
pos_inf in left[0], neg_inf in right[-1], huge in t, and constant / zero / neg_zero /
denormal in all four tensors.

Paths.  PATHS lists every dispatch path with the kernels that must and must not be launched
on it, written from comm_ops.cpp (line numbers in the comments below), never from a run.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import oracle_np as NP

F32, F16, BF16 = 0, 1, 2
DTYPE_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
MINMAX, ONEBIT = "MinMaxUInt8", "OneBitSignScale"
NAN, INF = float("nan"), float("inf")

CLASSES = ["benign", "one_nan", "all_nan_chunk", "pos_inf", "neg_inf", "inf_cancel", "constant",
           "all_ranks_constant", "zero", "neg_zero", "denormal", "huge"]
TAIL_CLASSES = ["tail_nan", "tail_pos_inf", "tail_neg_inf", "tail_3e4"]
TAIL_VALUE = {"tail_nan": NAN, "tail_pos_inf": INF, "tail_neg_inf": -INF, "tail_3e4": 3e4}
RING_CLASSES = ["benign", "one_nan", "w_nan", "pos_inf", "neg_inf", "huge", "constant", "zero", "neg_zero",
                "denormal"]
EF_CLASSES = ["benign", "one_nan", "pos_inf", "zero", "huge"]
# what a function that runs longer than about ten seconds on the GPU is cut to
SHORT_CLASSES = ["benign", "one_nan", "inf_cancel", "huge", "neg_zero"]

# smallest denormal of T, exact in f32 (bf16's 2^-133 is an f32 denormal)
DENORMAL = {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}
HUGE = {F32: 3e38, F16: 60000.0, BF16: 3e38}


def planted_chunks(p: int) -> list[int]:
    return [p - 1] + ([0] if p >= 4 else [])


def case_rng(*key) -> np.random.Generator:
    """one generator per case, the same in the CPU and the GPU test"""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _benign32(p: int, n: int, rng, offset: float = 0.01) -> list[np.ndarray]:
    return [(rng.standard_normal(n) * 1e-3 + offset * r).astype(np.float32) for r in range(p)]


def _denormals(rng, n: int, dtype: int) -> np.ndarray:
    return (rng.integers(-3, 4, n).astype(np.float32) * np.float32(DENORMAL[dtype])).astype(np.float32)


def build(cls: str, p: int, cs: int, dtype: int, rng) -> list[np.ndarray]:
    """every rank's gradient (p * cs elements, storage dtype of T) for class `cls`"""
    assert cls in CLASSES, cls
    v = _benign32(p, p * cs, rng)
    for c in planted_chunks(p):
        b, e = c * cs, (c + 1) * cs
        own = v[p - 1][b:e]
        if cls == "one_nan":
            own[cs // 2] = NAN
        elif cls == "all_nan_chunk":
            own[:] = NAN
        elif cls == "pos_inf":
            own[1] = INF
        elif cls == "neg_inf":
            own[cs - 1] = -INF
        elif cls == "inf_cancel":
            own[cs // 3] = INF
            v[0][b + cs // 3] = -INF
        elif cls == "constant":
            own[:] = 0.5
        elif cls == "all_ranks_constant":
            for r in range(p):
                v[r][b:e] = 0.25
        elif cls == "zero":
            own[:] = 0.0
        elif cls == "neg_zero":
            own[:] = -0.0
        elif cls == "denormal":
            own[:] = _denormals(rng, cs, dtype)
        elif cls == "huge":
            for r in range(p):
                v[r][b] = HUGE[dtype]
                v[r][b + 1] = -HUGE[dtype]
    return [NP.from_f32(x, dtype) for x in v]


def build_tail(cls: str, p: int, cs: int, dtype: int, short: int, rng) -> tuple[list[np.ndarray], int]:
    """(gradients, num_elem): the last `short` elements of every rank hold the class's value"""
    n = p * cs
    v = _benign32(p, n, rng)
    for x in v:
        x[n - short:] = TAIL_VALUE[cls]
    return [NP.from_f32(x, dtype) for x in v], n - short


def build_ring(cls: str, p: int, n: int, dtype: int, rng) -> dict:
    """{"t", "w", "l", "r"}: each a list of every rank's tensor of n elements"""
    assert cls in RING_CLASSES, cls
    a = {k: [(rng.standard_normal(n) * 1e-3).astype(np.float32) for _ in range(p)] for k in "twlr"}
    last = p - 1
    if cls == "one_nan":
        a["t"][last][n // 2] = NAN
    elif cls == "w_nan":
        a["w"][last][n // 2] = NAN
    elif cls == "pos_inf":
        a["l"][last][0] = INF
    elif cls == "neg_inf":
        a["r"][last][n - 1] = -INF
    elif cls == "huge":
        a["t"][last][0] = HUGE[dtype]
        a["t"][last][1] = -HUGE[dtype]
    elif cls in ("constant", "zero", "neg_zero", "denormal"):
        for k in "twlr":
            a[k][last][:] = (_denormals(rng, n, dtype) if cls == "denormal"
                             else {"constant": 0.5, "zero": 0.0, "neg_zero": -0.0}[cls])
    return {k: [NP.from_f32(x, dtype) for x in a[k]] for k in "twlr"}


def is_nan(x: np.ndarray, dtype: int) -> np.ndarray:
    return np.isnan(NP.to_f32(x, dtype))


def is_finite(x: np.ndarray, dtype: int) -> np.ndarray:
    return np.isfinite(NP.to_f32(x, dtype))


# ---- the path table -----------------------------------------------------------------------
FUSED_REDUCE = ("dequant_reduce_kernel", "dequant_reduce_quantize_kernel")
ONEBIT_FUSED = ("onebit_reduce_encode_kernel", "onebit_reduce_encode_lut_kernel")
RESIDENT = ("minmax_resident_encode_kernel", "minmax_resident_encode_kernel_stack",
            "minmax_resident_encode_kernel_window")
RING_FUSED = ("ring_mix_kernel", "ring_apply_kernel", "ring_one_rank_kernel")

# The MinMax op at p = 3 needs S = align32(3 cs) + 96 divisible by 3 (the alltoall's
# alignment, communicators/mod.rs:603-607), i.e. cs a multiple of 32: three full 1024-element
# tiles and a partial one.  cs = 3076 (three tiles + 4, the 1-bit rows' shape) gives S = 9344
# = 3 * 3114 + 2, which the reference and the op refuse (REFUSED_MINMAX_SHAPE).
MM_P3_CS = 3 * 1024 + 32
REFUSED_MINMAX_SHAPE = (3, 3076)


@dataclass(frozen=True)
class Path:
    """One dispatch path of one op.

    op: "centralized", "ef" (error feedback) or "ring"; entry: the C entry point's suffix;
    size: cs (centralized, ef) or n (ring); pieces: the op's `pieces` argument (pipelined
    entries and ef); env: switches set before the communicators are created; short > 0: the
    partially valid op with the tail classes.
    must: every item is a kernel name, a tuple of alternatives (one of them appears), or a
    (name, count) pair (appears at least `count` times); must_not: names that may not appear.
    aligned16: whether the chunk's byte size is a multiple of 16."""
    name: str
    op: str
    entry: str
    codec: str
    p: int
    dtype: int
    size: int
    pieces: int = 0
    env: tuple = ()
    short: int = 0
    must: tuple = ()
    must_not: tuple = ()
    aligned16: bool = True
    classes: tuple = tuple(CLASSES)

    @property
    def id(self) -> str:
        return f"{self.name}-{self.entry}-p{self.p}-{DTYPE_NAME[self.dtype]}"

    @property
    def ref_key(self) -> tuple:
        """what the reference result depends on (not the entry, the pieces or the switches)"""
        return (self.op, self.codec, self.p, self.dtype, self.size, self.short)


def _paths() -> list[Path]:
    P: list[Path] = []

    def add(name, op, entry, codec, p, dtypes, size, **kw):
        for dt in dtypes:
            P.append(Path(name, op, entry, codec, p, dt, size, **kw))

    # ---- centralized, MinMaxUInt8 ----
    # centralized() :232-262: bagua_minmax_u8_reduce_requantize runs dequant_reduce_kernel and
    # either dequant_reduce_quantize_kernel (recompute) or minmax_quantize_kernel (stored)
    fused = dict(must=(FUSED_REDUCE,), must_not=("reduce_chunks_kernel",) + RESIDENT)
    add("mm_fused", "centralized", "synchronous", MINMAX, 3, (F32, BF16), MM_P3_CS, **fused)
    add("mm_fused", "centralized", "synchronous", MINMAX, 16, (F16,), 1536, **fused)
    # :240-241 BAGUA_REDUCE_RECOMPUTE: 0 stores the reduced chunk (dequant_reduce_kernel, then
    # minmax_quantize_kernel), 1 recomputes it (dequant_reduce_quantize_kernel)
    add("mm_fused_stored", "centralized", "synchronous", MINMAX, 3, (F32,), MM_P3_CS,
        env=(("BAGUA_REDUCE_RECOMPUTE", "0"),),
        must=("dequant_reduce_kernel",), must_not=("dequant_reduce_quantize_kernel", "reduce_chunks_kernel"))
    add("mm_fused_recompute", "centralized", "synchronous", MINMAX, 3, (F32,), MM_P3_CS,
        env=(("BAGUA_REDUCE_RECOMPUTE", "1"),),
        must=("dequant_reduce_kernel", "dequant_reduce_quantize_kernel"), must_not=("reduce_chunks_kernel",))
    # :274-278 with fused = false: the reference sequence
    composed = dict(must=("reduce_chunks_kernel", "minmax_dequantize_kernel"), must_not=FUSED_REDUCE + RESIDENT)
    add("mm_unfused", "centralized", "unfused", MINMAX, 4, (F32, F16, BF16), 3072, **composed)
    # centralized_pipelined() :557-622: per piece quantise, reduce, requantise, dequantise
    piped = dict(must=(("minmax_quantize_kernel", 3), ("dequant_reduce_kernel", 3), ("minmax_dequantize_kernel", 3)),
                 must_not=("reduce_chunks_kernel",) + RESIDENT)
    add("mm_pipelined3", "centralized", "pipelined", MINMAX, 4, (F32, F16, BF16), 4104, pieces=3, **piped)
    add("mm_pipelined4_tapered", "centralized", "pipelined", MINMAX, 4, (F32, F16, BF16), 4104, pieces=4,
        env=(("BAGUA_PIPELINE_TAPER", "1"),), **piped)
    # a chunk whose byte size is no multiple of 16: reduce.hip dequant_reduce_impl refuses
    # (S / p is no multiple of the vector), pipeline_fits :398 fails, both land in :274-278
    for entry, pieces in (("synchronous", 0), ("pipelined", 3)):
        add("mm_misaligned", "centralized", entry, MINMAX, 16, (F32,), 4098, pieces=pieces, aligned16=False, **composed)
        add("mm_misaligned", "centralized", entry, MINMAX, 8, (F16,), 4100, pieces=pieces, aligned16=False, **composed)
        # p > 16: minmax_u8.hip reduce_requantize_impl refuses (kMaxFusedChunks), pipeline_fits fails
        add("mm_p17", "centralized", entry, MINMAX, 17, (F32, F16, BF16), 1536, pieces=pieces, **composed)
    add("mm_p33", "centralized", "synchronous", MINMAX, 33, (F32, F16), 1024, **composed)
    # :232 num_elem != num_elem_allocated: no fused middle step, pipeline_fits fails
    tail = dict(must=("reduce_chunks_kernel",), must_not=FUSED_REDUCE + RESIDENT, classes=tuple(TAIL_CLASSES))
    for entry, pieces in (("synchronous", 0), ("pipelined", 3)):
        add("mm_tail", "centralized", entry, MINMAX, 3, (F32, F16), 12288, pieces=pieces, short=4101, **tail)
    add("mm_tail_p17", "centralized", "synchronous", MINMAX, 17, (F32,), 1536, short=5, **tail)

    # ---- centralized, 1-bit ----
    # :263-272 bagua_onebit_reduce_requantize: one of the two fused kernels, nothing stored
    ob_fused = dict(must=(ONEBIT_FUSED,), must_not=("reduce_chunks_kernel",))
    ob_composed = dict(must=("reduce_chunks_kernel", "onebit_decode_kernel"), must_not=ONEBIT_FUSED)
    add("ob_fused", "centralized", "synchronous", ONEBIT, 3, (F32, F16, BF16), 3076, **ob_fused)
    add("ob_unfused", "centralized", "unfused", ONEBIT, 4, (F32, BF16), 2500, **ob_composed)
    # centralized_pipelined_onebit() :666-701: one encode and one decode per piece
    add("ob_pipelined3", "centralized", "pipelined", ONEBIT, 4, (F32, BF16), 3 * 4096, pieces=3,
        must=(("onebit_encode_kernel", 3), ONEBIT_FUSED, ("onebit_decode_kernel", 3)),
        must_not=("reduce_chunks_kernel",))
    # :642 p > 16 is unpieced, onebit.hip ob_reduce_requantize_impl refuses, :274-278
    for entry, pieces in (("synchronous", 0), ("pipelined", 3)):
        add("ob_p17", "centralized", entry, ONEBIT, 17, (F32, F16, BF16), 1536, pieces=pieces, **ob_composed)
    add("ob_p33", "centralized", "synchronous", ONEBIT, 33, (F32,), 1024, **ob_composed)

    # ---- error feedback (two steps, the class on step 1) ----
    # centralized_onebit_ef() :792: the fused _ef middle step; :793-801 from p = 17 decode +
    # reduce + the worker encode on the own chunk (a second onebit_encode_ef_kernel)
    ef = dict(must=("onebit_encode_ef_kernel", "onebit_reduce_encode_ef_kernel"), must_not=("reduce_chunks_kernel",),
              classes=tuple(EF_CLASSES))
    for pieces in (1, 3):
        add(f"ef_pieces{pieces}", "ef", "error_feedback", ONEBIT, 3, (F32, BF16), 3072, pieces=pieces, **ef)
    add("ef_p17", "ef", "error_feedback", ONEBIT, 17, (F16, BF16), 1536,
        must=(("onebit_encode_ef_kernel", 2), "reduce_chunks_kernel"), must_not=("onebit_reduce_encode_ef_kernel",),
        classes=tuple(EF_CLASSES))

    # ---- decentralized ring, MinMaxUInt8 ----
    # decentralized() :1111 mix, :1187 apply; :1163-1198 the reference sequence (binary_kernel)
    ring = dict(must=("ring_mix_kernel", "ring_apply_kernel"), must_not=("binary_kernel",), classes=tuple(RING_CLASSES))
    add("ring_fused", "ring", "synchronous", MINMAX, 4, (F32, F16, BF16), 4099, **ring)
    add("ring_unfused", "ring", "unfused", MINMAX, 4, (F32, BF16), 4099,
        must=("binary_kernel", "minmax_dequantize_kernel"), must_not=RING_FUSED, classes=tuple(RING_CLASSES))
    # :1133-1152 one quantise and one apply per piece
    ring_piped = dict(must=("ring_mix_kernel", ("minmax_quantize_kernel", 3), ("ring_apply_kernel", 3)),
                      must_not=("binary_kernel",), classes=tuple(RING_CLASSES))
    add("ring_pipelined3", "ring", "pipelined", MINMAX, 4, (F32, BF16), 30011, pieces=3, **ring_piped)
    # :1075-1077 multipath from 6 ranks makes the op pipelined at any piece count
    add("ring_multipath", "ring", "pipelined", MINMAX, 6, (F32,), 30011, pieces=3,
        env=(("BAGUA_RING_MULTIPATH", "1"),), **ring_piped)
    return P


PATHS = _paths()
assert len({q.id for q in PATHS}) == len(PATHS)


# ---- inputs and reference of one (path, class) ----------------------------------------------
def inputs(path: Path, cls: str):
    """centralized: (gradients, num_elem or None); ef: the gradients of the two steps (the class
    on the first, benign on the second); ring: build_ring's dict.  The same for every path
    with the same ref_key, whatever its entry point."""
    rng = case_rng(path.ref_key, cls)
    if path.op == "ring":
        return build_ring(cls, path.p, path.size, path.dtype, rng)
    if path.op == "ef":
        return [build(cls, path.p, path.size, path.dtype, rng), build("benign", path.p, path.size, path.dtype, rng)]
    if path.short:
        return build_tail(cls, path.p, path.size, path.dtype, path.short, rng)
    return build(cls, path.p, path.size, path.dtype, rng), None


def reference(backend, path: Path, cls: str, average: int):
    """What the op must leave behind, from the oracle (`backend`: oracle_c or oracle_np).
    centralized: every rank's tensor; ring: (t, w, l, r), each every rank's tensor; ef: per
    step (every rank's tensor, every rank's (wc, ws, sc, ss) after the step)."""
    from oracle import simulate
    data = inputs(path, cls)
    if path.op == "ring":
        with np.errstate(all="ignore"):
            return simulate.decentralized_low_precision(backend, data["t"], data["w"], data["l"], data["r"],
                                                        path.dtype)
    if path.op == "ef":
        import onebit_ef_reference as REF
        states = [REF.OpState(path.p * path.size, path.p) for _ in range(path.p)]
        steps = []
        with np.errstate(all="ignore"):
            for xs in data:
                want, _ = REF.centralized_step(backend, xs, path.dtype, states, bool(average))
                steps.append((want, [(s.wc.copy(), s.ws.copy(), s.sc.copy(), s.ss.copy()) for s in states]))
        return steps
    xs, num_elem = data
    with np.errstate(all="ignore"):
        return simulate.centralized_low_precision(backend, xs, path.dtype, bool(average), method=path.codec,
                                                  num_elem=num_elem)


def compared(path: Path, want) -> list[np.ndarray]:
    """every array of a reference result whose dtype is T (the NaN cap counts these)"""
    if path.op == "ring":
        return [a for tensors in want for a in tensors]
    if path.op == "ef":
        return [a for outs, _ in want for a in outs]
    return list(want)
