"""The reference is sound on the hostile op inputs (tests/op_edge_cases.py), without a GPU.

For every distinct reference of the path table (op, codec, p, dtype, size, tail), every class
and both modes: the C oracle and the numpy oracle agree byte for byte; at most half of the
compared values are NaN (a NaN result compares equal to any NaN, so it must never cover a
chunk that could be wrong); every class does to the reference result what its name says; and
every path has the host-derivable properties its row of the table claims.
"""
import numpy as np
import pytest

import op_edge_cases as E
from op_edge_cases import F16, F32, MINMAX, ONEBIT
from oracle import oracle_np as NP

KEYS = {}
for _q in E.PATHS:
    KEYS.setdefault(_q.ref_key, _q)
REFS = list(KEYS.values())
MODES = {"centralized": (1, 0), "ef": (1, 0), "ring": (1,)}  # the ring op has no mode


def _bytes_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(path, a, b):
    if path.op == "ef":
        return all(_bytes_equal(x, y) for (oa, sa), (ob, sb) in zip(a, b)
                   for x, y in list(zip(oa, ob)) + [(u, v) for ra, rb in zip(sa, sb) for u, v in zip(ra, rb)])
    return all(_bytes_equal(x, y) for x, y in zip(E.compared(path, a), E.compared(path, b)))


def _chunk_mask(path, chunks):
    m = np.zeros(path.p * path.size, bool)
    for c in chunks:
        m[c * path.size:(c + 1) * path.size] = True
    return m


def _check_class(path, cls, average, want):
    """what the class's name promises, read off the reference result"""
    what = f"{path.id} {cls} average={average}"
    dt = path.dtype
    if path.op == "ring":
        nan = [np.stack([E.is_nan(a, dt) for a in tensors]) for tensors in want]  # [tensor][rank, element]
        clean = [r for r in range(path.p) if not any(t[r].any() for t in nan)]
        assert clean, f"{what}: no rank is NaN-free"
        if cls in ("benign", "constant", "zero", "neg_zero", "denormal"):
            assert len(clean) == path.p, f"{what}: must be NaN-free"
        if cls in ("pos_inf", "neg_inf") or (cls == "huge" and dt != F16):
            # an infinite value (or a range that overflows: +-60000 does not) makes rank
            # p - 1's payload non-finite: it reaches both ring neighbours and nobody else
            hit = {r for r in range(path.p) if not all(E.is_finite(t[r], dt).all() for t in want)}
            assert hit == {path.p - 2, path.p - 1, 0}, f"{what}: non-finite on ranks {sorted(hit)}"
        if cls in ("one_nan", "w_nan"):
            # min/max skips a NaN and it quantises to the top level, so the payload carries
            # none: the NaN stays in the tensors of rank p - 1 that are rebuilt from the weight
            nans = sum(int(t.sum()) for t in nan)
            assert (nans == 0) if cls == "one_nan" else (0 < nans <= 4), f"{what}: {nans} NaN"
        return
    outs = E.compared(path, want)
    nan = np.stack([E.is_nan(a, dt) for a in outs])
    if path.short:
        assert not nan.any(), f"{what}: a value past num_elem reached a header"
        assert all(E.is_finite(a, dt).all() for a in outs), what
        return
    planted = _chunk_mask(path, E.planted_chunks(path.p))
    assert not nan[:, ~planted].any(), f"{what}: NaN outside the planted chunks"
    if cls in ("benign", "zero", "neg_zero", "constant", "all_ranks_constant", "denormal"):
        assert not nan.any(), f"{what}: must be NaN-free"
    if cls == "all_nan_chunk" or (cls == "one_nan" and path.codec == ONEBIT):
        assert nan[:, planted].all(), f"{what}: the planted chunks must be NaN on every rank"
    if cls == "one_nan" and path.codec == MINMAX:
        # the reference's min/max skips a NaN and its quantiser maps it to the top level:
        # a single NaN never reaches a header, and decodes to the chunk's maximum
        assert not nan.any(), f"{what}: one NaN must not spread under MinMax"
    if cls == "huge" and dt == F16 and average == 0 and path.codec == MINMAX:
        # (the 1-bit codec sends +-mean|x|, about 2 * 60000 / cs: nothing to overflow)
        bad = np.stack([~E.is_finite(a, dt) for a in outs])
        assert bad[:, planted].any(), f"{what}: the f16 sum must overflow"


@pytest.mark.parametrize("path", REFS, ids=lambda q: "-".join(str(k) for k in q.ref_key))
def test_reference_is_sound(oracle_c, path):
    for cls in path.classes:
        for average in MODES[path.op]:
            what = f"{path.id} {cls} average={average}"
            want = E.reference(oracle_c, path, cls, average)
            assert _same(path, want, E.reference(NP, path, cls, average)), f"{what}: the two oracles disagree"
            outs = E.compared(path, want)
            nans = sum(int(E.is_nan(a, path.dtype).sum()) for a in outs)
            assert 2 * nans <= sum(a.size for a in outs), f"{what}: more than half of the reference is NaN"
            _check_class(path, cls, average, want)


def test_hostile_classes_change_the_reference(oracle_c):
    """a class whose plant an edit of the builder lost would equal `benign`: every class
    changes the planted chunks' result on one small path of each codec"""
    for name in ("mm_fused", "ob_fused"):
        path = next(q for q in E.PATHS if q.name == name and q.dtype == F32)
        base = E.reference(oracle_c, path, "benign", 1)
        for cls in path.classes[1:]:
            got = E.reference(oracle_c, path, cls, 1)
            assert not all(_bytes_equal(a, b) for a, b in zip(got, base)), f"{path.id} {cls}"


@pytest.mark.parametrize("path", E.PATHS, ids=lambda q: q.id)
def test_path_properties(path):
    p, dt, es = path.p, path.dtype, NP.esize(path.dtype)
    if path.op == "ring":
        assert path.size % 8, "the ring shapes end in a partial vector"
        assert path.pieces == 0 or path.size > 3 * 512, "more than one piece"
        assert ("BAGUA_RING_MULTIPATH", "1") not in path.env or p >= 6
        return
    cs = path.size
    if path.codec == MINMAX:
        S = NP.minmax_compressed_size(p, cs, dt)
    else:
        S = NP.onebit_compressed_size(p, cs)
    assert S % p == 0, "the alltoall needs S % p == 0"
    vec = 4 if dt == F32 else 8
    if path.codec == MINMAX:
        assert ((cs * es) % 16 == 0) == path.aligned16
        # the fused middle step and the pipelined schedule need S / p on a vector boundary
        # (reduce.hip dequant_reduce_impl, comm_ops.cpp pipeline_fits)
        assert ((S // p) % vec == 0) == path.aligned16
    assert (p > 16) == (path.name.rsplit("_", 1)[-1] in ("p17", "p33"))
    assert cs > 1024 or p == 33, "a full tile and a partial or second one"
    if path.entry == "pipelined":
        assert path.pieces >= 3 and cs > (path.pieces - 1) * 512, "more than one non-empty piece"
    if path.short:
        # the tail lies inside the last chunk (a chunk with no valid element decodes to NaN in
        # f32, which the NaN-free assertion above excludes), ends off a vector boundary and,
        # at p = 3, covers more than a 4096-element stretch of it
        assert 0 < path.short < cs and (p * cs - path.short) % vec
        assert path.short > 4096 or p == 17
    assert set(path.classes) <= set(E.CLASSES + E.TAIL_CLASSES)


def test_the_issue_shape_the_reference_refuses():
    """MinMax at p = 3 with cs = 3076: S % p != 0, so there is no reference result (simulate
    asserts, the op returns INVALID_ARG); the p = 3 MinMax rows use MM_P3_CS instead"""
    p, cs = E.REFUSED_MINMAX_SHAPE
    assert NP.minmax_compressed_size(p, cs, F32) % p and NP.minmax_compressed_size(p, cs, F16) % p
    assert NP.minmax_compressed_size(p, E.MM_P3_CS, F32) % p == 0 and E.MM_P3_CS % 1024
