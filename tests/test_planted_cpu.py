"""The planted-extremum inputs (tests/planted_cases.py) can fail a wrong kernel:
on every (kind, dtype) of the two-pass shape the two oracles agree on every
byte, every plant decides its chunk's header (restoring that one element to
its base value changes the oracle's header), every region of the pass is
planted in both roles, and the helper refuses a plant that decides nothing.
Runs without a GPU.
"""
import numpy as np
import pytest

import planted_cases as PC
from planted_cases import BF16, F16, F32

DTYPES = [F32, F16, BF16]

EXPECTED_REGIONS = (["head_first", "head_last", "body_vec0_lane0", "body_vec0_lane_last"]
                    + [f"tile0_subtile{k}_first_vec" for k in range(1, 8)]
                    + ["thread63_vec", "thread64_vec", "thread255_vec", "full_tile_last_vec",
                       "tile16_second_iteration", "ragged_tile_first_vec", "ragged_tile_last_vec",
                       "tail_first", "tail_last", "rev_tile16_second_iteration", "rev_below_nt_until",
                       "rev_at_nt_until", "rev_straddling_tile_first_vec", "rev_last_nt_tile_last_vec"])


def chunk_header(oracle_c, x, dtype, p, c, restored=None, base=None):
    """the oracle's header of chunk c alone, optionally with one plant put back"""
    cs = x.size // p
    seg = x[c * cs:(c + 1) * cs].copy()
    if restored is not None:
        seg[restored.index] = base[c * cs + restored.index]
    return PC.header_bits(oracle_c.compress_minmax_u8(seg, dtype, 1), dtype, 1, 0)


def test_geometry_of_the_two_pass_shape():
    """the shape is what the issue states: 16 workgroups per chunk, 17 full tiles, a ragged
    tile of 3 subtiles and 5 vectors, 3 tail elements (chunk 0), heads of differing length"""
    for dtype in DTYPES:
        cs = PC.shape_a_cs(dtype)
        g = PC.two_pass(dtype, cs, 0, PC.SHAPE_A_P)
        assert (g.grid, g.head, g.full_tiles, g.nvec % PC.TILE, g.tail) == (16, 0, 17, 3 * 256 + 5, 3)
        heads = {PC.two_pass(dtype, cs, c, PC.SHAPE_A_P).head for c in range(PC.SHAPE_A_P)}
        assert len(heads) > 8 and cs % 2 == 1
        # workspace cap of bagua_minmax_u8_workspace_bytes does not bind
        assert PC.partials_blocks(cs, dtype, 64, 8 * (PC.K_TARGET_BLOCKS + 64) + 256) == 16
        # a target chunk: one workgroup per tile, no second iteration
        assert PC.two_pass(dtype, cs, 5, 1).grid == 18


@pytest.mark.parametrize("nan", [False, True], ids=["plain", "nan_in_vector"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
@pytest.mark.parametrize("kind", PC.KINDS)
def test_planted_inputs_bite(oracle_c, kind, dtype, nan):
    from oracle import oracle_np as NP
    p, cs = PC.SHAPE_A_P, PC.shape_a_cs(dtype)
    plants = PC.shape_a_plants(dtype, keep_mib=1)
    cover = PC.covered_names(plants)
    for name in EXPECTED_REGIONS:
        assert cover.get(name) == {"min", "max"}, f"region {name} is not planted in both roles: {cover.get(name)}"
    x, base = PC.build(dtype, kind, p, cs, plants, seed=dtype * 7 + len(kind), nan=nan,
                       vector_origin=PC.shape_a_origin(dtype))  # the self-check runs inside
    if nan:
        assert np.isnan(NP.to_f32(x, dtype)).sum() >= len(plants)
    want = oracle_c.compress_minmax_u8(x, dtype, p)
    assert np.array_equal(want, NP.compress_minmax_u8(x, dtype, p)), "the two oracles disagree"
    for pl in plants:
        with_plant = PC.header_bits(want, dtype, p, pl.chunk)
        without = chunk_header(oracle_c, x, dtype, p, pl.chunk, restored=pl, base=base)
        i = 0 if pl.role == "min" else 1
        assert without[i] != with_plant[i], f"restoring {pl} leaves the header at {with_plant}"
        assert with_plant[i] == PC.plant_bits(dtype, kind, pl.role), f"{pl}: header {with_plant}"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
def test_signed_zero_header_bits(oracle_c, dtype):
    """-0 as the only minimum below +0 is the header's minimum, bit for bit; +0 above -0 the maximum"""
    cs = 4099
    x, _ = PC.build(dtype, "signed_zero", 1, cs, [PC.Plant(0, 17, "min", "a"), PC.Plant(0, 4000, "max", "b")])
    assert PC.header_bits(oracle_c.compress_minmax_u8(x, dtype, 1), dtype, 1, 0)[0] == PC.neg_zero_bits(dtype)
    x, _ = PC.build(dtype, "signed_zero_mirror", 1, cs, [PC.Plant(0, 17, "min", "a"), PC.Plant(0, 4000, "max", "b")])
    assert PC.header_bits(oracle_c.compress_minmax_u8(x, dtype, 1), dtype, 1, 0)[1] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PC.DTYPE_NAME[d])
def test_negative_plants_stay_out_of_the_header(oracle_c, dtype):
    """partially valid bucket: the last valid element is planted, the first invalid one
    and the last element of an empty chunk hold +-INIT_MAX/2 and leave every header alone"""
    from oracle import oracle_np as NP
    p, cs = 4, PC.shape_a_cs(dtype)
    n_in = 2 * cs + cs // 3
    g = PC.two_pass(dtype, cs, 2, p, num_elem=n_in)
    plants = [PC.Plant(2, g.valid - 1, "max", "last_valid"), PC.Plant(2, g.elem(g.nvec // 2), "min", "body")]
    x, base = PC.build(dtype, "margin", p, cs, plants, num_elem=n_in)
    clean = oracle_c.compress_minmax_u8(x, dtype, p, num_elem=n_in)
    PC.plant_negative(x, dtype, n_in, n_in, negative=False)
    PC.plant_negative(x, dtype, p * cs - 1, n_in, negative=True)
    want = oracle_c.compress_minmax_u8(x, dtype, p, num_elem=n_in)
    assert np.array_equal(want, NP.compress_minmax_u8(x, dtype, p, num_elem=n_in))
    for c in range(p):
        assert PC.header_bits(want, dtype, p, c) == PC.header_bits(clean, dtype, p, c)
    assert PC.header_bits(want, dtype, p, 2) == (PC.t_bits(-1.0, dtype), PC.t_bits(1.0, dtype))


def test_helper_refuses_vacuous_plants():
    cs = 1000
    with pytest.raises(ValueError, match="outside"):
        PC.build(F32, "margin", 2, cs, [PC.Plant(1, cs, "max", "past_the_chunk")])
    with pytest.raises(ValueError, match="outside"):  # past input_num_element
        PC.build(F32, "margin", 2, cs, [PC.Plant(1, 10, "max", "invalid")], num_elem=cs + 10)
    with pytest.raises(ValueError, match="one element"):
        PC.build(F32, "margin", 1, cs, [PC.Plant(0, 3, "max", "a"), PC.Plant(0, 3, "min", "b")])
    # two maxima of the same value: neither decides the header alone
    with pytest.raises(ValueError, match="does not decide"):
        PC.build(F16, "ulp", 1, cs, [PC.Plant(0, 3, "max", "a"), PC.Plant(0, 900, "max", "b")])
    x = PC.base_data(F32, "margin", 2 * cs, 0)
    with pytest.raises(ValueError, match="valid prefix"):
        PC.plant_negative(x, F32, cs - 1, cs, negative=False)
    # the ulp plants are the neighbouring T values
    for dtype in (F32, F16, BF16):
        b = PC.t_bits(0.37, dtype)
        assert PC.plant_bits(dtype, "ulp", "max") == b + 1 and PC.plant_bits(dtype, "ulp", "min") == b - 1
