"""GPU parity of the double-buffered streamed loops of the one-launch MinMax-UInt8 encode
(minmax_resident.hip) at small size, for the stream-last and the stack order.

The streamed part of a slice is read in tiles of SB rows, two tiles in flight: pass 1
ascending, pass 2 descending (stream-last: the two top tiles requested before the exchange;
stack: descending, or ascending on the rows with ASC).  With two or more full tiles those loops
alternate between their two buffers, prefetch a clamped tile at an odd count's tail, and end in a
ragged top tile.  The shapes below cross each of those edges with slices of on_chip + k rows
(on_chip = R + H + RL), derived from the row's geometry and the CU count as in
test_gpu_resident_window.py (which holds the same table for the window rows); p = 1 and a
96-element scalar head.  Every case asserts that the one-launch path is taken (gpu_compress) and
compares every byte of the compressed buffer with the C oracle.

  rows: 30 (stream-last; f32, bf16), 0 (BLOCK = 256, no non-temporal loads), 3 (nothing on chip),
        24 (stack, first tile before the ticket, ascending re-read), 29 (f16; stack, descending),
        18 (bf16; stack)
"""
import pytest

from test_gpu_codec import BF16, F16, F32
from test_gpu_resident import K, env, small_threshold  # noqa: F401  (fixtures)
from test_gpu_resident_window import HEAD, check, elements, geometry, row, shared_input  # noqa: F401

pytestmark = pytest.mark.gpu


def tile_rows(name, on_chip, sb, block):
    """(rows per slice, vectors the last slice is short) of the named streamed-tile case."""
    return {
        "ragged_top_only": (on_chip + 3, 40),
        "two_full_tiles": (on_chip + 2 * sb, 0),
        "two_tiles_and_one_vector": (on_chip + 2 * sb + 1, block - 1),
        "three_tiles_and_three_rows": (on_chip + 3 * sb + 3, 40),
        "four_tiles_less_one_vector": (on_chip + 4 * sb, 1),
    }[name]


TILE_CASES = ["ragged_top_only", "two_full_tiles", "two_tiles_and_one_vector", "three_tiles_and_three_rows",
              "four_tiles_less_one_vector"]
ROWS = [(30, F32), (30, BF16), (0, F32), (3, F32), (24, F32), (29, F16), (18, BF16)]


@pytest.mark.parametrize("case", TILE_CASES)
@pytest.mark.parametrize("cfg,dtype", ROWS)
def test_streamed_tile_counts(K, oracle_c, monkeypatch, row, cfg, dtype, case):
    block, r, h, rl, sb, order = geometry(K, cfg)
    assert order in (0, 1) and rl == 0
    rows, short = tile_rows(case, r + h + rl, sb, block)
    n = HEAD + elements(K, cfg, dtype, rows, short)
    # a row with nothing on chip streams whole slices below the suite's size threshold
    monkeypatch.setenv("BAGUA_RESIDENT_MIN_ELEMS", str(min(n, 1 << 22)))
    check(K, oracle_c, shared_input(n, dtype, seed=11), dtype, 1)
