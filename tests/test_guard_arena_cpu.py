"""The guard-band harness (tests/guard_arena.py) on a CPU arena: planted stray writes are reported with
the right buffer, side and distance, writes inside writable buffers are not, `place` gives every phase
the kernel ABI documents; and the GPU test's table (tests/test_gpu_guard_bands.py) has a row for every
MX entry that include/bagua_kernels.h declares."""
import os
import re

import numpy as np
import pytest

from guard_arena import GUARD, POISONS, Arena, GuardError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arena(poison):
    a = Arena(poison, "cpu", capacity=1 << 20)
    x = a.place("input", 1001, 4, 4, readonly=True).write(np.arange(1001, dtype=np.uint8))
    out = a.place("output", 96, 16, 16).write(np.full(96, 0xAB, np.uint8))
    res = a.place("residual", 4 * 33, 4, 20).write(np.zeros(33, np.float32))
    return a, x, out, res


@pytest.mark.parametrize("poison", POISONS)
def test_planted_stray_writes_are_reported(poison):
    a, x, out, res = arena(poison)
    a.check("untouched")
    out.bytes[:] = 0           # writes inside the writable buffers: their first and last bytes included
    res.bytes[-1] = 0x55
    res.bytes[0] = 0x55
    a.check("writes inside the writable buffers")
    assert out.read()[-1] == 0 and res.read(np.float32).size == 33
    for off, report in ((out.off - 1, "1 bytes before the buffer 'output' (96 bytes)"),
                        (out.off + out.nbytes, "1 bytes after the buffer 'output' (96 bytes)"),
                        (x.off + x.nbytes, "1 bytes after the buffer 'input' (1001 bytes)"),
                        (x.off - GUARD, f"{GUARD} bytes before the buffer 'input'"),          # the far edges of bands
                        (res.off + res.nbytes + GUARD - 1, f"{GUARD} bytes after the buffer 'residual'"),
                        (a.capacity - 1, f"{a.capacity - res.off - res.nbytes} bytes after the buffer 'residual'"),
                        (x.off + 517, "inside the read-only buffer 'input', 517 bytes from its start")):
        old = int(a.mem[off])
        a.mem[off] = old ^ 0x5A
        with pytest.raises(GuardError) as e:
            a.check("planted")
        assert report in str(e.value) and f"[{poison}]" in str(e.value) and str(off) in str(e.value), str(e.value)
        a.mem[off] = old
        a.check("restored")
    # a whole stray 16-B vector behind the output: the count and the first byte
    a.mem[out.off + out.nbytes:out.off + out.nbytes + 16] = 0
    with pytest.raises(GuardError, match="16 bytes changed, the first 1 bytes after the buffer 'output'"):
        a.check("vector")


def test_poisons():
    a = Arena("hash", "cpu", capacity=1 << 18)
    m = a.mem.numpy()
    assert m.min() == 1 and m.max() == 254 and m[0] == 14 and m[1000] == 1 + (167 * 1000 + 13) % 254
    assert (Arena("ones", "cpu", capacity=1 << 18).mem.numpy() == 0xFF).all()
    with pytest.raises(ValueError):
        Arena("zeros")


@pytest.mark.parametrize("align", [2, 4, 8, 16])
def test_place_gives_the_requested_phase(align):
    """2: a 16-bit tensor one element off a vector; 4: a residual, MXFP4's decode input; 8: the other
    decode inputs; 16: every encode output and the vector path"""
    a = Arena("ones", "cpu", capacity=4 << 20)
    end = 0
    for phase in [k * align for k in (0, 1, 3, 5, 256 // align - 1)]:
        b = a.place(f"phase {phase}", 1000 + phase, align, phase)
        assert b.ptr % 256 == phase and b.ptr == a.mem.data_ptr() + b.off
        assert GUARD <= b.off - end < GUARD + 256 and b.bytes.numel() == 1000 + phase
        end = b.off + b.nbytes
    empty = a.place("empty", 0, align, align)
    assert empty.ptr % 256 == align and empty.read().size == 0
    a.check("placed, nothing written")
    with pytest.raises(AssertionError):
        a.place("off its alignment", 8, align, align + 1)
    with pytest.raises(AssertionError, match="full"):
        a.place("too large", 4 << 20, align, 0)


# ------------------------------------------------------------ header coverage ----
# entries that take no device pointer, by name: nothing of theirs could be placed in an arena
HOST_ONLY = {
    r"_compressed_bytes$": "size arithmetic on the host",
    r"_piece_range$": "the piece schedule: host arithmetic, two host out-pointers",
    r"_ef_state_bytes$": "size arithmetic on the host, two host out-pointers",
}


def test_every_mx_entry_of_the_header_has_a_row():
    import test_gpu_guard_bands as G
    text = open(os.path.join(ROOT, "include", "bagua_kernels.h")).read()
    declared = set(re.findall(r"\b(bagua_mxfp[468]_\w+|bagua_ring_\w+_mxfp[468])\s*\(", text))
    assert len(declared) >= 52, sorted(declared)
    need = {n for n in declared if not any(re.search(pat, n) for pat in HOST_ONLY)}
    rows = {row.entry for row in G.TABLE}
    assert not need - rows, f"no guard-band row for {sorted(need - rows)}"
    assert not rows - declared, f"rows for names the header does not declare: {sorted(rows - declared)}"
    # every row is run: each names the test function that drives it, and that function takes it from the table
    for row in G.TABLE:
        assert callable(getattr(G, row.test)) and row.test.startswith("test_"), row
