"""Guard-band arena: every buffer of a kernel call between poisoned bands.  TEST INFRASTRUCTURE ONLY.

One arena is a single uint8 tensor, poison all over.  `place` carves the call's buffers out of it with a
band of at least GUARD bytes before the first, between neighbours and after the last, each buffer starting
at the requested phase of 256 B and ending exactly nbytes later: its last byte is followed by poison.
`check` compares everything outside the buffers, and every read-only buffer, with what was put there and
names the nearest buffer, the side and the distance of the first byte that changed.

Two poisons.  "hash": byte i of the arena is 1 + (167 i + 13) mod 254, never 0x00 and never 0xFF, so that
neither a stray zeroed slack word nor a stray NaN scale byte can match it.  "ones": every byte 0xFF, a NaN
in f32, f16 and bf16 and the NaN scale byte, so that a read past a buffer that reaches an amax, a sum or a
decode shows in the output.  Works on CPU tensors as well (tests/test_guard_arena_cpu.py)."""
import numpy as np
import torch

GUARD = 64 * 1024  # a workgroup tile of f32 is 32 KiB: a whole stray tile still lands in a band
PHASE = 256
POISONS = ("hash", "ones")
_cache = {}


def poison_bytes(poison, nbytes, device):
    """the first nbytes of the poison pattern on `device` (kept: an arena is filled by one copy)"""
    key = (poison, str(device))
    if key not in _cache or _cache[key].numel() < nbytes:
        if poison == "hash":
            i = torch.arange(nbytes, dtype=torch.int64, device=device)
            _cache[key] = ((167 * i + 13) % 254 + 1).to(torch.uint8)
        elif poison == "ones":
            _cache[key] = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
        else:
            raise ValueError(f"unknown poison {poison!r}")
    return _cache[key][:nbytes]


class Buffer:
    """one placed buffer: bytes [off, off + nbytes) of the arena"""

    def __init__(self, arena, name, off, nbytes, readonly):
        self.arena, self.name, self.off, self.nbytes, self.readonly = arena, name, off, nbytes, readonly
        self.initial = None

    @property
    def ptr(self):
        return self.arena.mem.data_ptr() + self.off

    @property
    def bytes(self):
        """the buffer as a uint8 view of the arena"""
        return self.arena.mem[self.off:self.off + self.nbytes]

    def write(self, data):
        """fill the buffer with the bytes of a numpy array of exactly its size"""
        raw = np.ascontiguousarray(data).view(np.uint8).ravel()
        assert raw.size == self.nbytes, f"{self.name}: {raw.size} bytes for a buffer of {self.nbytes}"
        self.initial = torch.from_numpy(raw.copy()).to(self.arena.mem.device)
        self.bytes.copy_(self.initial)
        return self

    def read(self, dtype=np.uint8):
        """the buffer's bytes on the host, viewed as `dtype`"""
        return self.bytes.cpu().numpy().view(dtype)


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, poison, device="cpu", capacity=4 << 20):
        self.poison, self.capacity = poison, capacity
        self.mem = torch.empty(capacity, dtype=torch.uint8, device=device)
        self.mem.copy_(poison_bytes(poison, capacity, device))
        self.buffers = []

    def place(self, name, nbytes, align, phase=0, readonly=False):
        """a buffer of exactly nbytes with data_ptr % 256 == phase, phase a multiple of `align` (the minimum
        alignment the entry documents), a band of at least GUARD bytes after whatever was placed before"""
        assert 0 <= phase < PHASE and phase % align == 0 and PHASE % align == 0, (name, align, phase)
        off = (self.buffers[-1].off + self.buffers[-1].nbytes if self.buffers else 0) + GUARD
        off += (phase - (self.mem.data_ptr() + off)) % PHASE
        assert off + nbytes + GUARD <= self.capacity, f"{name}: the arena of {self.capacity} bytes is full"
        buf = Buffer(self, name, off, nbytes, readonly)
        self.buffers.append(buf)
        return buf

    def _report(self, lo, got, want):
        """the first differing byte of arena bytes [lo, lo + got.numel()): nearest buffer, side, distance"""
        bad = torch.nonzero(got != want).ravel()
        at = lo + int(bad[0])
        for b in self.buffers:
            if b.off <= at < b.off + b.nbytes:
                where = f"inside the read-only buffer {b.name!r}, {at - b.off} bytes from its start"
                break
        else:
            sides = [(b.off - at, "before", b) for b in self.buffers if at < b.off]
            sides += [(at - (b.off + b.nbytes) + 1, "after", b) for b in self.buffers if at >= b.off + b.nbytes]
            dist, side, b = min(sides, key=lambda s: s[0])
            where = f"{dist} bytes {side} the buffer {b.name!r} ({b.nbytes} bytes)"
        k = bad[:8].cpu()
        g, w = got.cpu()[k].tolist(), want.cpu()[k].tolist()
        return (f"{int(bad.numel())} bytes changed, the first {where}; arena offsets {[lo + int(i) for i in k]}: "
                f"{[hex(v) for v in g]} where {[hex(v) for v in w]} was put")

    def check(self, what=""):
        """every band against the poison and every read-only buffer against what was written into it"""
        pattern = poison_bytes(self.poison, self.capacity, self.mem.device)
        errors, lo = [], 0
        for b in self.buffers + [None]:
            hi = self.capacity if b is None else b.off
            if not torch.equal(self.mem[lo:hi], pattern[lo:hi]):
                errors.append(self._report(lo, self.mem[lo:hi], pattern[lo:hi]))
            if b is not None:
                if b.readonly and b.nbytes and not torch.equal(b.bytes, b.initial):
                    errors.append(self._report(b.off, b.bytes, b.initial))
                lo = b.off + b.nbytes
        if errors:
            raise GuardError(f"{what}: [{self.poison}] " + "; ".join(errors))
