"""Guarded device buffers for the C ABI's memory contract (tests/test_gpu_abi_memory.py).

The caching allocator rounds every size up, packs small tensors into shared segments and aligns to 256 bytes or more, so a kernel
that writes a few bytes past a buffer, reads a region it never wrote, or needs more alignment than include/leaf_hip.h promises
goes unnoticed on ordinary tensors.  ``guarded(nbytes, fill, offset)`` lays ONE allocation out as

    [ front guard | payload: exactly nbytes | back guard: 4096 bytes ]

with the payload starting ``offset`` bytes past a 4096-byte boundary (the front guard is the 4096 + offset bytes before it), both
guards holding a fixed position-dependent byte pattern and the payload pre-filled.  Plain module, no product logic, no fixtures."""
import ctypes

import torch

GUARD = 4096
DEV = "cuda:0"
_PERIOD = 251                                   # prime: the pattern never lines up with a power-of-two stride


def _pattern(n, phase, device):
    return ((torch.arange(n, device=device, dtype=torch.int32) + phase) % _PERIOD + 2).to(torch.uint8)    # never 0x00 / 0xFF


class Guarded:
    def __init__(self, nbytes, fill, offset=0, capacity=None, device=DEV):
        assert nbytes >= 0 and 0 <= offset < GUARD
        self.capacity = max(nbytes, capacity or 0)
        self.offset = offset
        self.raw = torch.empty(GUARD + GUARD + offset + self.capacity + GUARD, dtype=torch.uint8, device=device)
        self.lead = (-self.raw.data_ptr()) % GUARD                       # bytes before the first 4096-byte boundary
        self.start = self.lead + GUARD + offset                          # payload offset inside raw
        self.raw[self.lead:self.start] = _pattern(GUARD + offset, 0, device)
        self.nbytes = None
        self.relayout(nbytes)
        self.fill(fill)
        assert (self.address - offset) % GUARD == 0

    # ---- layout
    def relayout(self, nbytes):
        """Move the back guard so that the payload is exactly ``nbytes`` long; the payload keeps the bytes it has (what an earlier
        call through a longer payload left there)."""
        assert 0 <= nbytes <= self.capacity
        self.nbytes = nbytes
        end = self.start + nbytes
        self.raw[end:end + GUARD] = _pattern(GUARD, 7, self.raw.device)
        return self

    def fill(self, fill):
        """``fill``: a byte value, or a tensor whose bytes are copied in (it must have exactly nbytes)."""
        pay = self.bytes()
        if isinstance(fill, int):
            pay.fill_(fill)
        else:
            src = fill.detach().contiguous().reshape(-1).view(torch.uint8)
            assert src.numel() == self.nbytes, (src.numel(), self.nbytes)
            pay.copy_(src)
        return self

    # ---- access
    @property
    def address(self):
        return self.raw.data_ptr() + self.start

    @property
    def ptr(self):
        return ctypes.c_void_p(self.address)

    def bytes(self):
        return self.raw[self.start:self.start + self.nbytes]

    def view(self, dtype, shape=None):
        """Typed view of the payload.  torch refuses views below the element alignment, so a payload at an odd offset comes back
        as a copy (read-only use)."""
        b = self.bytes()
        item = torch.empty(0, dtype=dtype).element_size()
        t = b.view(dtype) if self.address % item == 0 and b.storage_offset() % item == 0 else b.clone().view(dtype)
        return t if shape is None else t.reshape(shape)

    def cpu(self, dtype, shape=None):
        t = self.bytes().cpu().clone().view(dtype)
        return t if shape is None else t.reshape(shape)

    # ---- checks
    def check(self, what=""):
        dev = self.raw.device
        front = self.raw[self.lead:self.start]
        end = self.start + self.nbytes
        back = self.raw[end:end + GUARD]
        for name, got, want, base in (("front", front, _pattern(GUARD + self.offset, 0, dev), -(GUARD + self.offset)),
                                      ("back", back, _pattern(GUARD, 7, dev), self.nbytes)):
            bad = (got != want).nonzero()
            if bad.numel():
                first = int(bad[0])
                raise AssertionError(f"{what}: {name} guard changed; first changed byte at payload offset {base + first} "
                                     f"(payload is {self.nbytes} bytes), {int(bad.numel())} bytes changed")


def guarded(nbytes, fill, offset=0, capacity=None):
    return Guarded(nbytes, fill, offset, capacity)


def guarded_tensor(t, offset=0):
    """A read-only input: the tensor's bytes in a guarded payload, plus the copy ``unchanged`` compares against after the call."""
    t = t.detach().contiguous()
    g = Guarded(t.numel() * t.element_size(), t, offset)
    g.before = g.bytes().clone()
    return g


def unchanged(g, what=""):
    g.check(what)
    assert torch.equal(g.bytes(), g.before), f"{what}: a read-only input was modified"
