"""Guarded buffers: what a kernel writes OUTSIDE the memory the ABI sizes (tests/test_gpu_write_extent.py,
CPU tier tests/test_guards_cpu.py).

A Guarded is one uint8 backing tensor [front pad | interior | back pad].  The pads hold the guard byte
0xCB (non-zero: a stray zero fill is the commonest wrong write), the interior a fill byte the test
chooses.  Running an operation with interior fills 0x00 and 0xFF and comparing the results also shows
reads of scratch nobody initialised: fresh allocator memory is usually zero, 0xFF words are NaN / -1.

GuardedBuffers puts every scratch request and forward output of the rasterizer bindings into a
Guarded of exactly the requested size (it is a _native.static_buffers); guarded_allocations does the
same for the bindings that call torch.empty / zeros / empty_like / zeros_like themselves, by giving
their module a proxy of torch for the length of a block.  No product code knows of either.
"""
import contextlib
import math

import torch

from langsplat_amd import _native

GUARD = 0xCB
MIN_PAD = 64 * 1024
ALIGN = 256  # what torch's allocators (and lsr_alloc_fn's contract) align to


class GuardError(AssertionError):
    pass


def default_pad(nbytes):
    """Pad bytes on each side: a stray store near an end of the interior lands in memory the test owns."""
    return max(MIN_PAD, nbytes // 4)


class Guarded:
    def __init__(self, shape, dtype, device, front=None, back=None, fill=0x00, misalign=0, name=None):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        self.shape, self.dtype, self.fill, self.name = shape, dtype, int(fill), name
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = math.prod(shape) * self.itemsize
        front = default_pad(self.nbytes) if front is None else int(front)
        back = default_pad(self.nbytes) if back is None else int(back)
        if misalign % self.itemsize:
            raise ValueError("Guarded: misalign must be a multiple of the element size")
        self.backing = torch.empty((front + ALIGN + misalign + self.nbytes + back,), dtype=torch.uint8, device=device)
        self.backing.fill_(GUARD)
        base = self.backing.data_ptr()
        self.start = front + (-(base + front)) % ALIGN + misalign
        self.end = self.start + self.nbytes
        self.bytes = self.backing[self.start:self.end]
        self.bytes.fill_(self.fill)
        self.tensor = self.bytes.view(dtype).view(shape)
        assert (self.tensor.data_ptr() - misalign) % ALIGN == 0
        assert self.start >= front and self.backing.numel() - self.end >= back

    @property
    def back_pad(self):
        return self.backing.numel() - self.end

    def refill(self, fill=None):
        """The interior back to its fill byte (or to a new one); the pads are left as they are."""
        if fill is not None:
            self.fill = int(fill)
        self.bytes.fill_(self.fill)

    def check(self, name=None):
        """Both pads still hold the guard byte, else GuardError naming the buffer and the offset of the
        first changed byte: `start-k` is k bytes before the interior, `end+k` k bytes past its last."""
        name = name if name is not None else (self.name or "buffer")
        for pad, origin in ((self.backing[:self.start], "start"), (self.backing[self.end:], "end")):
            bad = torch.nonzero(pad != GUARD)
            if bad.numel():
                i = int(bad[0, 0])
                off = f"start-{self.start - i}" if origin == "start" else f"end+{i}"
                raise GuardError(f"{name}: {bad.shape[0]} guard byte(s) changed, the first at {off} "
                                 f"(interior of {self.nbytes} bytes, value {int(pad[i]):#04x})")

    def unwritten(self):
        """Interior elements whose every byte still holds the fill byte."""
        if self.nbytes == 0:
            return 0
        return int((self.bytes.view(-1, self.itemsize) == self.fill).all(dim=1).sum())

    def assert_only_written(self, views, name=None):
        """Every interior byte outside `views` (tensors that are views of the interior) still holds the
        fill byte: the alignment gaps between sub-tensors carved out of one allocation are guards too."""
        name = name if name is not None else (self.name or "buffer")
        keep = torch.ones((self.nbytes,), dtype=torch.bool, device=self.backing.device)
        p0 = self.tensor.data_ptr()
        for v in views:
            if v is None or v.numel() == 0:
                continue
            o = v.data_ptr() - p0
            n = v.numel() * v.element_size()
            assert 0 <= o and o + n <= self.nbytes and v.is_contiguous(), f"{name}: not a view of the interior"
            keep[o:o + n] = False
        bad = torch.nonzero(keep & (self.bytes != self.fill))
        if bad.numel():
            raise GuardError(f"{name}: {bad.shape[0]} byte(s) between the views changed, the first at byte "
                             f"{int(bad[0, 0])} of the interior")


class GuardedBuffers(_native.static_buffers):
    """A static_buffers set whose every tensor is a Guarded of exactly the requested size.  `fill`: the
    interior byte of new buffers; `extra_back`: {key: bytes} added to a buffer's back pad (capacity
    mode: the difference to the full-size buffer, so even an unchecked write of the whole view lands in
    owned memory).  A request of another size checks the buffer it replaces first; replaced buffers
    stay allocated until the set goes, so nothing that still points at one can reach freed memory."""

    def __init__(self, fill=0x00, extra_back=None):
        super().__init__()
        self.fill = int(fill)
        self.extra_back = dict(extra_back or {})
        self.guards = {}
        self.requests = []  # (key, bytes) of every request, in order
        self.retired = []

    def tensor(self, key, shape, dtype, device, at_least=False):
        shape = tuple(int(s) for s in shape)
        g = self.guards.get(key)
        self.requests.append((key, math.prod(shape) * torch.empty((), dtype=dtype).element_size()))
        if g is None or g.shape != shape or g.dtype != dtype or g.backing.device != torch.device(device):
            if g is not None:
                g.check(f"{key} (before it was replaced)")
                self.retired.append(g)
            nbytes = self.requests[-1][1]
            g = Guarded(shape, dtype, device, back=default_pad(nbytes) + int(self.extra_back.get(key, 0)),
                        fill=self.fill, name=str(key))
            self.guards[key] = g
            self.tensors[key] = g.tensor
        return g.tensor

    def requested(self, key):
        """Bytes of the last request for `key` (None: never requested)."""
        for k, n in reversed(self.requests):
            if k == key:
                return n
        return None

    def check_all(self):
        for key, g in self.guards.items():
            g.check(str(key))
        for g in self.retired:
            g.check(f"{g.name} (replaced)")

    def assert_abi_sizes(self, P, W, H, num_rendered=0, entries=0):
        """Whatever scratch the calls over (P, W, H) requested is what include/lsr.h says: geometry and
        image exactly lsr_geom_bytes / lsr_image_bytes, the backward's exactly lsr_backward_bytes, the
        binning at most lsr_binning_bytes (the header: an upper bound; the forward asks for what its
        entry count needs)."""
        lib = _native.load()
        exact = {_native.LSR_BUF_GEOM: lib.lsr_geom_bytes(P, W, H), _native.LSR_BUF_IMAGE: lib.lsr_image_bytes(W, H),
                 _native.LSR_BUF_BACKWARD: lib.lsr_backward_bytes(P)}
        for which, want in exact.items():
            got = self.requested(("scratch", which))
            assert got is None or got == max(int(want), 1), f"scratch {which}: {got} bytes requested, not {want}"
        got = self.requested(("scratch", _native.LSR_BUF_BINNING))
        most = lib.lsr_binning_bytes(W, H, max(int(num_rendered), int(entries)))
        assert got is None or 0 < got <= max(int(most), 1), f"binning: {got} bytes requested, the ABI's bound is {most}"


class _TorchProxy:
    """torch, except that empty / zeros / empty_like / zeros_like return Guarded interiors."""

    def __init__(self, record):
        self._record = record

    def __getattr__(self, name):
        return getattr(torch, name)

    def _new(self, shape, dtype, device, fill):
        g = Guarded(shape, dtype if dtype is not None else torch.get_default_dtype(),
                    device if device is not None else "cpu", fill=fill, name=f"allocation {len(self._record.guards)}")
        self._record.guards.append(g)
        return g.tensor

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = size[0]
        return tuple(int(s) for s in size)

    def empty(self, *size, dtype=None, device=None):
        return self._new(self._shape(size), dtype, device, self._record.fill)

    def zeros(self, *size, dtype=None, device=None):
        return self._new(self._shape(size), dtype, device, 0x00)

    def empty_like(self, t, dtype=None, device=None):
        return self._new(t.shape, dtype or t.dtype, device or t.device, self._record.fill)

    def zeros_like(self, t, dtype=None, device=None):
        return self._new(t.shape, dtype or t.dtype, device or t.device, 0x00)


class Allocations:
    """What a guarded_allocations block handed out, in order."""

    def __init__(self, fill):
        self.fill = int(fill)
        self.guards = []

    def of(self, t):
        """The Guarded whose interior holds tensor `t` (a view of it included)."""
        p = t.data_ptr()
        for g in self.guards:
            p0 = g.tensor.data_ptr()
            if p0 <= p < p0 + max(g.nbytes, 1):
                return g
        raise KeyError("not a guarded allocation")

    def check_all(self):
        for g in self.guards:
            g.check()


@contextlib.contextmanager
def guarded_allocations(monkeypatch, module, fill=0x00):
    """Within the block, `module`'s global `torch` is a proxy whose four allocating calls return Guarded
    interiors (empty / empty_like filled with `fill`, zeros / zeros_like with zeros); yields the
    Allocations record.  The module gets its torch back on exit."""
    rec = Allocations(fill)
    with monkeypatch.context() as m:
        m.setattr(module, "torch", _TorchProxy(rec))
        yield rec
