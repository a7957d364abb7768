"""The guard harness itself (tests/guards.py) on CPU tensors: a byte written just outside an interior
is reported with its buffer's name and offset, a write inside is not, and the torch proxy of
guarded_allocations leaves the module as it found it."""
import pytest
import torch

from langsplat_amd import _native
from tests import guards
from tests.guards import GUARD, Guarded, GuardedBuffers, GuardError, guarded_allocations


@pytest.mark.parametrize("shape,dtype,misalign", [((7,), torch.float32, 0), ((3, 5, 3), torch.float32, 4),
                                                  ((13,), torch.uint8, 1), ((0,), torch.int32, 0),
                                                  ((66,), torch.int64, 8)])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_layout_fill_and_alignment(shape, dtype, misalign, fill):
    g = Guarded(shape, dtype, "cpu", fill=fill, misalign=misalign)
    assert tuple(g.tensor.shape) == shape and g.tensor.dtype == dtype and g.tensor.is_contiguous()
    assert g.tensor.data_ptr() % guards.ALIGN == misalign
    assert g.start >= guards.MIN_PAD and g.back_pad >= guards.MIN_PAD
    assert bool((g.backing[:g.start] == GUARD).all()) and bool((g.backing[g.end:] == GUARD).all())
    assert bool((g.bytes == fill).all()) and g.unwritten() == g.tensor.numel()
    g.check("fresh")


def test_pad_rule():
    assert guards.default_pad(100) == 64 * 1024
    assert guards.default_pad(4 * 1024 * 1024) == 1024 * 1024
    g = Guarded((1024 * 1024,), torch.uint8, "cpu")
    assert g.start >= 256 * 1024 and g.back_pad >= 256 * 1024
    g = Guarded((16,), torch.uint8, "cpu", front=512, back=1024)
    assert 512 <= g.start < 512 + guards.ALIGN and g.back_pad >= 1024


def test_write_before_and_after_the_interior_is_reported():
    g = Guarded((5,), torch.float32, "cpu", fill=0xFF)
    g.backing[g.end] = 0
    with pytest.raises(GuardError, match=r"lang grad: 1 guard byte\(s\) changed, the first at end\+0 "):
        g.check("lang grad")
    g.backing[g.end] = GUARD
    g.backing[g.end + 15] = 7
    with pytest.raises(GuardError, match=r"the first at end\+15 .*value 0x07"):
        g.check("x")
    g.backing[g.end + 15] = GUARD
    g.check("restored")
    g.backing[g.start - 1] = 0
    with pytest.raises(GuardError, match=r"moments: 1 guard byte\(s\) changed, the first at start-1 "):
        g.check("moments")
    g.backing[g.start - 8:g.start] = 0
    with pytest.raises(GuardError, match=r"8 guard byte\(s\) changed, the first at start-8 "):
        g.check("moments")


def test_write_inside_the_interior_is_not_reported_and_is_counted():
    g = Guarded((4, 3), torch.float32, "cpu", fill=0xFF)
    assert g.unwritten() == 12
    g.tensor[0, 0] = 1.5
    g.tensor[3, 2] = 0.0
    g.check("inside")
    assert g.unwritten() == 10
    g.bytes[4] = 0  # one byte of an element: that element no longer holds the pattern
    assert g.unwritten() == 9
    g.refill()
    assert g.unwritten() == 12
    # a value equal to the fill byte pattern counts as unwritten: why the tests look under 0xFF, not 0x00
    z = Guarded((4,), torch.float32, "cpu", fill=0x00)
    z.tensor[1] = 0.0
    assert z.unwritten() == 4


def test_gaps_between_views_are_guards():
    g = Guarded((192,), torch.float32, "cpu", fill=0xFF)
    a, b = g.tensor[0:30].view(10, 3), g.tensor[64:64 + 40].view(10, 4)
    a.zero_()
    b.fill_(2.0)
    g.assert_only_written([a, b, None])
    g.tensor[30] = 0.0  # the word after the first view
    with pytest.raises(GuardError, match="flat: 4 byte.s. between the views changed, the first at byte 120 "):
        g.assert_only_written([a, b], "flat")


def test_guarded_buffers_hand_out_exact_sizes_and_check_replaced_buffers():
    gb = GuardedBuffers(fill=0xFF, extra_back={("scratch", 1): 4096})
    with gb:
        assert _native.static_buffers.active() is gb
        t = gb.tensor(("scratch", 0), (1000,), torch.uint8, "cpu", at_least=True)
    assert _native.static_buffers.active() is None
    assert tuple(t.shape) == (1000,) and bool((t == 0xFF).all()) and t.data_ptr() % 256 == 0
    assert gb.tensor(("scratch", 0), (1000,), torch.uint8, "cpu", at_least=True).data_ptr() == t.data_ptr()
    out = gb.tensor(("out", "color"), (3, 5, 7), torch.float32, "cpu")
    assert tuple(out.shape) == (3, 5, 7) and gb.tensors[("out", "color")] is out
    b = gb.tensor(("scratch", 1), (10,), torch.uint8, "cpu", at_least=True)
    assert gb.guards[("scratch", 1)].back_pad >= guards.MIN_PAD + 4096
    assert gb.requested(("scratch", 0)) == 1000 and gb.requested(("out", "color")) == 420
    assert gb.requested(("scratch", 3)) is None
    gb.check_all()
    # a smaller request is a new buffer of exactly that size (no at_least slack for a stray store to hide in)
    s = gb.tensor(("scratch", 0), (600,), torch.uint8, "cpu", at_least=True)
    assert s.numel() == 600 and s.data_ptr() != t.data_ptr() and len(gb.retired) == 1
    # the old binning buffer was overrun by one byte: found when a larger request replaces it
    gb.guards[("scratch", 1)].backing[gb.guards[("scratch", 1)].end] = 0
    with pytest.raises(GuardError, match=r"\('scratch', 1\) \(before it was replaced\).*end\+0 "):
        gb.tensor(("scratch", 1), (20,), torch.uint8, "cpu", at_least=True)
    del b
    # and check_all names the buffer
    gb2 = GuardedBuffers()
    o = gb2.tensor(("out", "radii"), (9,), torch.int32, "cpu")
    gb2.guards[("out", "radii")].backing[gb2.guards[("out", "radii")].start - 4] = 1
    with pytest.raises(GuardError, match=r"\('out', 'radii'\).*start-4 "):
        gb2.check_all()
    o[:] = 3  # inside: fine
    gb2.guards[("out", "radii")].backing[gb2.guards[("out", "radii")].start - 4] = GUARD
    gb2.check_all()


def test_alloc_callback_goes_through_guarded_buffers():
    """_native's allocator callback (what lsr_forward calls for scratch) and output_tensor both land in
    the active GuardedBuffers, at exactly the requested size."""
    gb = GuardedBuffers(fill=0xFF)
    alloc = _native._Allocator(torch.device("cpu"))
    with gb, alloc:
        p = _native._alloc_cb(None, _native.LSR_BUF_GEOM, 12345)
        out = _native.output_tensor("color", (3, 4, 5), torch.float32, "cpu")
    g = gb.guards[("scratch", _native.LSR_BUF_GEOM)]
    assert p == g.tensor.data_ptr() and g.nbytes == 12345 and alloc.get(_native.LSR_BUF_GEOM).numel() == 12345
    assert out.data_ptr() == gb.guards[("out", "color")].tensor.data_ptr() and out.shape == (3, 4, 5)
    gb.check_all()


def test_proxy_guards_the_four_allocating_calls_and_restores_the_module(monkeypatch):
    from langsplat_amd import loss as module
    assert module.torch is torch
    with guarded_allocations(monkeypatch, module, fill=0xFF) as rec:
        assert module.torch is not torch
        assert module.torch.float32 is torch.float32 and module.torch.Tensor is torch.Tensor  # delegated
        e = module.torch.empty((5, 3), dtype=torch.float32, device="cpu")
        z = module.torch.zeros(7, dtype=torch.uint8, device="cpu")
        el = module.torch.empty_like(e)
        zl = module.torch.zeros_like(e, dtype=torch.int32)
        assert e.shape == (5, 3) and z.shape == (7,) and el.shape == (5, 3) and zl.dtype == torch.int32
        assert e.isnan().all() and not z.any() and el.isnan().all() and not zl.any()
        assert len(rec.guards) == 4 and rec.of(e) is rec.guards[0] and rec.of(zl[2:]) is rec.guards[3]
        rec.check_all()
        g = rec.of(z)
        g.backing[g.end] = 0
        with pytest.raises(GuardError, match=r"allocation 1: .*end\+0 "):
            rec.check_all()
    assert module.torch is torch


def test_proxy_restores_the_module_when_the_block_raises(monkeypatch):
    from langsplat_amd import knn as module
    with pytest.raises(RuntimeError, match="boom"):
        with guarded_allocations(monkeypatch, module):
            assert module.torch is not torch
            raise RuntimeError("boom")
    assert module.torch is torch
