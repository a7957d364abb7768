"""The view cache without a GPU: the C ABI's declarations, pack size and argument checks (dummy
pointers, never dereferenced: every check precedes the device work), and ViewCache's bookkeeping
against a stand-in for the native calls."""
import ctypes
import os
import re

import pytest

from langsplat_amd import _native
from langsplat_amd.pipeline import ViewCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsr_view_pack_bytes", "lsr_view_counts", "lsr_view_save", "lsr_view_restore")


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "lsr.h")).read()
    assert "#define LSR_ABI_VERSION 18" in header  # additive: detected by symbol
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES and getattr(lib, name) is not None


def _tiles(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def _up(n):
    return (n + 15) // 16 * 16


def _documented(P, W, H, R):
    """include/lsr.h: 320 B of counters, 32 P + 3 x 4 P per Gaussian, 8 T + 4 T per tile, 4 R."""
    T = _tiles(W, H)
    return 320 + 32 * P + 3 * _up(4 * P) + _up(8 * T) + _up(4 * T) + _up(4 * R)


@pytest.mark.parametrize("W,H", [(70, 50), (17, 33), (1920, 1080)])
def test_pack_bytes(W, H):
    f = _native.view_pack_bytes
    for P in (1, 2, 3, 4, 5, 1501, 1000003):
        for R in (0, 1, 3, 4, 7777, 8500001):
            n = f(P, W, H, R)
            assert n % 16 == 0 and n == _documented(P, W, H, R), (P, R)
    sizes_p = [f(P, W, H, 1000) for P in range(1, 40)]
    sizes_r = [f(300, W, H, R) for R in range(0, 40)]
    assert sizes_p == sorted(sizes_p) and sizes_p[0] < sizes_p[-1]
    assert sizes_r == sorted(sizes_r) and sizes_r[0] < sizes_r[-1]
    for bad in ((0, W, H, 0), (1, 0, H, 0), (1, W, 0, 0), (1, W, H, -1)):
        assert f(*bad) == 0


def _args(**kw):
    a = _native.LsrViewArgs()
    a.P, a.width, a.height = 100, 70, 50
    a.capacity_rendered, a.capacity_entries, a.num_rendered = 5000, 4000, 1234
    for name in ("geom", "image", "binning", "radii", "pack"):
        setattr(a, name, 0x10000)
    a.pack_bytes = _native.view_pack_bytes(100, 70, 50, 1234)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("fn", ["lsr_view_save", "lsr_view_restore"])
def test_invalid_arguments(fn):
    lib = _native.load()
    call = getattr(lib, fn)
    assert call(None, None) == 1
    cases = [dict(P=0), dict(P=-3), dict(width=0), dict(height=-1), dict(capacity_rendered=0),
             dict(capacity_entries=0), dict(num_rendered=-1), dict(num_rendered=5001),
             dict(geom=None), dict(image=None), dict(binning=None), dict(radii=None), dict(pack=None),
             dict(pack_bytes=_native.view_pack_bytes(100, 70, 50, 1234) - 1), dict(pack_bytes=0),
             dict(pack=0x10008), dict(geom=0x10004), dict(radii=0x10002), dict(flags=8), dict(reserved=1)]
    for kw in cases:
        assert call(ctypes.byref(_args(**kw)), None) == 1, kw
        assert fn in _native.last_error(), kw


def test_view_counts_invalid_arguments():
    lib = _native.load()
    for bad in ((0, 50, 0x10000, 0x20000), (70, 0, 0x10000, 0x20000), (70, 50, None, 0x20000), (70, 50, 0x10000, None),
                (70, 50, 0x10002, 0x20000), (70, 50, 0x10000, 0x20001)):
        assert lib.lsr_view_counts(*bad, None) == 1, bad
        assert "lsr_view_counts" in _native.last_error()


# ---- the bookkeeping -------------------------------------------------------------------------------------

class _Event:
    def __init__(self, done=True):
        self.done = done

    def query(self):
        return self.done


class _Native:
    """Records the calls; a pack is (bytes, serial)."""

    def __init__(self, per_instance=4, fixed=100):
        self.log = []
        self.per, self.fixed = per_instance, fixed

    def pack_bytes(self, rendered):
        return self.fixed + self.per * rendered

    def alloc(self, nbytes):
        self.log.append(("alloc", nbytes))
        return ("pack", nbytes, len(self.log))

    def save(self, r, rendered, pack):
        self.log.append(("save", r, rendered, pack))

    def restore(self, r, rendered, pack):
        self.log.append(("restore", r, rendered, pack))


def _host(rendered, overflow=0):
    h = [0] * 8
    h[ViewCache.RENDERED], h[ViewCache.OVERFLOW] = rendered, overflow
    return h


def _geometry(vc, r, key, rendered=10, overflow=0, done=True):
    """What PipelinedGraphStep._geometry does for set r and view `key`; True on a hit."""
    if vc.visit(r, key):
        return True
    vc.computed(r, key, object(), _Event(done), _host(rendered, overflow))
    return False


def test_a_view_is_saved_when_its_set_is_released_and_then_hits():
    n = _Native()
    vc = ViewCache(3, 10_000, n)
    assert not _geometry(vc, 0, "a", rendered=10)
    assert not _geometry(vc, 1, "b", rendered=20)
    assert not _geometry(vc, 2, "a")           # "a" again before set 0 was released: still a miss
    assert n.log == []
    assert not _geometry(vc, 0, "c")           # set 0 released: "a" saved first, then "c" computed
    assert [e[0] for e in n.log] == ["alloc", "save"] and n.log[1][1:3] == (0, 10)
    assert _geometry(vc, 1, "a")               # "b" saved from set 1, then "a" restored into it
    assert [e[0] for e in n.log[2:]] == ["alloc", "save", "restore"]
    assert n.log[3][1:3] == (1, 20) and n.log[4][1:3] == (1, 10) and n.log[4][3] == n.log[1][3]
    assert _geometry(vc, 2, "b")               # set 2 held "a", which has a pack: no second save
    assert [e[0] for e in n.log[5:]] == ["restore"]
    st = vc.stats()
    assert st == {"hits": 2, "misses": 4, "packs": 2, "bytes": n.pack_bytes(10) + n.pack_bytes(20), "drops": 0}
    assert _geometry(vc, 1, "b") and vc.pending[1] is None  # a restored set holds nothing to save


def test_no_wait_no_overflow_and_the_budget():
    n = _Native()
    vc = ViewCache(2, n.pack_bytes(10) + n.pack_bytes(10) - 1, n)   # room for one pack of 10 instances
    _geometry(vc, 0, "late", done=False)
    _geometry(vc, 1, "over", overflow=0x3F800000)
    assert not _geometry(vc, 0, "x", rendered=10)   # the event has not signalled: skipped, not waited for
    assert not _geometry(vc, 1, "y", rendered=10)   # the view overflowed: never cached
    assert n.log == [] and vc.stats()["packs"] == 0
    assert not _geometry(vc, 0, "late")             # "x" saved
    assert not _geometry(vc, 1, "over")             # "y" does not fit the budget: not saved
    assert [e[0] for e in n.log] == ["alloc", "save"] and set(vc.packs) == {"x"}
    assert _geometry(vc, 0, "x") and not _geometry(vc, 1, "y")
    assert vc.stats()["bytes"] == n.pack_bytes(10) <= vc.budget
    assert ViewCache(2, 0, n).budget == 0


def test_the_stamp_and_invalidate_drop_everything():
    n = _Native()
    vc = ViewCache(2, 10_000, n)
    vc.check((1, 0))
    _geometry(vc, 0, "a")
    _geometry(vc, 1, "b")
    _geometry(vc, 0, "b")
    assert set(vc.packs) == {"a"} and vc.pending[1] is not None
    vc.check((1, 0))
    assert set(vc.packs) == {"a"}                   # the same stamp: kept
    vc.check((1, 1))                                # an in-place edit (the version moved)
    assert vc.packs == {} and vc.pending == [None, None] and vc.bytes == 0 and vc.stats()["drops"] == 1
    assert not _geometry(vc, 1, "a")                # nothing computed before the change is saved
    assert not _geometry(vc, 0, "c") and vc.packs == {}
    assert _geometry(vc, 1, "zz") is False and set(vc.packs) == {"a"}   # computed after it: saved
    vc.check((2, 1))                                # the tensor was replaced (another address)
    assert vc.packs == {} and vc.stats()["drops"] == 2
    _geometry(vc, 0, "k")
    _geometry(vc, 0, "k2")
    assert set(vc.packs) == {"k"}
    vc.invalidate()
    assert vc.packs == {} and vc.stats()["drops"] == 3 and vc.stats()["bytes"] == 0


def test_keys_hold_their_reference():
    """The cache keeps the camera object with its id, so the id cannot be reused by another view."""
    n = _Native()
    vc = ViewCache(2, 10_000, n)
    cam = object()
    assert not vc.visit(0, id(cam))
    vc.computed(0, id(cam), cam, _Event(), _host(5))
    assert vc.pending[0][1] is cam
    assert not vc.visit(0, "other")
    assert vc.packs[id(cam)][0] is cam
