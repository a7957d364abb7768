"""The bound form of the view cache without a GPU (include/lsr.h lsr_view_bind): the declarations, the
layout arithmetic of the plane and the table, the argument checks (dummy pointers, never
dereferenced: every check precedes the device work) and ViewCache's protocol against a stand-in for
the native calls."""
import ctypes
import os
import re

import pytest

from langsplat_amd import _native
from langsplat_amd.pipeline import ViewCache
from tests.test_view_cache_cpu import _args, _Event, _Native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_optional():
    header = open(os.path.join(ROOT, "include", "lsr.h")).read()
    assert "#define LSR_ABI_VERSION 18" in header  # additive: detected by symbol
    lib = _native.load()
    for name in _native.OPTIONAL:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES and getattr(lib, name) is not None
    assert _native.has_view_bind()
    enum = re.search(r"enum lsr_bind_flags \{([^}]*)\}", header).group(1)
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in enum.split(",") if "=" in e))
    assert vals == {"LSR_BIND_FORWARD": _native.BIND_FORWARD, "LSR_BIND_BACKWARD": _native.BIND_BACKWARD,
                    "LSR_BIND_FILL_PLANE": _native.BIND_FILL_PLANE, "LSR_BIND_CLAMPED": _native.BIND_CLAMPED}
    # above lsr_forward_flags' (1, 2, 4) and lsr_backward_flags' (1, 2, 4) own bits
    assert _native.BIND_FORWARD > 4 and _native.BIND_BACKWARD > 4 and _native.BIND_FILL_PLANE > 4
    assert _native.BIND_BACKWARD != _native.BIND_FILL_PLANE


@pytest.mark.parametrize("W,H", [(70, 50), (17, 33), (1920, 1080)])
def test_layout_arithmetic(W, H):
    lib = _native.load()
    for P in (1, 2, 3, 302, 1501, 1000003):
        lay = _native.view_bind_layout(P, W, H)
        geom = lib.lsr_geom_bytes(P, W, H)
        assert lay["plane"] % 16 == 0 and lay["table"] % 16 == 0
        assert lay["plane"] + 16 * P <= lay["table"] and lay["table"] + 32 <= geom
        # behind everything the geometry buffer held before: no earlier offset moved
        st = _native.state_layout(P, W, H, 0)
        assert all(st[k] < lay["plane"] for k in ("depth_key", "tiles_touched", "rect", "record", "clamped",
                                                  "sorted_ids", "super_offset", "grad_records"))
        assert st["record"] + 48 * P <= lay["plane"]
    assert lib.lsr_image_bytes(W, H) > 0  # (the table and the plane live in the geometry buffer)
    one, two = _native.view_bind_layout(1000, W, H), _native.view_bind_layout(2000, W, H)
    assert two["table"] - two["plane"] >= 16 * 2000 > one["table"] - one["plane"] >= 16 * 1000
    sz = ctypes.c_size_t(0)
    assert lib.lsr_view_bind_layout(-1, W, H, ctypes.byref(sz), ctypes.byref(sz)) == 1
    assert lib.lsr_view_bind_layout(10, W, H, None, ctypes.byref(sz)) == 1
    assert "lsr_view_bind_layout" in _native.last_error()


def test_bind_invalid_arguments():
    lib = _native.load()
    assert lib.lsr_view_bind(None, 0, None) == 1
    full = _native.view_pack_bytes(100, 70, 50, 1234)
    cases = [dict(P=0), dict(P=-3), dict(width=0), dict(height=-1), dict(capacity_rendered=0),
             dict(capacity_entries=0), dict(num_rendered=-1), dict(num_rendered=5001),
             dict(geom=None), dict(image=None), dict(binning=None), dict(radii=None),
             dict(pack_bytes=full - 1), dict(pack_bytes=0), dict(pack=0x10008), dict(geom=0x10004),
             dict(radii=0x10002), dict(flags=8), dict(flags=_native.BIND_FORWARD), dict(reserved=1)]
    for kw in cases:
        assert lib.lsr_view_bind(ctypes.byref(_args(**kw)), 0, None) == 1, kw
        assert "lsr_view_bind" in _native.last_error(), kw
    # a null binding (the table lives in the geometry buffer) is refused with or without a pack
    assert lib.lsr_view_bind(ctypes.byref(_args(geom=None, pack=None, pack_bytes=0)), 0, None) == 1
    assert "table" in _native.last_error()
    assert lib.lsr_view_bind(ctypes.byref(_args()), 2, None) == 1 and "bind flag" in _native.last_error()


def test_flags_are_refused_where_they_mean_nothing():
    """LSR_BIND_FORWARD needs a forward phase; LSR_BIND_FILL_PLANE needs a fill target."""
    lib = _native.load()
    s, a = _native.LsrSettings(), _native.LsrForwardArgs()
    s.image_width, s.image_height = 70, 50
    for name in ("bg", "viewmatrix", "projmatrix", "campos"):
        setattr(s, name, 0x10000)
    a.P, a.flags = 10, _native.BIND_FORWARD
    for name in ("means3D", "opacities", "shs", "scales", "rotations", "out_color", "out_language_feature", "radii"):
        setattr(a, name, 0x10000)
    a.M = 1
    nr = ctypes.c_int64(0)
    assert lib.lsr_forward(ctypes.byref(s), ctypes.byref(a), _native._ALLOC_CB, None, None, ctypes.byref(nr)) == 1
    assert "LSR_BIND_FORWARD" in _native.last_error()
    b = _native.LsrBackwardArgs()
    b.P, b.flags = 10, _native.BIND_FILL_PLANE
    assert lib.lsr_backward(ctypes.byref(s), ctypes.byref(b), _native._ALLOC_CB, None, None) == 1
    assert "LSR_BIND_FILL_PLANE" in _native.last_error()


# ---- the protocol -----------------------------------------------------------------------------------------

class _BindNative(_Native):
    """test_view_cache_cpu's stand-in plus the bound form's calls; done[r]: set r's step has finished."""

    def __init__(self, can=True, sets=3, **kw):
        super().__init__(**kw)
        self.can = can
        self.done = [True] * sets

    def can_bind(self):
        return self.can

    def bind(self, r, rendered, pack):
        self.log.append(("bind", r, rendered, pack))

    def step_done(self, r):
        return self.done[r]


def _cached(vc, nat, r, key, rendered=50):
    """View `key` through set r: a miss, its counters arrive, the set's next visit saves it."""
    assert vc.visit(r, key) is False
    host = [0] * 8
    host[ViewCache.RENDERED] = rendered
    vc.computed(r, key, None, _Event(True), host)
    assert vc.save_pending(r)
    return vc.packs[key][2]


def test_a_hit_binds_and_a_miss_runs_the_geometry():
    nat = _BindNative()
    vc = ViewCache(3, 10**6, nat)
    assert vc.bind
    pack = _cached(vc, nat, 0, "a")
    assert [e[0] for e in nat.log] == ["alloc", "save"]
    assert vc.visit(1, "a") is True
    assert nat.log[-1] == ("bind", 1, 50, pack) and vc.bound[1] is pack
    assert not any(e[0] == "restore" for e in nat.log)
    n = len(nat.log)
    assert vc.visit(2, "b") is False and len(nat.log) == n  # a miss enqueues nothing: the caller runs G_geo
    assert vc.stats()["hits"] == 1 and vc.stats()["misses"] == 2


def test_a_missing_symbol_falls_back_to_the_restore():
    for nat in (_BindNative(can=False), _Native()):  # the library lacks lsr_view_bind / an older stand-in
        vc = ViewCache(3, 10**6, nat)
        assert not vc.bind
        pack = _cached(vc, nat, 0, "a")
        assert vc.visit(1, "a") is True
        assert nat.log[-1] == ("restore", 1, 50, pack) and vc.bound == [None] * 3
    # _native.load() tolerates a library of the same ABI without the optional symbols
    assert set(_native.OPTIONAL) <= set(_native.SIGNATURES)


def test_one_pack_may_be_bound_into_several_sets():
    nat = _BindNative()
    vc = ViewCache(3, 10**6, nat)
    pack = _cached(vc, nat, 0, "a")
    assert vc.visit(0, "a") and vc.visit(1, "a") and vc.visit(2, "a")
    assert vc.bound == [pack, pack, pack] and vc.retired == []
    assert [e[:2] for e in nat.log[-3:]] == [("bind", 0), ("bind", 1), ("bind", 2)]
    assert vc.visit(1, "a") and vc.retired == []  # the same pack again: nothing to retire


def test_a_pack_is_held_until_the_bound_sets_step_event():
    nat = _BindNative()
    vc = ViewCache(3, 10**6, nat)
    pa = _cached(vc, nat, 0, "a")
    pb = _cached(vc, nat, 1, "b")
    assert vc.visit(2, "a") and vc.bound[2] is pa
    # every pack is dropped while set 2 is bound to one: the set keeps its reference
    vc.invalidate()
    assert vc.packs == {} and vc.bound[2] is pa and vc.stats()["drops"] == 1
    # set 2's next visit (a miss now): its step may still be reading the pack
    nat.done[2] = False
    assert vc.visit(2, "b") is False
    assert vc.bound[2] is None and vc.retired == [(2, pa)]
    assert vc.visit(0, "c") is False and vc.retired == [(2, pa)]  # other sets' visits do not release it
    # ... until the set's step event has completed
    nat.done[2] = True
    assert vc.visit(0, "c") is False and vc.retired == []
    # a hit with another pack retires the one the set was bound to in the same way
    pc = _cached(vc, nat, 1, "d")
    pd = _cached(vc, nat, 0, "e")
    assert vc.visit(2, "d") and vc.bound[2] is pc
    nat.done[2] = False
    assert vc.visit(2, "e") and vc.bound[2] is pd and vc.retired == [(2, pc)]
    assert pb is not pa


def test_disable_keeps_the_bound_packs_and_stops_caching():
    """A geometry tensor became trainable: the step switches the cache off but keeps the object, because
    sets bound ahead still read their packs in steps that are not enqueued yet."""
    nat = _BindNative()
    vc = ViewCache(3, 10**6, nat)
    pa = _cached(vc, nat, 0, "a")
    assert vc.visit(1, "a") and vc.visit(2, "a")
    vc.disable()
    assert vc.off and vc.packs == {} and vc.bound[1] is pa and vc.bound[2] is pa and vc.stats()["drops"] == 1
    n = len(nat.log)
    nat.done[1] = False
    assert vc.visit(1, "a") is False and vc.retired == [(1, pa)] and vc.bound[2] is pa
    host = [0] * 8
    host[ViewCache.RENDERED] = 50
    vc.computed(1, "a", None, _Event(True), host)  # nothing is pending while it is off
    assert vc.pending[1] is None and not vc.save_pending(1) and len(nat.log) == n
