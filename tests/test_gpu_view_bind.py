"""The bound form of the view cache (include/lsr.h lsr_view_bind; langsplat_amd.pipeline): a buffer set
whose table names a view pack must serve the composite phase and both backwards exactly as the set
the geometry phase filled -- reading the pack's records and point list where they are -- and the
step must compute in the bound form what it computes with the copying restore and with no cache.

Shapes (tests/test_gpu_view_cache.py's): 70 x 50 with 1501 Gaussians (5 x 4 tiles, partial edge
tiles, more than one workgroup of the bind kernel) and 17 x 33 with 302; counts are no multiple of 4.
Exact outputs (images, loss, radii, final_T, n_contrib) are compared bit for bit, gradients with
assert_grad_close (the float atomics' tolerance), step states with assert_states_close.
"""
import ctypes
import weakref

import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.distributed import GradBucket
from langsplat_amd.graph import ViewSlot
from langsplat_amd.pipeline import PipelinedGraphStep
from langsplat_amd.render import render
from tests.scenes import scene
from tests.test_gpu_captured_forms import _adam, _frozen_model, _slot_forward, _state, assert_states_close
from tests.test_gpu_fused import _Opt, _Pipe
from tests.test_gpu_view_cache import (COMPOSITE, DEV, SEQ, _assert_same, _Case, _edge_case, _gaussians, _Set, _views,
                                       bench_target)

pytestmark = pytest.mark.gpu
GEOM, IMAGE, BINNING = _native.LSR_BUF_GEOM, _native.LSR_BUF_IMAGE, _native.LSR_BUF_BINNING


def _bound_set():
    s = _Set()
    s.bufs.view_bind = True  # its split-phase forwards and their backwards go through the set's table
    return s


def _plane(case, s):
    off = _native.view_bind_layout(case.P, case.W, case.H)["plane"]
    return s.tensor(GEOM)[off:off + 16 * case.P].view(torch.float32).view(case.P, 4)


def _table(case, s):
    off = _native.view_bind_layout(case.P, case.W, case.H)["table"]
    t = s.tensor(GEOM)[off:off + 32].cpu()
    ptrs = t[:24].view(torch.int64).tolist()
    return ptrs + t[24:].view(torch.int32).tolist()  # rec01, recb, point_list, s01, sb


def _own_arrays(case, s):
    """The bytes of set s's own record array and point list (up to its capacity)."""
    rec = s.tensor(GEOM)[case.lay["record"]:case.lay["record"] + 48 * case.P]
    pl = s.tensor(BINNING)[case.lay["point_list"]:case.lay["point_list"] + 4 * case.cap[0]]
    return rec, pl


def _bind(case, s, rendered, pack):
    a = _native.view_args(s.bufs, rendered, pack)
    _native.view_bind(a, torch.cuda.current_stream(), clamped=case.mode == "all")


def _bind_identity(s):
    a = _native.view_args(s.bufs, 0, torch.empty((16,), dtype=torch.uint8, device=DEV))
    a.pack, a.pack_bytes = None, 0
    _native.view_bind(a, torch.cuda.current_stream())


def _blank_bound(case, s, seed):
    """Every byte of set s to 0xFF (its overflow flag set), then known values in its plane's slots."""
    for which in (GEOM, IMAGE, BINNING):
        s.tensor(which).fill_(0xFF)
    s.bufs.tensors[("out", "radii")].fill_(-1)
    s.overflow.fill_(0x3F800000)
    vals = torch.randn((case.P, 4), generator=torch.Generator().manual_seed(seed)).to(DEV)
    _plane(case, s).copy_(vals)
    return vals


def _composite(case, s):
    """case.composite(s) with what a caller of the native calls owes a bound set: the backward's
    BIND_BACKWARD flag (langsplat_amd.rasterizer keeps it in the autograd context)."""
    exact, out = _forward_only(case, s)
    return exact, _backward_only(case, out, s.bufs.view_bind)


def _reference(case):
    """Geometry into an unbound set A, its composite + backward, and A's pack saved after them."""
    A = _Set()
    case.geometry(A)
    ref = _composite(case, A)
    rendered, pack = case.pack_of(A)
    return A, ref, rendered, pack


# ---- 1. a bound composite equals the original -----------------------------------------------------------

def _bound_round_trip(case, tag):
    A, ref, rendered, pack = _reference(case)
    before = pack.clone()
    B = _bound_set()
    case.geometry(B)  # (allocates B at the capacity sizes)
    vals = _blank_bound(case, B, seed=11)
    _bind(case, B, rendered, pack)
    plane = _plane(case, B)
    assert torch.equal(plane[:, 1:4], vals[:, 1:4]), f"{tag}: the bind touched the language slots"
    vis = A.bufs.tensors[("out", "radii")] > 0
    assert torch.equal(plane[vis, 0], case.records(A)[vis, 8]), f"{tag}: b did not reach the plane"
    assert int(B.overflow.item()) == 0
    cb, ca = case.counters(B), case.counters(A)
    assert int(cb[7]) == 0 and [int(cb[i]) for i in (1, 2, 4, 5, 6)] == [int(ca[i]) for i in (1, 2, 4, 5, 6)]
    rec01, recb, plist, s01, sb = _table(case, B)
    # (an empty point list sits at the pack's very end)
    assert (s01, sb) == (2, 1) and pack.data_ptr() <= rec01 < plist <= pack.data_ptr() + pack.numel() - 4 * rendered
    assert recb == plane.data_ptr()
    got = _composite(case, B)
    _assert_same(case, ref, got, tag)
    rec, pl = _own_arrays(case, B)
    assert bool((rec == 0xFF).all()) and bool((pl == 0xFF).all()), f"{tag}: the set's own records / point list " \
                                                                    "were written: not read in place"
    assert torch.equal(pack, before), f"{tag}: the pack was written"
    return ref


@pytest.mark.parametrize("mode", ["language", "all"])
@pytest.mark.parametrize("W,H,P", [(70, 50, 1501), (17, 33, 302)])
def test_bound_composite_equals_the_original(mode, W, H, P):
    st, inp = scene(P=P, W=W, H=H, seed=4, scale_range=(0.03, 0.2))
    case = _Case(st, inp, mode)
    ref = _bound_round_trip(case, f"{mode} {W}x{H}")
    assert case.counts[0] > 0 and float(ref[0]["loss"]) > 0
    assert any(float(v.abs().sum()) > 0 for v in ref[1].values())


# ---- 2. the identity binding (a miss) --------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["language", "all"])
@pytest.mark.parametrize("how", ["geometry phase", "lsr_view_bind without a pack"])
def test_identity_bind(mode, how):
    st, inp = scene(P=1501, W=70, H=50, seed=4, scale_range=(0.03, 0.2))
    case = _Case(st, inp, mode)
    A = _Set()
    case.geometry(A)
    ref = _composite(case, A)  # the plain composite phase on an unbound set
    if how == "geometry phase":
        B = _bound_set()
        case.geometry(B)  # the preprocess writes the table and b
    else:
        B = _Set()
        case.geometry(B)
        B.bufs.view_bind = True
        _plane(case, B).fill_(float("nan"))  # (whatever the plane held: the bind brings b, the composite's fill f)
        _bind_identity(B)
    rec01, recb, plist, s01, sb = _table(case, B)
    rec, pl = _own_arrays(case, B)
    assert (rec01, plist, s01, sb) == (rec.data_ptr(), pl.data_ptr(), 3, 1) and recb == _plane(case, B).data_ptr()
    _assert_same(case, ref, _composite(case, B), f"identity {mode} {how}")


# ---- 3. re-initialisation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["language", "all"])
def test_bind_reinitialises(mode):
    """Three composite + backward passes on ONE bound set with a bind between them: the same bits each
    time (stale loss words, work-class counters or forward flags would show); a fourth with another
    target equals a fresh set's.  (tests/test_gpu_view_cache.py test_restore_reinitialises' scenario.)"""
    st, inp = scene(P=1501, W=70, H=50, seed=5, scale_range=(0.03, 0.2))
    case = _Case(st, inp, mode)
    A = _bound_set()
    case.geometry(A)
    first = _composite(case, A)
    rendered, pack = case.pack_of(A)

    def bind():  # (the set's plane held another view's b since)
        _plane(case, A)[:, 0] = 7.0
        _bind(case, A, rendered, pack)

    bind()
    _assert_same(case, first, _composite(case, A), f"{mode} second pass")
    bind()
    _assert_same(case, first, _composite(case, A), f"{mode} third pass")
    case.gt = torch.nn.functional.normalize(bench_target(case.H, case.W, 5)[0], dim=0).to(DEV).contiguous().neg()
    bind()
    fourth = _composite(case, A)
    C = _Set()
    case.geometry(C)
    _assert_same(case, _composite(case, C), fourth, f"{mode} another target")
    assert not torch.equal(fourth[0]["loss"], first[0]["loss"])


# ---- 4. two sets on one pack ---------------------------------------------------------------------------------

def _forward_only(case, s):
    out = case._forward(s, COMPOSITE)
    nr, color, lang, radii, geom, binning, image = out
    HW = case.H * case.W
    exact = {"color": color.clone(), "language": lang.clone(), "loss": s.loss.clone(), "radii": radii.clone()}
    for name, dt in (("final_T", torch.float32), ("n_contrib", torch.int32)):
        exact[name] = image[case.lay[name]:case.lay[name] + 4 * HW].view(dt).clone()
    return exact, out


def _backward_only(case, out, bound):
    nr, color, lang, radii, geom, binning, image = out
    bind = _native.BIND_BACKWARD if bound else 0
    i = case.inp
    common = (case.st, i["means3D"], i["shs"], None, i["language_feature_precomp"], i["scales"], i["rotations"],
              None, radii)
    if case.mode == "language":
        g = _native.rasterize_gaussians_backward(*common, None, None, nr, geom, binning, image,
                                                 opacities=i["opacities"], geometry=False, grad_loss=case.one,
                                                 flags=_native.BWD_RECORDS_ZEROED | bind)
    else:
        g = _native.rasterize_gaussians_backward(*common, case.gc, case.gl, nr, geom, binning, image,
                                                 opacities=i["opacities"], geometry=True, grad_loss=case.one, flags=bind)
    return {k: v.clone() for k, v in g.items() if v is not None}


@pytest.mark.parametrize("mode", ["language", "all"])
def test_two_sets_on_one_pack(mode):
    st, inp = scene(P=1501, W=70, H=50, seed=4, scale_range=(0.03, 0.2))
    case = _Case(st, inp, mode)
    _, ref, rendered, pack = _reference(case)
    before = pack.clone()
    A, B = _bound_set(), _bound_set()
    for s in (A, B):
        case.geometry(s)
        _blank_bound(case, s, seed=12)
    _bind(case, A, rendered, pack)
    _bind(case, B, rendered, pack)
    ea, oa = _forward_only(case, A)
    eb, ob = _forward_only(case, B)
    ga, gb = _backward_only(case, oa, True), _backward_only(case, ob, True)
    _assert_same(case, ref, (ea, ga), f"{mode} set A")
    _assert_same(case, ref, (eb, gb), f"{mode} set B")
    assert torch.equal(pack, before)


# ---- 5. edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["language", "all"])
@pytest.mark.parametrize("name", ["nothing", "one", "full"])
def test_edge_views(name, mode):
    if name == "full":  # a view that exactly fills its capacity
        st, inp = scene(P=1501, W=70, H=50, seed=4, scale_range=(0.03, 0.2))
        case = _Case(st, inp, mode)
        case.cap = case.counts
    else:
        case = _edge_case(name, mode)
    assert (case.counts[0] == 0) == (name == "nothing")
    _bound_round_trip(case, f"{name} {mode}")


def test_misuse_on_device_buffers():
    st, inp = scene(P=302, W=17, H=33, seed=4)
    case = _Case(st, inp, "language")
    A = _bound_set()
    case.geometry(A)
    torch.cuda.synchronize()
    rendered = case.counts[0]
    pack = torch.empty((_native.view_pack_bytes(case.P, case.W, case.H, rendered) + 16,), dtype=torch.uint8, device=DEV)
    lib = _native.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw, word in ((dict(pack_bytes=_native.view_pack_bytes(case.P, case.W, case.H, rendered) - 1), "pack_bytes"),
                     (dict(geom=None), "table"), (dict(num_rendered=case.cap[0] + 1), "num_rendered"),
                     (dict(pack=pack.data_ptr() + 4), "aligned")):
        a = _native.view_args(A.bufs, rendered, pack)
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.lsr_view_bind(ctypes.byref(a), 0, stream) == 1, kw
        assert "lsr_view_bind" in _native.last_error() and word in _native.last_error(), kw
    torch.cuda.synchronize()


# ---- 6. the step ----------------------------------------------------------------------------------------------

def _drop_and_reuse(pg, drop, visited=None):
    """Run `drop` (something that drops every pack) and then ask the allocator for blocks of the dropped
    packs' sizes, zero-filled: had the cache let go of a pack that a set bound ahead still reads, the
    allocator (idle: the device was synchronised) would hand its memory out here, and the next composites
    would read zeros -- Gaussian 0 everywhere, zero records -- instead of the view: the comparison with
    the other forms would fail.  The test itself holds no pack: only addresses and weak references.
    visited: the set that `drop` itself gives new geometry (a replay's), whose pack may go."""
    vc = pg._views
    if vc is None or not vc.bind:
        drop()
        return None
    sizes = [p.numel() for p in vc.bound if p is not None]
    addrs = [p.data_ptr() if p is not None else None for p in vc.bound]
    refs = [weakref.ref(p) if p is not None else None for p in vc.bound]
    ahead = [i for i, a in enumerate(addrs) if a is not None and i != visited]
    assert ahead, "no set is bound ahead at this point of the run"
    drop()
    assert vc is pg._views and vc.packs == {}, "the cache object (and its references) must survive the drop"
    for i in ahead:  # the cache still owns what the sets bound ahead will read
        assert vc.bound[i] is not None and vc.bound[i].data_ptr() == addrs[i] and refs[i]() is not None, i
    return [torch.zeros((n,), dtype=torch.uint8, device=DEV) for n in sizes for _ in range(2)]


def _run(g, views, seq, sets, wait, at=None, what=None, bucket=None, **kw):
    """A PipelinedGraphStep with slots over views[seq]; before replay `at`: "invalidate" (invalidate_views),
    "edit" (an in-place edit of a frozen geometry tensor), "trainable" (a geometry tensor starts to require
    grad: the cache switches off) or "param" (the caller halves the feature and calls follow_caller: the
    refill path) -> (losses, state, step).  bucket: the N > 1 structure on one process (a GradBucket
    without a process group, as tests/test_gpu_captured_forms.py uses it)."""
    m = _frozen_model(g)
    opt = _adam(m)
    slots = [ViewSlot(*views[seq[0]]) for _ in range(sets)]
    pg = PipelinedGraphStep(_slot_forward(m), [m._language_feature], opt, slots=slots, model=m,
                            bucket=GradBucket([m._language_feature]) if bucket else None, **kw)
    pg.capture(views=[views[v] for v in seq[:sets - 1]])
    L = sets - 1
    losses, junk = [], None
    for k in range(len(seq)):
        if k == at:
            pg.synchronize()
            torch.cuda.synchronize()
            if what == "invalidate":
                junk = _drop_and_reuse(pg, pg.invalidate_views)
            elif what == "trainable":
                # (the drop happens inside the next replay; the blocks are asked for right after it)
                m._opacity.requires_grad_(True)
            elif what == "edit":
                with torch.no_grad():
                    m._xyz.mul_(1.01)
            elif what == "param":
                with torch.no_grad():
                    m._language_feature.mul_(0.5)
                pg.follow_caller()
        nxt = views[seq[k + L]] if k + L < len(seq) else None
        if k == at and what == "trainable":
            def replay():
                losses.append(pg.replay(next_view=nxt, wait=wait))
            junk = _drop_and_reuse(pg, replay, visited=(k + L) % sets)
        else:
            losses.append(pg.replay(next_view=nxt, wait=wait))
        pg.synchronize()
        torch.cuda.synchronize()
        losses[-1] = losses[-1].clone()
    assert pg.check()
    pg.sync()
    del junk
    return torch.stack(losses), _state(m, opt), pg


@pytest.mark.parametrize("what", [None, "invalidate", "edit", "trainable", "param"])
@pytest.mark.parametrize("wait", [True, False])
def test_step_bound_matches_copying_and_uncached(what, wait, monkeypatch):
    """12 replays (4 S) over three rotating views, one of them on consecutive steps (SEQ): the bound form
    against view_cache=False and against the forced copying form.  The losses agree to the step's
    existing tolerance (the backward's float atomics reorder the gradient sums from run to run, so the
    feature, and with it the next loss, is not bit-stable in any form)."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g, views = _gaussians(), _views()
    l0, s0, _ = _run(g, views, SEQ, 3, wait, at=6, what=what, view_cache=False)
    lc, sc, pc = _run(g, views, SEQ, 3, wait, at=6, what=what, view_cache="copy")
    lb, sb, pb = _run(g, views, SEQ, 3, wait, at=6, what=what)
    assert pb.bound and pb._views.bind and not pc.bound and not pc._views.bind
    assert all(st.view_bind for st in pb.sets) and not any(st.view_bind for st in pc.sets)
    for tag, l, s in (("bound vs uncached", l0, s0), ("bound vs copying", lc, sc)):
        torch.testing.assert_close(lb, l, rtol=1e-5, atol=0)
        assert_states_close(sb, s, f"{tag}, {what}, wait={wait}")
    st, stc = pb.view_cache_stats(), pc.view_cache_stats()
    assert st["hits"] + st["misses"] == len(SEQ) + 2 and st["hits"] >= (2 if what in ("invalidate", "edit") else 4), st
    assert (st["hits"], st["misses"], st["drops"]) == (stc["hits"], stc["misses"], stc["drops"])
    assert st["drops"] == (1 if what in ("invalidate", "edit", "trainable") else 0)
    if what == "trainable":  # switched off, not discarded: nothing was hit or saved after the flip
        assert pb._views.off and pb._views.packs == {} and st["hits"] == 4, st
    assert pb.captures == 1


@pytest.mark.parametrize("form", ["defer", "fill"])
def test_step_bound_n_gt_1_forms(form, monkeypatch):
    """The N > 1 structure on one process, with model= so that the sets are bound: "defer", the deferred
    tail (lsr_language_tail with LSR_BIND_FILL_PLANE); "fill" (LSR_PG_DEFER=0), the update through
    lsr_adam_fill_language_plane.  Both start with the plane refilled from the parameter (no earlier
    update filled the first composite's slots).  Against the forced copying form and the uncached one."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    monkeypatch.setenv("LSR_PG_DEFER", "0" if form == "fill" else "1")
    g, views = _gaussians(), _views()
    l0, s0, _ = _run(g, views, SEQ, 3, True, bucket=True, view_cache=False)
    lc, sc, pc = _run(g, views, SEQ, 3, True, bucket=True, view_cache="copy")
    lb, sb, pb = _run(g, views, SEQ, 3, True, bucket=True)
    assert pb.bound and pb._views.bind and not pc.bound and pb.fill_after and pb.defer == (form == "defer")
    for tag, l, s in (("bound vs uncached", l0, s0), ("bound vs copying", lc, sc)):
        torch.testing.assert_close(lb, l, rtol=1e-5, atol=0)
        assert_states_close(sb, s, f"{tag}, N > 1 {form}")
    st, stc = pb.view_cache_stats(), pc.view_cache_stats()
    assert st["hits"] >= 4 and (st["hits"], st["misses"]) == (stc["hits"], stc["misses"]), st


def test_fixed_view_binds_several_sets_to_one_pack(monkeypatch):
    """No slots (bench.py's form): one constant key, so from the second visit on every set is bound to
    the one pack, several at once."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g = _gaussians()
    cam, gt, mask = _views(1)[0]
    bg = torch.zeros(3, device=DEV)

    def run(**kw):
        m = _frozen_model(g)
        opt = _adam(m)
        pg = PipelinedGraphStep(lambda: render(cam, m, _Pipe, bg, _Opt, language_target=(gt, mask))["language_l1"],
                                [m._language_feature], opt, model=m, **kw)
        pg.capture()
        losses = []
        for _ in range(9):
            losses.append(pg.replay().clone())
            torch.cuda.synchronize()
        assert pg.check()
        pg.sync()
        return torch.stack(losses), _state(m, opt), pg

    l0, s0, _ = run(view_cache=False)
    l1, s1, pg = run()
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=0)
    assert_states_close(s1, s0, "fixed view, bound")
    st = pg.view_cache_stats()
    assert st["packs"] == 1 and st["misses"] == 3 and st["hits"] == 8, st
    (pack,) = [v[2] for v in pg._views.packs.values()]
    assert all(b is pack for b in pg._views.bound)
