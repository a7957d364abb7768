"""The view cache of the pipelined language step (include/lsr.h lsr_view_save / lsr_view_restore,
langsplat_amd.pipeline.PipelinedGraphStep view_cache): a restored buffer set must serve the
composite phase and both backwards exactly as the set the geometry phase filled, and the step with
the cache on must compute what it computes with the cache off.

Shapes: 70 x 50 (5 x 4 tiles, partial edge tiles) and 17 x 33 (2 x 3), 1 to 1500 Gaussians: more
than one workgroup of the copy kernel, counts that are no multiple of 4 (the 16-byte words' tails).
"""
import pytest
import torch

from langsplat_amd import _native
from langsplat_amd.graph import ViewSlot
from langsplat_amd.pipeline import PipelinedGraphStep
from langsplat_amd.render import render
from langsplat_amd.synthetic import make_cameras, make_gaussians
from tests.scenes import POSES, grad_seed, posed_camera, scene, to_device
from tests.test_gpu_captured_forms import (_adam, _frozen_model, _slot_forward, _state, assert_states_close)
from tests.test_gpu_fused import _Opt, _Pipe
from tests.test_gpu_parity import assert_grad_close
from tests.test_gpu_timed_step import bench_target

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOMETRY, COMPOSITE = _native.forward_phase.GEOMETRY, _native.forward_phase.COMPOSITE
LANG_FLAGS = _native.FWD_ZERO_GRAD_RECORDS | _native.FWD_NO_COLOR_GRAD  # the language step's forward


# ---- the native round trip ---------------------------------------------------------------------------

class _Set:
    """One static buffer set with its overflow flag and fused-loss output."""

    def __init__(self):
        self.bufs = _native.static_buffers()
        self.overflow = torch.zeros((), dtype=torch.int32, device=DEV)
        self.loss = torch.zeros((), device=DEV)

    def tensor(self, which):
        return self.bufs.tensors[("scratch", which)]


class _Case:
    """A scene on the device, its capacities (from one eager forward) and its language target."""

    def __init__(self, st, inp, mode):
        self.st, self.inp = to_device(st, inp, DEV)
        self.mode = mode  # "language": the language step's backward; "all": every gradient
        self.P = int(self.inp["means3D"].shape[0])
        self.W, self.H = int(st.image_width), int(st.image_height)
        gt, mask = bench_target(self.H, self.W, 0)
        self.gt, self.mask = gt.to(DEV).contiguous(), mask.to(DEV).reshape(-1).contiguous()
        self.flags = LANG_FLAGS if mode == "language" else 0
        _native.LAST_COUNTS.clear()
        self._forward(None, 0)
        torch.cuda.synchronize()
        r, e = _native.LAST_COUNTS[(self.P, self.W, self.H)]
        self.counts = (r, e)
        self.cap = (r + 1024, e + 1024)
        self.lay = _native.state_layout(self.P, self.W, self.H, 0)
        self.gc, self.gl = (t.to(DEV) for t in grad_seed(self.H, self.W, seed=3))
        self.one = torch.ones((), device=DEV)

    def _forward(self, s, phase):
        i = self.inp
        args = (self.st, i["means3D"], i["shs"], None, i["language_feature_precomp"], i["opacities"], i["scales"],
                i["rotations"], None)
        if s is None:
            return _native.rasterize_gaussians(*args, flags=self.flags)
        with _native.capacity(*self.cap, s.overflow), s.bufs, _native.forward_phase(phase):
            return _native.rasterize_gaussians(*args, loss_target=self.gt, loss_mask=self.mask, out_loss=s.loss,
                                               flags=self.flags)

    def geometry(self, s):
        self._forward(s, GEOMETRY)

    def counters(self, s):
        off = self.lay["counters"]
        return s.tensor(_native.LSR_BUF_IMAGE)[off:off + 32].view(torch.int32).cpu()

    def records(self, s):
        off = self.lay["record"]
        return s.tensor(_native.LSR_BUF_GEOM)[off:off + 48 * self.P].view(torch.float32).view(self.P, 12)

    def composite(self, s):
        """The composite phase and the backward on set s -> (exact outputs, gradients)."""
        out = self._forward(s, COMPOSITE)
        nr, color, lang, radii, geom, binning, image = out
        HW = self.H * self.W
        exact = {"color": color.clone(), "language": lang.clone(), "loss": s.loss.clone(), "radii": radii.clone()}
        for name, dt in (("final_T", torch.float32), ("n_contrib", torch.int32)):
            exact[name] = image[self.lay[name]:self.lay[name] + 4 * HW].view(dt).clone()
        i = self.inp
        common = (self.st, i["means3D"], i["shs"], None, i["language_feature_precomp"], i["scales"], i["rotations"],
                  None, radii)
        if self.mode == "language":
            g = _native.rasterize_gaussians_backward(*common, None, None, nr, geom, binning, image,
                                                     opacities=i["opacities"], geometry=False, grad_loss=self.one,
                                                     flags=_native.BWD_RECORDS_ZEROED)
        else:
            g = _native.rasterize_gaussians_backward(*common, self.gc, self.gl, nr, geom, binning, image,
                                                     opacities=i["opacities"], geometry=True, grad_loss=self.one)
        return exact, {k: v.clone() for k, v in g.items() if v is not None}

    def pack_of(self, s):
        """Save set s -> (view args factory's inputs): the view's count from its counters, its pack."""
        cnt = self.counters(s)
        assert int(cnt[7]) == 0 and int(s.overflow.item()) == 0, "the view must fit its capacities"
        rendered = int(cnt[1])
        assert rendered == self.counts[0]
        pack = torch.empty((_native.view_pack_bytes(self.P, self.W, self.H, rendered),), dtype=torch.uint8, device=DEV)
        _native.view_save(_native.view_args(s.bufs, rendered, pack), torch.cuda.current_stream())
        return rendered, pack

    def restore(self, s, rendered, pack):
        _native.view_restore(_native.view_args(s.bufs, rendered, pack), torch.cuda.current_stream())


def _assert_same(case, a, b, tag):
    ea, ga = a
    eb, gb = b
    for k in ea:
        assert torch.equal(ea[k], eb[k]), f"{tag}: {k} differs"
    assert set(ga) == set(gb)
    for k in ga:
        assert_grad_close(f"{tag} {k}", gb[k].cpu().numpy(), ga[k].cpu().numpy())


def _blank(case, s, seed):
    """Every byte of set s to 0xFF (its overflow flag set), then known values in its language slots."""
    for which in (_native.LSR_BUF_GEOM, _native.LSR_BUF_IMAGE, _native.LSR_BUF_BINNING):
        s.tensor(which).fill_(0xFF)
    s.bufs.tensors[("out", "radii")].fill_(-1)
    s.overflow.fill_(0x3F800000)
    slots = torch.randn((case.P, 3), generator=torch.Generator().manual_seed(seed)).to(DEV)
    case.records(s)[:, 9:12] = slots
    return slots


def _round_trip(case, tag):
    A, B = _Set(), _Set()
    case.geometry(A)
    ref = case.composite(A)
    # saved as the step saves it: after the composite and the backward have used the set
    rendered, pack = case.pack_of(A)
    case.geometry(B)  # (allocates B at the capacity sizes)
    slots = _blank(case, B, seed=11)
    case.restore(B, rendered, pack)
    assert torch.equal(case.records(B)[:, 9:12], slots), f"{tag}: the restore touched the language slots"
    assert int(B.overflow.item()) == 0
    cb, ca = case.counters(B), case.counters(A)
    assert int(cb[7]) == 0 and [int(cb[i]) for i in (1, 2, 4, 5, 6)] == [int(ca[i]) for i in (1, 2, 4, 5, 6)]
    got = case.composite(B)
    _assert_same(case, ref, got, tag)
    return ref, A, rendered, pack


@pytest.mark.parametrize("mode", ["language", "all"])
@pytest.mark.parametrize("W,H,P", [(70, 50, 1501), (17, 33, 302)])
def test_native_round_trip(mode, W, H, P):
    """Geometry into set A, saved after its composite and backward; set B filled with 0xFF and known
    language slots, restored: composite + backward on B equal A's (images, loss, radii, final_T,
    n_contrib bit for bit; gradients within the atomics' tolerance), the slots untouched."""
    st, inp = scene(P=P, W=W, H=H, seed=4, scale_range=(0.03, 0.2))
    case = _Case(st, inp, mode)
    ref, *_ = _round_trip(case, f"{mode} {W}x{H}")
    assert case.counts[0] > 0 and float(ref[0]["loss"]) > 0
    assert any(float(v.abs().sum()) > 0 for v in ref[1].values())


@pytest.mark.parametrize("mode", ["language", "all"])
def test_restore_reinitialises(mode):
    """Two composite + backward passes on ONE set with a restore between them: the same loss bits and
    images the second time (stale loss words, work-class counters or forward flags would show)."""
    st, inp = scene(P=1501, W=70, H=50, seed=5, scale_range=(0.03, 0.2))
    case = _Case(st, inp, mode)
    A = _Set()
    case.geometry(A)
    first = case.composite(A)
    rendered, pack = case.pack_of(A)
    case.restore(A, rendered, pack)
    second = case.composite(A)
    _assert_same(case, first, second, f"{mode} second pass")
    # ... and a third after another restore, the set's counters as the second pass left them
    case.restore(A, rendered, pack)
    _assert_same(case, first, case.composite(A), f"{mode} third pass")
    # another target: loss words left over from the passes above would hold the old target's shares
    # (the last workgroup adds whatever words are already flagged), a fresh set's are cleared
    case.gt = torch.nn.functional.normalize(bench_target(case.H, case.W, 5)[0], dim=0).to(DEV).contiguous().neg()
    case.restore(A, rendered, pack)
    fourth = case.composite(A)
    C = _Set()
    case.geometry(C)
    _assert_same(case, case.composite(C), fourth, f"{mode} another target")
    assert not torch.equal(fourth[0]["loss"], first[0]["loss"])


def _edge_case(name, mode):
    W, H = 70, 50
    if name == "nothing":  # the camera looks away from the cube
        cam = posed_camera((0.0, 0.0, -3.0), (0.0, 0.0, -6.0), 0.0, W, H)
        st, inp = scene(P=303, W=W, H=H, seed=6, cam=cam)
    elif name == "one":
        st, inp = scene(P=1, W=W, H=H, seed=6, scale_range=(0.2, 0.3), extent=0.1)
    else:
        pos, target, roll = POSES[name]
        st, inp = scene(P=1203, W=W, H=H, seed=6, cam=posed_camera(pos, target, roll, W, H),
                        scale_range=(0.03, 0.3))
    return _Case(st, inp, mode)


@pytest.mark.parametrize("mode", ["language", "all"])
@pytest.mark.parametrize("name", ["nothing", "one", "inside", "rolled"])
def test_edge_views(name, mode):
    case = _edge_case(name, mode)
    if name == "nothing":
        assert case.counts[0] == 0
    else:
        assert case.counts[0] > 0
    _round_trip(case, f"{name} {mode}")


def test_invalid_arguments_on_device_buffers():
    """The checks that need real buffers: num_rendered over capacity, a short pack, a misaligned pack."""
    st, inp = scene(P=302, W=17, H=33, seed=4)
    case = _Case(st, inp, "language")
    A = _Set()
    case.geometry(A)
    torch.cuda.synchronize()
    rendered = case.counts[0]
    pack = torch.empty((_native.view_pack_bytes(case.P, case.W, case.H, rendered) + 16,), dtype=torch.uint8, device=DEV)
    lib = _native.load()
    import ctypes
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn in (lib.lsr_view_save, lib.lsr_view_restore):
        a = _native.view_args(A.bufs, rendered, pack)
        a.num_rendered = a.capacity_rendered + 1
        assert fn(ctypes.byref(a), stream) == 1
        a = _native.view_args(A.bufs, rendered, pack)
        a.pack_bytes = _native.view_pack_bytes(case.P, case.W, case.H, rendered) - 1
        assert fn(ctypes.byref(a), stream) == 1
        a = _native.view_args(A.bufs, rendered, pack)
        a.pack = a.pack + 4
        assert fn(ctypes.byref(a), stream) == 1
        a = _native.view_args(A.bufs, rendered, pack)
        a.geom = None
        assert fn(ctypes.byref(a), stream) == 1
    torch.cuda.synchronize()


# ---- the step ------------------------------------------------------------------------------------------

W_, H_ = 70, 50
SEQ = [0, 1, 2, 0, 2, 1, 1, 0, 2, 0, 1, 2]  # 12 steps over 3 views, with repeats


def _views(n=3):
    cams = make_cameras(n, W_, H_, device=DEV)
    out = []
    for v in range(n):
        gt, mask = bench_target(H_, W_, v)
        out.append((cams[v], gt.to(DEV), mask.to(DEV)))
    return out


def _gaussians():
    return make_gaussians(1500, seed=2, scale_range=(0.03, 0.2))


def _run_slots(g, views, seq, sets, wait, edit_at=None, capture_caps=(0, 0), **kw):
    """A PipelinedGraphStep with slots over views[seq] -> (losses, state, step)."""
    m = _frozen_model(g)
    opt = _adam(m)
    slots = [ViewSlot(*views[seq[0]]) for _ in range(sets)]
    pg = PipelinedGraphStep(_slot_forward(m), [m._language_feature], opt, slots=slots, model=m, **kw)
    pg.capture(*capture_caps, views=[views[v] for v in seq[:sets - 1]])
    L = sets - 1
    losses = []
    for k in range(len(seq)):
        if edit_at is not None and k == edit_at:
            pg.synchronize()
            torch.cuda.synchronize()
            with torch.no_grad():
                m._xyz.mul_(1.01)  # an in-place edit of a frozen geometry tensor
        nxt = views[seq[k + L]] if k + L < len(seq) else None
        # (synchronised every step, so a set's counters have always arrived at its next visit and the
        # expected hit counts are exact)
        losses.append(pg.replay(next_view=nxt, wait=wait))
        pg.synchronize()
        torch.cuda.synchronize()
        losses[-1] = losses[-1].clone()
    assert pg.check()
    pg.sync()
    return torch.stack(losses), _state(m, opt), pg


@pytest.mark.parametrize("sets,wait", [(2, True), (3, True), (2, False), (3, False)])
def test_step_with_slots_matches_uncached(sets, wait, monkeypatch):
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g, views = _gaussians(), _views()
    l0, s0, pg0 = _run_slots(g, views, SEQ, sets, wait, view_cache=False)
    assert pg0.view_cache_stats() == {"hits": 0, "misses": 0, "packs": 0, "bytes": 0, "drops": 0}
    l1, s1, pg1 = _run_slots(g, views, SEQ, sets, wait)
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=0)
    assert_states_close(s1, s0, f"view cache, {sets} sets, wait={wait}")
    st = pg1.view_cache_stats()
    # every geometry (S - 1 at the priming, one per replay) is a hit or a miss; each view misses until
    # it was saved once (when its set was next released), so all three views end up cached
    assert st["hits"] + st["misses"] == len(SEQ) + sets - 1 and st["packs"] == 3 and st["hits"] >= 4, st
    assert st["bytes"] == sum(v[3] for v in pg1._views.packs.values()) > 0
    assert pg1.captures == 1


def test_fixed_view_hits_from_the_second_visit(monkeypatch):
    """No slots: one constant key; the first replay that finds a set's counters arrived saves it and
    every later replay restores."""
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
        for _ in range(8):
            losses.append(pg.replay().clone())
            torch.cuda.synchronize()
        assert pg.check()
        pg.sync()
        return torch.stack(losses), _state(m, opt), pg

    l0, s0, _ = run(view_cache=False)
    l1, s1, pg = run()
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=0)
    assert_states_close(s1, s0, "fixed view")
    st = pg.view_cache_stats()
    # 3 sets: 2 primed + 8 replays = 10 geometries; set 0 is released at the second replay, saved, and
    # everything from then on restores
    assert st["packs"] == 1 and st["misses"] == 3 and st["hits"] == 7, st


def test_inplace_edit_drops_the_packs(monkeypatch):
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g, views = _gaussians(), _views()
    l0, s0, _ = _run_slots(g, views, SEQ, 3, True, edit_at=7, view_cache=False)
    l1, s1, pg = _run_slots(g, views, SEQ, 3, True, edit_at=7)
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=0)
    assert_states_close(s1, s0, "in-place edit")
    st = pg.view_cache_stats()
    assert st["drops"] == 1 and st["hits"] >= 2, st
    # without the edit the same sequence gives other losses: the edit did reach the replays
    l2, _, _ = _run_slots(g, views, SEQ, 3, True, view_cache=False)
    assert not torch.allclose(l2[-2:], l0[-2:], rtol=1e-5, atol=0)


def test_budget_and_gates(monkeypatch):
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g, views = _gaussians(), _views()
    l0, s0, _ = _run_slots(g, views, SEQ, 3, True, view_cache=False)
    # a budget of zero behaves as off
    l1, s1, pg = _run_slots(g, views, SEQ, 3, True, view_cache_bytes=0)
    assert pg._views is None and pg.view_cache_stats()["hits"] == 0
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=0)
    # a budget of one pack caches one view and recomputes the rest
    one = max(_native.view_pack_bytes(1500, W_, H_, r) for r in (pg.rendered,))
    l2, s2, pg = _run_slots(g, views, SEQ, 3, True, view_cache_bytes=one)
    st = pg.view_cache_stats()
    assert st["packs"] == 1 and st["hits"] >= 1 and st["misses"] > 3 and st["bytes"] <= one, st
    torch.testing.assert_close(l2, l0, rtol=1e-5, atol=0)
    assert_states_close(s2, s0, "budget of one pack")
    # a trainable geometry tensor, or no model: inactive
    m = _frozen_model(g)
    m._opacity.requires_grad_(True)
    slots = [ViewSlot(*views[0]) for _ in range(3)]
    pg = PipelinedGraphStep(_slot_forward(m), [m._language_feature], _adam(m), slots=slots, model=m)
    pg.capture(views=views[:2])
    assert pg._views is None
    m = _frozen_model(g)
    slots = [ViewSlot(*views[0]) for _ in range(3)]
    pg = PipelinedGraphStep(_slot_forward(m), [m._language_feature], _adam(m), slots=slots)
    pg.capture(views=views[:2])
    assert pg._views is None


def test_overflowed_view_is_never_cached_and_recapture_refills(monkeypatch):
    """Capacities that only the first view fits: the larger view overflows, is skipped and is not
    saved; check() re-captures with doubled capacities, the cache starts empty and fills again."""
    monkeypatch.setenv("LANGSPLAT_AMD_FUSED", "1")
    g = _gaussians()
    far = make_cameras(1, W_, H_, radius=12.0, device=DEV)[0]
    near = make_cameras(1, W_, H_, radius=2.0, device=DEV)[0]
    views = []
    for v, cam in enumerate((far, near)):
        gt, mask = bench_target(H_, W_, v)
        views.append((cam, gt.to(DEV), mask.to(DEV)))
    m = _frozen_model(g)
    opt = _adam(m)
    slots = [ViewSlot(*views[0]) for _ in range(3)]
    pg = PipelinedGraphStep(_slot_forward(m), [m._language_feature], opt, slots=slots, model=m, headroom=1.0)
    pg.capture(views=[views[0], views[0]])  # measured on the far view only
    seq = [0, 0, 1, 0, 1, 0, 1, 0]
    for k in range(len(seq)):
        nxt = views[seq[k + 2]] if k + 2 < len(seq) else None
        pg.replay(next_view=nxt)
        pg.synchronize()
        torch.cuda.synchronize()
    st = pg.view_cache_stats()
    assert st["packs"] == 1 and id(near) not in pg._views.packs, st  # the near view overflowed every time
    assert not pg.check() and pg.captures == 2
    assert pg.view_cache_stats() == {"hits": 0, "misses": 0, "packs": 0, "bytes": 0, "drops": 0}
    for _ in range(4):  # (each failed check doubles the capacities again)
        for k in range(6):
            pg.replay(next_view=views[k % 2])
            pg.synchronize()
            torch.cuda.synchronize()
        if pg.check():
            break
    else:
        raise AssertionError("the near view still overflows")
    st = pg.view_cache_stats()
    assert st["packs"] == 2 and st["hits"] >= 1, st
