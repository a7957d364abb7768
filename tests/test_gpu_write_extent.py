"""What the kernels write OUTSIDE the buffers the ABI sizes, and what they read of scratch nobody
initialised (tests/guards.py).

Every case has one shape: the operation once on plain tensors for the reference result, then twice
with every output and scratch buffer a Guarded of exactly the size include/lsr.h gives it, the
interiors filled with 0x00 and with 0xFF.  Asserted: every guard byte intact; every output the header
documents as fully written holds no fill pattern (under 0xFF); the two guarded results and the plain
one equal -- forward results bit for bit, gradients (float atomics) with test_gpu_parity's
assert_grad_close.  A difference between the two fills is a read of uninitialised memory.  Buffers
with a documented initial state (in/out tensors, the masked-L1 scratch: zeroed once) get that state
and are still guarded.  Each case first asserts that it reached the path it is there for.
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from langsplat_amd import _native, knn, loss as loss_module
from langsplat_amd.distributed import GradBucket
from langsplat_amd.synthetic import make_cameras
from oracle import oracle
from tests import guards
from tests.guards import Guarded, GuardedBuffers, guarded_allocations
from tests.scenes import EDGE_SCENES, edge_scene, grad_seed, posed_scene, scene, settings_for, to_device
from tests.test_gpu_binning import dense_bucket_scene, strip_scene
from tests.test_gpu_fused import _raw_scene
from tests.test_gpu_levels import level_features
from tests.test_gpu_parity import assert_grad_close, native_forward, state

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (0x00, 0xFF)
GEOM, BINNING, IMAGE, BACKWARD, LEVELS = (("scratch", w) for w in range(5))
TH, TW = _native.RGB_LOSS_TILE


def _sync():
    torch.cuda.synchronize()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def unwritten(t, fill=0xFF):
    """Elements of the contiguous tensor t whose every byte is still the fill byte."""
    if t.numel() == 0:
        return 0
    return int((t.reshape(-1).view(torch.uint8).view(-1, t.element_size()) == fill).all(dim=1).sum())


def holding(src, fill, misalign=0, name=None):
    """A Guarded holding a copy of src: an in/out tensor, or an input whose alignment the case sets."""
    g = Guarded(tuple(src.shape), src.dtype, DEV, fill=fill, misalign=misalign, name=name)
    g.tensor.copy_(src)
    return g


def plain(src, misalign=0):
    """A plain copy of src, `misalign` bytes off torch's allocation alignment."""
    k = misalign // src.element_size()
    buf = torch.empty((src.numel() + k,), dtype=src.dtype, device=DEV)
    out = buf[k:].view(src.shape)
    out.copy_(src)
    assert out.data_ptr() % 16 == misalign % 16
    return out


def check(*gs):
    for g in gs:
        g.check()


def reset_binning_hint():
    """The eager forward asks for its binning buffer before the host wait at the size this thread's last
    forward of the same P and image size needed, plus 12.5 %; a forward of another size in between makes
    the next one ask once, after the wait, for exactly what its view needs."""
    native_forward(*scene(P=2, W=8, H=8, seed=0))


# ---- the rasterizer forward and backward ---------------------------------------------------------------

VARIANTS = ("full", "no_colour", "language", "language+colour")


def activated_case(st, inp, variants=None):
    std, ind = to_device(st, inp, DEV)
    inc = bool(st.include_feature)
    f = dict(means3D=ind["means3D"], shs=ind.get("shs"), colors_precomp=ind.get("colors_precomp"),
             language_feature=ind.get("language_feature_precomp") if inc else None, opacities=ind["opacities"],
             scales=ind.get("scales"), rotations=ind.get("rotations"), cov3D_precomp=ind.get("cov3D_precomp"))
    P = int(inp["means3D"].shape[0])
    if variants is None:
        variants = VARIANTS if inc and P > 0 else ("full",)
    return SimpleNamespace(st=std, f=f, kw={}, inc=inc, P=P, W=int(st.image_width), H=int(st.image_height),
                           variants=variants)


def raw_case(P, W, H, seed, sh_degree):
    """The fused raw path (test_gpu_fused's builder): GaussianModel's raw parameters, features_dc / _rest."""
    g, st = _raw_scene(P, W, H, seed, sh_degree)
    std, _ = to_device(st, {}, DEV)
    gd = g.to(DEV)
    f = dict(means3D=gd.xyz, shs=gd.features_dc.contiguous(), colors_precomp=None, language_feature=gd.language_feature,
             opacities=gd.opacity, scales=gd.scaling, rotations=gd.rotation, cov3D_precomp=None)
    raw = _native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS | _native.RAW_LANGUAGE
    return SimpleNamespace(st=std, f=f, kw=dict(raw=raw, shs_rest=gd.features_rest.contiguous()), inc=True, P=P, W=W,
                           H=H, variants=VARIANTS)


def forward(c, **kw):
    f = c.f
    return _native.rasterize_gaussians(c.st, f["means3D"], f["shs"], f["colors_precomp"], f["language_feature"],
                                       f["opacities"], f["scales"], f["rotations"], f["cov3D_precomp"], **c.kw, **kw)


def backward(c, out, variant, seeds, **kw):
    nr, color, lang, radii, geom, binning, image = out
    gc, gl = seeds
    f = c.f
    return _native.rasterize_gaussians_backward(
        c.st, f["means3D"], f["shs"], f["colors_precomp"], f["language_feature"], f["scales"], f["rotations"],
        f["cov3D_precomp"], radii, gc if variant in ("full", "language+colour") else None, gl if c.inc else None, nr,
        geom, binning, image, opacities=f["opacities"], geometry=variant in ("full", "no_colour"), **c.kw, **kw)


def run_raster(c, seeds, fwd_kw=None):
    out = forward(c, **(fwd_kw or {}))
    _sync()
    grads = {v: backward(c, out, v, seeds) for v in c.variants}
    _sync()
    return out, grads


def assert_same_forward(c, ref, out, tag, with_state=True):
    assert out[0] == ref[0], tag
    for name, a, b in zip(("color", "language", "radii"), ref[1:4], out[1:4]):
        assert torch.equal(a, b), f"{tag}: {name} differs"
    if not with_state or c.P == 0 or ref[0] == 0:
        return
    sr, so = state(ref, c.P, c.W, c.H), state(out, c.P, c.W, c.H)
    full = sr["ranges"][:, 1] > sr["ranges"][:, 0]
    np.testing.assert_array_equal(so["ranges"][full], sr["ranges"][full], err_msg=f"{tag}: ranges")
    assert np.all(so["ranges"][~full, 1] == so["ranges"][~full, 0]), f"{tag}: an empty tile is not empty"
    for k in ("point_list", "final_T", "n_contrib", "depth_key", "counters"):
        np.testing.assert_array_equal(so[k], sr[k], err_msg=f"{tag}: {k}")


def assert_same_grads(ref, got, tag, fill, rec=None):
    for v in ref:
        for name, r in ref[v].items():
            g = got[v][name]
            assert (r is None) == (g is None), f"{tag} {v}: {name}"
            if r is None:
                continue
            assert bool(torch.isfinite(g).all()), f"{tag} {v}: {name} is not finite"
            if fill == 0xFF:
                assert unwritten(g) == 0, f"{tag} {v}: {name} was not fully written"
            assert_grad_close(f"{tag} {v} {name}", g.cpu().numpy(), r.cpu().numpy())
        if rec is not None:  # the 256-byte aligned views of one allocation: the gaps between them are guards too
            rec.of(got[v]["means2D"]).assert_only_written(list(got[v].values()), f"{tag} {v}: flat")


def guarded_raster(c, ref, tag, monkeypatch, path=None, fwd_kw=None, seed=7):
    """The case's forward and its backward variants under both fills against `ref`, the plain run."""
    seeds = tuple(t.to(DEV) for t in grad_seed(c.H, c.W, seed=seed))
    ref_out, ref_grads = ref
    for v in ref_grads:
        for name, r in ref_grads[v].items():
            assert r is None or bool(torch.isfinite(r).all()), f"{tag} {v}: plain {name} is not finite"
    for fill in FILLS:
        t = f"{tag} fill {fill:#04x}"
        reset_binning_hint()
        gb = GuardedBuffers(fill)
        with gb, guarded_allocations(monkeypatch, _native, fill) as rec:
            out, grads = run_raster(c, seeds, fwd_kw)
        gb.check_all()
        rec.check_all()
        R, E = _native.LAST_COUNTS[(c.P, c.W, c.H)]
        assert R == out[0]
        gb.assert_abi_sizes(c.P, c.W, c.H, out[0], E)
        if c.P > 0:  # one request, after the wait, for exactly what the view needs (reset_binning_hint)
            assert [k for k, _ in gb.requests].count(BINNING) == 1, t
        if path is not None:
            path(out, gb)
        if fill == 0xFF:
            for key in ("color", "language", "radii"):
                assert gb.guards[("out", key)].unwritten() == 0, f"{t}: {key} was not fully written"
        assert_same_forward(c, ref_out, out, t)
        assert_same_grads(ref_grads, grads, t, fill, rec)


def plain_raster(c, seed=7, fwd_kw=None):
    seeds = tuple(t.to(DEV) for t in grad_seed(c.H, c.W, seed=seed))
    return run_raster(c, seeds, fwd_kw)


def _precomp_scene():
    """test_gpu_parity's colors_precomp + cov3D_precomp path."""
    st, inp = scene(P=400, W=64, H=48, seed=11, sh_degree=3, scale_range=(0.03, 0.2))
    run0 = oracle.forward(st, **inp)
    inp2 = dict(inp)
    del inp2["shs"], inp2["scales"], inp2["rotations"]
    inp2["colors_precomp"] = torch.tensor(run0.get("rgb")).clone()
    inp2["cov3D_precomp"] = torch.tensor(oracle.cov3d(inp["scales"].numpy(), 1.0, inp["rotations"].numpy()))
    return st, inp2


def _edge(name):
    _, st, inp = edge_scene(**EDGE_SCENES[name])
    return st, inp


FORWARD_SCENES = {
    "300_64x48": lambda: scene(P=300, W=64, H=48, seed=0),
    "500_67x45_sh2_bg": lambda: scene(P=500, W=67, H=45, seed=1, sh_degree=2, bg=(0.2, 0.5, 0.9),
                                      scale_range=(0.03, 0.2)),
    "400_48x40_sh1_no_feature": lambda: scene(P=400, W=48, H=40, seed=2, sh_degree=1, include_feature=False,
                                              scale_range=(0.03, 0.2)),
    "tiny_1x1": lambda: posed_scene("inside", 200, 1, 1, 6, sh_degree=3, scale_range=(0.03, 0.2), bg=(0.3, 0.1, 0.7)),
    "tiny_7x5": lambda: posed_scene("inside", 200, 7, 5, 6, sh_degree=3, scale_range=(0.03, 0.2), bg=(0.3, 0.1, 0.7)),
    "tiny_16x16": lambda: posed_scene("inside", 200, 16, 16, 6, sh_degree=3, scale_range=(0.03, 0.2),
                                      bg=(0.3, 0.1, 0.7)),
    "tiny_17x33": lambda: posed_scene("inside", 200, 17, 33, 6, sh_degree=3, scale_range=(0.03, 0.2),
                                      bg=(0.3, 0.1, 0.7)),
    "one_gaussian": lambda: scene(P=1, W=64, H=48, seed=6, scale_range=(0.2, 0.3), extent=0.1),
    "edge_A": lambda: _edge("A"),
    "edge_C": lambda: _edge("C"),
    "precomp": _precomp_scene,
}


@pytest.mark.parametrize("name", sorted(FORWARD_SCENES))
def test_rasterizer_forward_and_backward(name, monkeypatch):
    c = activated_case(*FORWARD_SCENES[name]())
    ref = plain_raster(c)
    assert ref[0][0] > 0, "the scene draws nothing"
    if name == "precomp":
        assert c.f["shs"] is None and c.f["scales"] is None and ref[1]["full"]["cov3D_precomp"] is not None
    guarded_raster(c, ref, name, monkeypatch)


def test_rasterizer_fused_raw_path(monkeypatch):
    """P = 501, SH degree 3: the last block of 117 Gaussians stages 5265 features_rest floats, a float4
    run plus a one-float tail."""
    c = raw_case(501, 64, 48, 5, 3)
    assert (501 % 128) * 45 % 4 == 1 and c.kw["shs_rest"].data_ptr() % 16 == 0
    ref = plain_raster(c)
    assert ref[0][0] > 0 and ref[1]["full"]["shs_rest"] is not None
    guarded_raster(c, ref, "fused raw", monkeypatch)


@pytest.mark.parametrize("W,H", [(5, 3), (67, 45)])
@pytest.mark.parametrize("kind", ["empty", "culled"])
def test_rasterizer_empty_and_fully_culled(kind, W, H, monkeypatch):
    """P = 0 zero-fills the caller's images (3 H W 4 bytes: no multiple of 16, the fill's byte tail); a
    scene behind the near plane composites the background over empty tiles."""
    st, inp = scene(P=50, W=W, H=H, seed=0, bg=(0.3, 0.3, 0.3))
    if kind == "empty":
        inp = {k: v[:0] for k, v in inp.items()}
    else:
        inp = dict(inp, means3D=inp["means3D"] * 0.01 + torch.tensor([0.0, 0.0, -3.9]))
    c = activated_case(st, inp, variants=("full", "language") if kind == "empty" else VARIANTS)
    assert (3 * H * W * 4) % 16 != 0
    ref = plain_raster(c)
    assert ref[0][0] == 0 and not ref[0][2].any()
    assert torch.equal(ref[0][1], torch.full((3, H, W), 0.0 if kind == "empty" else 0.3, device=DEV))

    def path(out, gb):
        assert (gb.requested(GEOM) is None) == (kind == "empty")

    guarded_raster(c, ref, f"{kind} {W}x{H}", monkeypatch, path=path)


@pytest.mark.parametrize("W,H", [(5, 3), (67, 45)])
@pytest.mark.parametrize("misalign", [0, 4, 8, 12])
def test_zero_fill_of_caller_outputs_at_every_alignment(misalign, W, H):
    """lsr_forward with P = 0 on images that start 0, 4, 8 and 12 bytes past a 16-byte boundary:
    zero_fill's byte head, its 16-byte body and its byte tail, on memory the caller owns."""
    st, _ = scene(P=1, W=W, H=H, seed=0)
    std, _ = to_device(st, {}, DEV)
    keep = []
    s = _native.make_settings(std, keep)
    n = 3 * H * W * 4
    head = (16 - misalign) % 16
    assert (n - head) // 16 > 0 and (head != 0 or (n - head) % 16 != 0)  # a body, and a head or a tail beside it
    for fill in FILLS:
        color = Guarded((3, H, W), torch.float32, DEV, fill=fill, misalign=misalign, name="out_color")
        lang = Guarded((3, H, W), torch.float32, DEV, fill=fill, misalign=misalign, name="out_language_feature")
        assert color.tensor.data_ptr() % 16 == misalign
        a = _native.LsrForwardArgs()
        a.P = 0
        a.out_color, a.out_language_feature = color.tensor.data_ptr(), lang.tensor.data_ptr()
        nr = ctypes.c_int64(-1)
        with _native._Allocator(torch.device(DEV)):
            _native._check(_native.load().lsr_forward(ctypes.byref(s), ctypes.byref(a), _native._ALLOC_CB, None,
                                                      _stream(), ctypes.byref(nr)), "lsr_forward")
        _sync()
        check(color, lang)
        assert nr.value == 0 and not color.tensor.any() and not lang.tensor.any()
        if fill == 0xFF:
            assert color.unwritten() == 0 and lang.unwritten() == 0


def _over_capacity_scene():
    """test_gpu_binning.test_fused_emission_over_capacity's scene: E > 3 P on a 1280x720 image."""
    P, W, H = 300, 1280, 720
    g = torch.Generator().manual_seed(41)
    cam = make_cameras(1, W, H)[0]
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    d = 3.0 + torch.rand(P, generator=g) * 2.0
    u, v = torch.rand(P, generator=g) * 2 - 1, torch.rand(P, generator=g) * 2 - 1
    means = torch.stack([u * d * tx * 0.8, v * d * ty * 0.8, d - 4.0], 1)
    inp = dict(means3D=means, opacities=torch.rand((P, 1), generator=g) * 0.3 + 0.05,
               colors_precomp=torch.rand((P, 3), generator=g),
               language_feature_precomp=torch.nn.functional.normalize(torch.randn((P, 3), generator=g)),
               scales=0.15 + 0.15 * torch.rand((P, 3), generator=g),
               rotations=torch.nn.functional.normalize(torch.randn((P, 4), generator=g)))
    return settings_for(cam, sh_degree=0), inp


@pytest.mark.parametrize("buckets", ["256", "512"])
def test_rasterizer_fused_emission_over_capacity(buckets, monkeypatch):
    """kFusedEntries = 3 entries per Gaussian: a view with E > 3 P emits nothing into the fixed arrays
    and takes the unfused depth order and k_emit_super after the host wait."""
    monkeypatch.setenv("LSR_MSD_BUCKETS", buckets)
    c = activated_case(*_over_capacity_scene())
    ref = plain_raster(c)
    assert state(ref[0], c.P, c.W, c.H)["counters"][4] > 3 * c.P

    def path(out, gb):
        assert state(out, c.P, c.W, c.H)["counters"][4] > 3 * c.P

    guarded_raster(c, ref, f"over capacity, {buckets} buckets", monkeypatch, path=path)


@pytest.mark.parametrize("placed", ["1", "0"])
def test_rasterizer_dense_bucket(placed, monkeypatch):
    """kBucketCap = 8192: one depth bucket with more entries than an LDS list, within the fused capacity,
    with placed and with depth-order emission."""
    monkeypatch.setenv("LSR_PLACED", placed)
    c = activated_case(*dense_bucket_scene())
    ref = plain_raster(c)
    E = int(state(ref[0], c.P, c.W, c.H)["counters"][4])
    assert 7000 + 8192 < E <= 3 * c.P
    guarded_raster(c, ref, f"dense bucket, placed {placed}", monkeypatch)


def test_rasterizer_two_pass_super_tile_sort(monkeypatch):
    """33000 x 64: 258 super-tiles, one more than a single 8-bit radix pass orders."""
    W, H = 33000, 64
    c = activated_case(*strip_scene(3000, W, H, seed=W + H))
    assert (((W + 15) // 16 + 7) // 8) * (((H + 15) // 16 + 7) // 8) == 258
    ref = plain_raster(c)
    assert ref[0][0] > 0
    guarded_raster(c, ref, "strip", monkeypatch)


# ---- capacity mode ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("short", ["exact", "rendered", "entries"])
def test_capacity_mode_stays_inside_capacity_sized_buffers(short, monkeypatch):
    """test_gpu_graph.test_capacity_overflow_is_flagged_and_safe's scene with the buffers sized for the
    capacity while the view holds more: here an unguarded store is a heap overflow.  Capacities exactly
    (R, E), then (R // 2, E) and (R, E // 2); each scratch buffer's back pad also holds the difference to
    the full-size buffer, so even an unchecked write of the whole view lands in owned memory.  The
    language-step and the full backward then run over the overflowed state, as a captured replay does."""
    P, W, H = 4000, 128, 96
    st, inp = scene(P=P, W=W, H=H, seed=6, scale_range=(0.03, 0.2), bg=(0.25, 0.5, 0.75))
    c = activated_case(st, inp, variants=("language", "full"))
    seeds = tuple(t.to(DEV) for t in grad_seed(H, W, seed=5))
    eager, eager_grads = run_raster(c, seeds)
    R, E = _native.LAST_COUNTS[(P, W, H)]
    assert R == eager[0] and 0 < E <= R
    cap = {"exact": (R, E), "rendered": (R // 2, E), "entries": (R, E // 2)}[short]
    lib = _native.load()
    full = int(lib.lsr_binning_bytes(W, H, R))
    bg = torch.tensor([0.25, 0.5, 0.75], device=DEV).view(3, 1, 1).expand(3, H, W)
    for fill in FILLS:
        t = f"capacity {cap} fill {fill:#04x}"
        gb = GuardedBuffers(fill, extra_back={GEOM: full, BINNING: full, IMAGE: full, BACKWARD: full})
        ovf = torch.full((), 7, dtype=torch.int32, device=DEV)
        with gb, guarded_allocations(monkeypatch, _native, fill) as rec, _native.capacity(*cap, ovf):
            out, grads = run_raster(c, seeds)
        gb.check_all()
        rec.check_all()
        gb.assert_abi_sizes(P, W, H, cap[0], cap[1])
        small = gb.requested(BINNING)
        assert gb.guards[BINNING].back_pad >= guards.default_pad(small) + max(full - small, 0)
        assert out[0] == cap[0]
        if fill == 0xFF:
            for key in ("color", "language", "radii"):
                assert gb.guards[("out", key)].unwritten() == 0, f"{t}: {key} was not fully written"
        assert torch.equal(out[3], eager[3]), t
        if short == "exact":
            assert int(ovf.item()) == 0
            assert small <= full
            for a, b in zip(eager[1:3], out[1:3]):
                assert torch.equal(a, b), t
            se, sc = state(eager, P, W, H), state(out, P, W, H)
            for k in ("ranges", "final_T", "n_contrib", "point_list"):
                np.testing.assert_array_equal(se[k], sc[k], err_msg=f"{t}: {k}")
            assert_same_grads(eager_grads, grads, t, fill, rec)
        else:
            assert ovf.view(torch.float32).item() == 1.0  # the bits of 1.0f (include/lsr.h)
            assert small < full  # the path: buffers smaller than the view needs
            assert torch.equal(out[1], bg) and not out[2].any(), t
            assert not state(out, P, W, H)["n_contrib"].any(), t
            for v in grads:
                for name, g in grads[v].items():
                    assert g is None or not g.any(), f"{t} {v}: {name} is not zero"
                    assert g is None or fill != 0xFF or unwritten(g) == 0
                rec.of(grads[v]["means2D"]).assert_only_written(list(grads[v].values()), f"{t} {v}: flat")


# ---- view packs ------------------------------------------------------------------------------------------

def _view_modules():
    from tests import test_gpu_view_bind as vb, test_gpu_view_cache as vc, test_gpu_view_plan as vp
    return vc, vb, vp


class _GuardedSet:
    """test_gpu_view_cache._Set over GuardedBuffers."""

    def __init__(self, fill, bound=False):
        self.bufs = GuardedBuffers(fill)
        self.bufs.view_bind = bound
        self.overflow = torch.zeros((), dtype=torch.int32, device=DEV)
        self.loss = torch.zeros((), device=DEV)

    def tensor(self, which):
        return self.bufs.tensors[("scratch", which)]

    def blank(self):
        """Every buffer of the set back to its fill byte (what the geometry call left is gone)."""
        for g in self.bufs.guards.values():
            g.refill()
        self.overflow.fill_(0x3F800000)


def _assert_same_view(case, ref, got, tag):
    """test_gpu_view_cache._assert_same, and every gradient finite (a NaN passes a tolerance test)."""
    vc, _, _ = _view_modules()
    for k, g in got[1].items():
        assert bool(torch.isfinite(g).all()), f"{tag}: {k} is not finite"
    vc._assert_same(case, ref, got, tag)


def _view_case(name, mode):
    vc, _, _ = _view_modules()
    if name in ("nothing", "one"):
        return vc._edge_case(name, mode)
    W, H, P = {"17x33": (17, 33, 302), "70x50": (70, 50, 1501)}[name]
    return vc._Case(*scene(P=P, W=W, H=H, seed=4, scale_range=(0.03, 0.2)), mode)


@pytest.mark.parametrize("mode", ["language", "all"])
@pytest.mark.parametrize("name", ["17x33", "70x50", "nothing", "one"])
def test_view_packs(name, mode, monkeypatch):
    """lsr_view_save into packs of exactly lsr_view_pack_bytes / lsr_view_plan_pack_bytes, lsr_view_restore
    into a blanked set, the cover masks of a bound set's first compositing saved into a plan pack, and
    lsr_view_bind of two blanked sets to that one pack: every composite + backward equals the plain
    set's, the packs' and every set's guards intact."""
    vc, vb, vp = _view_modules()
    case = _view_case(name, mode)
    R = case.counts[0]
    assert (R == 0) == (name == "nothing")
    A0 = vc._Set()
    case.geometry(A0)
    ref = vb._composite(case, A0)
    _sync()
    plan_bytes = _native.view_plan_pack_bytes(case.P, case.W, case.H, R)
    pack_bytes = _native.view_pack_bytes(case.P, case.W, case.H, R)
    assert plan_bytes >= pack_bytes > 0 and (R == 0 or plan_bytes > pack_bytes)
    stream = torch.cuda.current_stream()
    for fill in FILLS:
        t = f"{name} {mode} fill {fill:#04x}"
        with guarded_allocations(monkeypatch, _native, fill) as rec:
            # a miss on a bound set, its state saved into both kinds of pack
            A = _GuardedSet(fill, bound=True)
            case.geometry(A)
            got = vb._composite(case, A)
            _assert_same_view(case, ref, got, f"{t}: miss")
            pack = Guarded((pack_bytes,), torch.uint8, DEV, fill=fill, name="pack")
            plan = Guarded((plan_bytes,), torch.uint8, DEV, fill=fill, name="plan pack")
            _native.view_save(_native.view_args(A.bufs, R, pack.tensor), stream)
            _native.view_save(_native.view_args(A.bufs, R, plan.tensor), stream)
            _sync()
            check(pack, plan)
            if R > 0:  # the path: the first compositing's cover masks went into the plan pack
                assert int(plan.tensor[:64].view(torch.int32)[8]) == 1, f"{t}: the compositing flagged no plan"
            before = plan.tensor.clone()
            # the copying restore into a blanked plain set
            B = _GuardedSet(fill)
            case.geometry(B)
            B.blank()
            slots = _rand((case.P, 3), 11)
            case.records(B)[:, 9:12] = slots
            case.restore(B, R, pack.tensor)
            _sync()
            assert torch.equal(case.records(B)[:, 9:12], slots), f"{t}: the restore touched the language slots"
            assert int(B.overflow.item()) == 0
            _assert_same_view(case, ref, vb._composite(case, B), f"{t}: restored")
            # two blanked bound sets on the one plan pack
            C, D = _GuardedSet(fill, bound=True), _GuardedSet(fill, bound=True)
            for s in (C, D):
                case.geometry(s)
                s.blank()
                vb._bind(case, s, R, plan.tensor)
            ec, oc = vb._forward_only(case, C)
            ed, od = vb._forward_only(case, D)
            gc, gd = vb._backward_only(case, oc, True), vb._backward_only(case, od, True)
            _assert_same_view(case, ref, (ec, gc), f"{t}: bound set C")
            _assert_same_view(case, ref, (ed, gd), f"{t}: bound set D")
            _sync()
            assert torch.equal(plan.tensor, before), f"{t}: a bound set wrote the pack"
            for s in (A, B, C, D):
                s.bufs.check_all()
            check(pack, plan)
        rec.check_all()


# ---- levels ----------------------------------------------------------------------------------------------

LP, LW, LH = 301, 67, 45


def _levels_scene():
    st, inp = scene(P=LP, W=LW, H=LH, seed=3, scale_range=(0.03, 0.2))
    return to_device(st, inp, DEV)


def _levels_args(ind):
    return (ind["means3D"], ind.get("shs"), ind.get("colors_precomp")), (
        ind["opacities"], ind.get("scales"), ind.get("rotations"), ind.get("cov3D_precomp"))


def level_quads(L):
    return (3 * (L - 1) + 3) // 4


def rounded(nbytes):
    """The lsr_*_bytes functions round a buffer's content up to the allocation granule."""
    return (nbytes + guards.ALIGN - 1) // guards.ALIGN * guards.ALIGN


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_levels_forward_and_backward(L, monkeypatch):
    """lsr_forward_levels (its LSR_BUF_LEVELS request is lsr_levels_bytes) and lsr_backward_levels (its
    accumulator lsr_backward_levels_bytes, cleared by the call itself)."""
    lib = _native.load()
    std, ind = _levels_scene()
    pre, post = _levels_args(ind)
    feats = level_features(L, LP)
    seeds = torch.stack([grad_seed(LH, LW, seed=7 + l)[1] for l in range(L)]).to(DEV)
    assert lib.lsr_levels_bytes(LP, L) == rounded(16 * level_quads(L) * LP)
    assert lib.lsr_backward_levels_bytes(LP, L) == rounded(4 * 3 * L * LP)

    def run():
        fwd = _native.rasterize_gaussians_levels(std, *pre, feats, *post, with_visibility=True, keep_state=True)
        nr, color, langs, radii, visible, geom, binning, image = fwd
        grad = _native.rasterize_gaussians_levels_backward(std, feats, radii, nr, geom, binning, image,
                                                           grad_images=seeds)
        _sync()
        return fwd, grad

    ref, ref_grad = run()
    assert ref[0] > 0 and bool(ref_grad.any()) and bool(torch.isfinite(ref_grad).all())
    for fill in FILLS:
        t = f"L = {L} fill {fill:#04x}"
        reset_binning_hint()
        gb = GuardedBuffers(fill)
        with gb, guarded_allocations(monkeypatch, _native, fill) as rec:
            fwd, grad = run()
        gb.check_all()
        rec.check_all()
        gb.assert_abi_sizes(LP, LW, LH, fwd[0], _native.LAST_COUNTS[(LP, LW, LH)][1])
        assert gb.requested(LEVELS) == (lib.lsr_levels_bytes(LP, L) if L > 1 else None)
        assert rec.of(grad).nbytes == 4 * 3 * L * LP  # the output; the accumulator is the allocation after it
        assert any(g.nbytes == lib.lsr_backward_levels_bytes(LP, L) and g.dtype == torch.uint8 for g in rec.guards)
        assert fwd[0] == ref[0]
        for name, a, b in zip(("color", "maps", "radii", "visible"), ref[1:5], fwd[1:5]):
            assert torch.equal(a, b), f"{t}: {name} differs"
            assert fill != 0xFF or unwritten(b) == 0, f"{t}: {name} was not fully written"
        assert bool(torch.isfinite(grad).all()) and (fill != 0xFF or unwritten(grad) == 0), t
        assert_grad_close(t, grad.cpu().numpy(), ref_grad.cpu().numpy())


def step_block(count, lrs, fill=None):
    """lsr_adam_multi's device block: the count, the skipped count 0 and the learning rates; the scratch
    words 1 .. 48 keep the fill byte of a Guarded block (else zeros)."""
    if fill is None:
        t = torch.zeros((_native.ADAM_STEP_WORDS,), dtype=torch.int64, device=DEV)
        g = None
    else:
        g = Guarded((_native.ADAM_STEP_WORDS,), torch.int64, DEV, fill=fill, name="step block")
        t = g.tensor
    t[0] = count
    t[_native.ADAM_WORD_SKIPPED] = 0
    lr = torch.tensor([float(x) for x in lrs] + [0.0] * (16 - len(lrs)), dtype=torch.float64).view(torch.int64)
    t[_native.ADAM_WORD_LR:] = lr.to(DEV)
    return g, t


def torch_adam(p0, grad, m0, v0, lr, betas, eps, steps_before):
    """One step of torch.optim.Adam (single-tensor) from the given state: (param, exp_avg, exp_avg_sq)."""
    p = p0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(steps_before)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = grad.clone()
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def assert_adam_close(got, want, tag):
    """test_gpu_optim.py's tolerance: rtol 2e-6 with an absolute floor of 1e-6 x max|value|."""
    for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
        torch.testing.assert_close(x, y, rtol=2e-6, atol=1e-6 * float(y.abs().max()),
                                   msg=lambda m: f"{tag} {name}: {m}")


BETAS, EPS, LR = (0.9, 0.999), 1e-15, 0.0025


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_levels_step_forward_and_backward_with_update(L, skip, monkeypatch):
    """lsr_levels_step_forward in capacity mode and lsr_levels_step_backward with the fused Adam step and
    the fills of another forward's records and level array (k_levels_tail: the last level quad is zero
    padded).  The level array is lsr_levels_bytes: level_quads(L) P float4, rounded up to 256 bytes; in
    the records only the three language slots change; with the skip flag set nothing but the fills and
    the gradient is written."""
    lib = _native.load()
    std, ind = _levels_scene()
    pre, post = _levels_args(ind)
    raw = _native.RAW_LANGUAGE
    feats0 = (level_features(L, LP) * torch.linspace(0.5, 2.0, LP, device=DEV)[None, :, None]).contiguous()
    m0, v0 = _rand((L, LP, 3), 3, 1e-3), _rand((L, LP, 3), 4, 1e-3).abs()
    records0 = _rand((LP, 12), 5)
    seeds = torch.stack([grad_seed(LH, LW, seed=7 + l)[1] for l in range(L)]).to(DEV)
    _native.rasterize_gaussians_levels(std, *pre, feats0, *post, raw=raw)
    R, E = _native.LAST_COUNTS[(LP, LW, LH)]
    assert R > 0
    cap = (R + 64, E + 16)
    levels_bytes = int(lib.lsr_levels_bytes(LP, L))
    assert levels_bytes == rounded(16 * level_quads(L) * LP)

    def run(fill):
        guarded = fill is not None
        new = (lambda src, name: holding(src, fill, name=name)) if guarded else (lambda src, name: None)
        gs = dict(feats=new(feats0, "features"), m=new(m0, "exp_avg"), v=new(v0, "exp_avg_sq"),
                  records=new(records0, "fill_record"))
        t = {k: (g.tensor if guarded else {"feats": feats0, "m": m0, "v": v0, "records": records0}[k].clone())
             for k, g in gs.items()}
        if guarded:
            gs["levels"] = Guarded((max(levels_bytes, 1),), torch.uint8, DEV, fill=fill, name="fill_levels")
            gs["grad"] = Guarded((L, LP, 3), torch.float32, DEV, fill=fill, name="dL_dlanguage_feature")
            gs["scratch"] = Guarded((int(lib.lsr_backward_levels_bytes(LP, L)),), torch.uint8, DEV, fill=fill,
                                    name="scratch")
            t.update(levels=gs["levels"].tensor, grad=gs["grad"].tensor, scratch=gs["scratch"].tensor)
        else:
            t.update(levels=torch.zeros((max(levels_bytes, 1),), dtype=torch.uint8, device=DEV),
                     grad=torch.empty((L, LP, 3), device=DEV), scratch=None)
        gs["block"], block = step_block(4, [LR], fill if guarded else None)
        flag = torch.full((), skip, dtype=torch.int32, device=DEV)
        ovf = torch.zeros((), dtype=torch.int32, device=DEV)
        bufs = GuardedBuffers(fill) if guarded else _native.static_buffers()
        with _native.capacity(*cap, ovf), bufs:
            out = _native.levels_step_forward(std, *pre, t["feats"], *post, raw=raw)
        nr, color, langs, radii, visible, geom, binning, image, lev = out
        upd = _native.LevelsUpdate(t["feats"], t["m"], t["v"], BETAS, EPS, block, skip=flag,
                                   fill_record=t["records"].data_ptr(), fill_levels=t["levels"] if L > 1 else None)
        _native.levels_step_backward(std, t["feats"], radii, nr, geom, binning, image, raw=raw, grad_images=seeds,
                                     update=upd, out=t["grad"], scratch=t["scratch"])
        _sync()
        assert int(ovf.item()) == 0
        return SimpleNamespace(out=out, t=t, gs={k: g for k, g in gs.items() if g is not None}, block=block, bufs=bufs)

    ref = run(None)
    assert bool(ref.t["grad"].any()) and bool(torch.isfinite(ref.t["grad"]).all())
    for fill in FILLS:
        tag = f"L = {L} skip {skip} fill {fill:#04x}"
        with guarded_allocations(monkeypatch, _native, fill) as rec:
            got = run(fill)
        got.bufs.check_all()
        rec.check_all()
        check(*got.gs.values())
        got.bufs.assert_abi_sizes(LP, LW, LH, cap[0], cap[1])
        assert got.bufs.requested(LEVELS) == (levels_bytes if L > 1 else None)
        for name, a, b in zip(("color", "maps", "radii", "visible"), ref.out[1:5], got.out[1:5]):
            assert torch.equal(a, b), f"{tag}: {name} differs"
            assert fill != 0xFF or unwritten(b) == 0, f"{tag}: {name} was not fully written"
        grad = got.t["grad"]
        assert bool(torch.isfinite(grad).all()) and (fill != 0xFF or unwritten(grad) == 0), tag
        assert_grad_close(tag, grad.cpu().numpy(), ref.t["grad"].cpu().numpy())
        # the records: only the three language slots; the level array: every word (zero padded)
        assert torch.equal(got.t["records"][:, :9], records0[:, :9]), f"{tag}: a record word outside the slots changed"
        f = got.t["feats"][0]
        want = f / (f.norm(dim=-1, keepdim=True) + 1e-9)
        torch.testing.assert_close(got.t["records"][:, 9:12], want, rtol=1e-6, atol=1e-7)
        if L > 1:
            rows = got.t["levels"][:16 * level_quads(L) * LP].view(torch.float32).view(LP, 4 * level_quads(L))
            assert fill != 0xFF or unwritten(rows) == 0, f"{tag}: the level array was not fully written"
            assert not rows[:, 3 * (L - 1):].any(), f"{tag}: the last quad's padding is not zero"
            others = got.t["feats"][1:]
            want = (others / (others.norm(dim=-1, keepdim=True) + 1e-9)).permute(1, 0, 2).reshape(LP, 3 * (L - 1))
            torch.testing.assert_close(rows[:, :3 * (L - 1)], want, rtol=1e-6, atol=1e-7)
        # the step block: words 1 .. 48 are the call's scratch, the learning rate is the caller's
        assert int(got.block[_native.ADAM_WORD_LR:].view(torch.float64)[0] == LR) == 1
        if skip:
            assert int(got.block[0]) == 4 and int(got.block[_native.ADAM_WORD_SKIPPED]) == 1
            for k, src in (("feats", feats0), ("m", m0), ("v", v0)):
                assert torch.equal(got.t[k], src), f"{tag}: a skipped step changed {k}"
        else:
            assert int(got.block[0]) == 5 and int(got.block[_native.ADAM_WORD_SKIPPED]) == 0
            assert_adam_close((got.t["feats"], got.t["m"], got.t["v"]),
                              torch_adam(feats0, grad, m0, v0, LR, BETAS, EPS, 4), tag)


# ---- the optimizer family --------------------------------------------------------------------------------

ADAM_NS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 4097)


def _adam_state(n, seed):
    """(param, exp_avg, exp_avg_sq) after one torch step, the next gradient and torch's result of it."""
    p0, g1, g2 = _rand((n,), seed), _rand((n,), seed + 1), _rand((n,), seed + 2)
    zeros = torch.zeros_like(p0)
    p1, m1, v1 = torch_adam(p0, g1, zeros, zeros, 0.01, BETAS, EPS, 0)
    return (p1, m1.clone(), v1.clone()), g2, torch_adam(p1, g2, m1, v1, 0.007, BETAS, EPS, 1)


def _adam_call(entry, bufs, n, block=None, skip=None):
    p, g, m, v = bufs
    lib = _native.load()
    if entry == "step":
        _native._check(lib.lsr_adam_step(n, _p(p), _p(g), _p(m), _p(v), 0.007, *BETAS, EPS, 2, _stream()),
                       "lsr_adam_step")
    else:
        one = _native.LsrAdamTensor(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0.007, *BETAS, EPS, 2)
        tab = (_native.LsrAdamTensor * 1)(one)
        _native._check(lib.lsr_adam_multi(1, tab, 1.0, None, None, _stream()), "lsr_adam_multi")
    _sync()


@pytest.mark.parametrize("which", [None, 0, 1, 2, 3], ids=["aligned", "param+4", "grad+4", "exp_avg+4", "exp_avg_sq+4"])
@pytest.mark.parametrize("entry", ["step", "multi"])
def test_adam_vector_path_tails_and_scalar_path(entry, which):
    """lsr_adam_step (k_adam) and lsr_adam_multi (adam_segment) over one tensor: all four pointers 16-byte
    aligned, so the float4 path runs with every tail length, then each pointer in turn 4 bytes off, which
    takes the scalar path."""
    assert {n % 4 for n in ADAM_NS} == {0, 1, 2, 3} and max(ADAM_NS) > 4 * 256  # every tail, several workgroups
    for n in ADAM_NS:
        state0, grad, want = _adam_state(n, 10 * n)
        srcs = (state0[0], grad, state0[1], state0[2])
        mis = [4 if k == which else 0 for k in range(4)]
        ref = tuple(plain(s, m) for s, m in zip(srcs, mis))
        _adam_call(entry, ref, n)
        assert_adam_close((ref[0], ref[2], ref[3]), want, f"n = {n}")
        for fill in FILLS:
            gs = [holding(s, fill, misalign=m, name=nm)
                  for s, m, nm in zip(srcs, mis, ("param", "grad", "exp_avg", "exp_avg_sq"))]
            got = tuple(g.tensor for g in gs)
            assert [t.data_ptr() % 16 for t in got] == mis  # the path: vector iff all four are aligned
            _adam_call(entry, got, n)
            check(*gs)
            for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), ref, got):
                assert torch.equal(a, b), f"n = {n} {name} fill {fill:#04x}"


RGB_GROUPS = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
RGB_LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


@pytest.mark.parametrize("grads", ["separate", "bucket"])
def test_adam_multi_rgb_groups(grads):
    """The RGB stage's six parameter groups at P = 257 in one launch, their gradients separate tensors
    (float4 path, tails of 257 * k floats) and slices of one GradBucket (offsets not 16-byte aligned: the
    scalar path beside the vector one), with a gradient scale."""
    P, scale = 257, 1.0 / 3.0
    src = {k: (_rand((P,) + s, i), _rand((P,) + s, 10 + i, 1e-2), _rand((P,) + s, 20 + i, 1e-2).abs(),
               _rand((P,) + s, 30 + i)) for i, (k, s) in enumerate(RGB_GROUPS.items())}
    want = {k: torch_adam(p, g * scale, m, v, RGB_LRS[k], BETAS, EPS, 2) for k, (p, m, v, g) in src.items()}

    def run(fill):
        gs, t = {}, {}
        for k, (p, m, v, g) in src.items():
            if fill is None:
                t[k] = [p.clone(), m.clone(), v.clone()]
            else:
                gs[k] = [holding(x, fill, name=f"{k} {nm}")
                         for x, nm in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq"))]
                t[k] = [g_.tensor for g_ in gs[k]]
        if grads == "bucket":
            params = [torch.nn.Parameter(t[k][0]) for k in RGB_GROUPS]
            bucket = GradBucket(params)
            bucket.zero()
            for q, k in zip(params, RGB_GROUPS):
                q.grad.add_(src[k][3])
            gr = {k: q.grad for q, k in zip(params, RGB_GROUPS)}
            assert any(x.data_ptr() % 16 != 0 for x in gr.values()) and any(x.data_ptr() % 16 == 0 for x in gr.values())
        else:
            gr = {k: src[k][3] for k in RGB_GROUPS}
            assert all(x.data_ptr() % 16 == 0 for x in gr.values())
        tab = (_native.LsrAdamTensor * 6)(*[
            _native.LsrAdamTensor(t[k][0].numel(), t[k][0].data_ptr(), gr[k].data_ptr(), t[k][1].data_ptr(),
                                  t[k][2].data_ptr(), RGB_LRS[k], *BETAS, EPS, 3) for k in RGB_GROUPS])
        _native._check(_native.load().lsr_adam_multi(6, tab, scale, None, None, _stream()), "lsr_adam_multi")
        _sync()
        for k in gs:
            check(*gs[k])
        return t

    ref = run(None)
    for k in RGB_GROUPS:
        assert_adam_close(ref[k], want[k], k)
    for fill in FILLS:
        got = run(fill)
        for k in RGB_GROUPS:
            for a, b in zip(ref[k], got[k]):
                assert torch.equal(a, b), f"{k} fill {fill:#04x}"


@pytest.mark.parametrize("skip", [0, 1])
def test_adam_multi_sixteen_tensors_device_step(skip):
    """lsr_adam_multi's device form with 16 tensors: the step block is exactly LSR_ADAM_STEP_WORDS int64
    and guarded (k_adam_advance writes 3 words per tensor, 48 in all, after the count); the skipped
    count and the learning-rate words are the caller's and a normal step leaves them alone."""
    ns = list(ADAM_NS) + [7, 64, 100, 513, 31]
    lrs = [0.001 * (k + 1) for k in range(16)]
    offsets = [0, -1, 0, -3] * 4
    src = [(_rand((n,), 40 + k), _rand((n,), 60 + k, 1e-2), _rand((n,), 80 + k, 1e-2).abs(), _rand((n,), 100 + k))
           for k, n in enumerate(ns)]
    count = 6
    want = [torch_adam(p, g, m, v, lrs[k], BETAS, EPS, count + offsets[k]) for k, (p, m, v, g) in enumerate(src)]

    def run(fill):
        gs, t = [], []
        for k, (p, m, v, g) in enumerate(src):
            if fill is None:
                t.append([p.clone(), m.clone(), v.clone()])
            else:
                gs.append([holding(x, fill, name=f"tensor {k} {nm}")
                           for x, nm in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq"))])
                t.append([g_.tensor for g_ in gs[-1]])
        gblock, block = step_block(count, lrs, fill)
        flag = torch.full((), skip, dtype=torch.int32, device=DEV)
        tab = (_native.LsrAdamTensor * 16)(*[
            _native.LsrAdamTensor(ns[k], t[k][0].data_ptr(), src[k][3].data_ptr(), t[k][1].data_ptr(),
                                  t[k][2].data_ptr(), 123.0, *BETAS, EPS, offsets[k]) for k in range(16)])
        _native._check(_native.load().lsr_adam_multi(16, tab, 1.0, _p(block), _p(flag), _stream()), "lsr_adam_multi")
        _sync()
        for g3 in gs:
            check(*g3)
        if gblock is not None:
            gblock.check()
        return t, block

    ref, ref_block = run(None)
    for fill in FILLS:
        got, block = run(fill)
        tag = f"skip {skip} fill {fill:#04x}"
        assert torch.equal(block[_native.ADAM_WORD_LR:], ref_block[_native.ADAM_WORD_LR:]), f"{tag}: a rate changed"
        assert block[_native.ADAM_WORD_LR:].view(torch.float64).tolist() == lrs
        assert int(block[0]) == count + (0 if skip else 1) and int(block[_native.ADAM_WORD_SKIPPED]) == skip, tag
        for k in range(16):
            for a, b in zip(ref[k], got[k]):
                assert torch.equal(a, b), f"tensor {k} {tag}"
            if skip:
                assert all(torch.equal(a, b) for a, b in zip(got[k], src[k][:3])), f"tensor {k}: a skipped step wrote"
            else:
                assert_adam_close(got[k], want[k], f"tensor {k}")


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("plane", [False, True])
def test_adam_fill_language(plane, skip):
    """lsr_adam_fill_language / _plane at P = 257: parameter and moments guarded; of the records (3 float4
    per Gaussian; plane: one) only the three language slots change -- word b included in what stays; with
    the skip flag set nothing but the fill is written."""
    P, scale = 257, 0.5
    p0, m0, v0, g = _rand((P, 3), 1), _rand((P, 3), 2, 1e-2), _rand((P, 3), 3, 1e-2).abs(), _rand((P, 3), 4)
    words = 4 if plane else 12
    rec0 = _rand((P, words), 5)
    lib = _native.load()
    fn = lib.lsr_adam_fill_language_plane if plane else lib.lsr_adam_fill_language

    def run(fill):
        if fill is None:
            gs = []
            t = [x.clone() for x in (p0, m0, v0, rec0)]
        else:
            gs = [holding(x, fill, name=nm) for x, nm in ((p0, "param"), (m0, "exp_avg"), (v0, "exp_avg_sq"),
                                                           (rec0, "records"))]
            t = [g_.tensor for g_ in gs]
        gblock, block = step_block(2, [LR], fill)
        flag = torch.full((), skip, dtype=torch.int32, device=DEV)
        tab = _native.LsrAdamTensor(3 * P, t[0].data_ptr(), g.data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 99.0,
                                    *BETAS, EPS, 0)
        _native._check(fn(ctypes.byref(tab), scale, _p(block), _p(flag), _p(t[3]), _native.RAW_LANGUAGE, _stream()),
                       "lsr_adam_fill_language")
        _sync()
        check(*gs)
        if gblock is not None:
            gblock.check()
        return t, block

    ref, _ = run(None)
    for fill in FILLS:
        got, block = run(fill)
        tag = f"plane {plane} skip {skip} fill {fill:#04x}"
        for a, b in zip(ref, got):
            assert torch.equal(a, b), tag
        rec = got[3]
        assert torch.equal(rec[:, :words - 3], rec0[:, :words - 3]), f"{tag}: a word outside the language slots changed"
        f = got[0]
        torch.testing.assert_close(rec[:, words - 3:], f / (f.norm(dim=-1, keepdim=True) + 1e-9), rtol=1e-6, atol=1e-7)
        assert int(block[0]) == 2 + (0 if skip else 1) and int(block[_native.ADAM_WORD_SKIPPED]) == skip
        assert block[_native.ADAM_WORD_LR:].view(torch.float64)[0].item() == LR
        if skip:
            assert all(torch.equal(a, b) for a, b in zip(got[:3], (p0, m0, v0))), f"{tag}: a skipped step wrote"
        else:
            assert_adam_close(got[:3], torch_adam(p0, g * scale, m0, v0, LR, BETAS, EPS, 2), tag)


class _Update:
    """What _native.rasterize_gaussians_backward reads of a _native.fused_update, without a capture."""

    def __init__(self, param, m, v, block, skip, fill, defer):
        self.param, self.m, self.v, self.skip, self.fill, self.defer = param, m, v, skip, fill, defer
        self.optimizer = SimpleNamespace(_step_dev=block)
        self.fill_plane, self.used, self.pending = False, False, None

    def table(self):
        return _native.LsrAdamTensor(self.param.numel(), self.param.data_ptr(), None, self.m.data_ptr(),
                                     self.v.data_ptr(), 0.0, *BETAS, EPS, 0)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("defer", [False, True], ids=["direct", "deferred"])
def test_language_tail(defer, skip, monkeypatch):
    """The N = 1 tail (lsr_backward_args.update: k_language_tail), direct and deferred (LSR_BWD_DEFER_TAIL,
    then lsr_language_tail): dL_dmeans2D and dL_dlanguage_feature are fully written; the parameter, its
    moments, the step block and the filled records are guarded."""
    P, W, H = 301, 67, 45
    st, inp = scene(P=P, W=W, H=H, seed=3, scale_range=(0.03, 0.2))
    lang0 = (inp["language_feature_precomp"] * torch.linspace(0.5, 2.0, P)[:, None]).contiguous().to(DEV)
    c = activated_case(st, inp)
    c.kw = dict(raw=_native.RAW_LANGUAGE)
    m0, v0, rec0 = _rand((P, 3), 2, 1e-3), _rand((P, 3), 3, 1e-3).abs(), _rand((P, 12), 5)
    seeds = tuple(t.to(DEV) for t in grad_seed(H, W, seed=9))
    lib = _native.load()

    def run(fill, update=True):
        if fill is None:
            gs = []
            t = [x.clone() for x in (lang0, m0, v0, rec0)]
        else:
            gs = [holding(x, fill, name=nm) for x, nm in ((lang0, "param"), (m0, "exp_avg"), (v0, "exp_avg_sq"),
                                                           (rec0, "records"))]
            t = [g_.tensor for g_ in gs]
        gblock, block = step_block(3, [LR], fill)
        flag = torch.full((), skip, dtype=torch.int32, device=DEV)
        c.f["language_feature"] = t[0]
        bufs = GuardedBuffers(fill) if fill is not None else _native.static_buffers()
        with bufs:
            out = forward(c)
            upd = _Update(t[0], t[1], t[2], block, flag, t[3].data_ptr(), defer) if update else None
            g = backward(c, out, "language", seeds, update=upd)
            if update and defer:
                s, a, keep, part, device = upd.pending
                assert part.numel() == 3 * P + 1
                _native._check(lib.lsr_language_tail(ctypes.byref(s), ctypes.byref(a), _stream()), "lsr_language_tail")
        _sync()
        check(*gs)
        if gblock is not None:
            gblock.check()
        if fill is not None:
            bufs.check_all()
            bufs.assert_abi_sizes(P, W, H, out[0], _native.LAST_COUNTS[(P, W, H)][1])
            # deferred: the gradient records stay in the geometry buffer
            assert (bufs.requested(BACKWARD) is None) == (update and defer)
        return out, g, t, block

    _, plain_grads, _, _ = run(None, update=False)
    ref = run(None)
    assert int((ref[0][3] > 0).sum()) > 0 and int((ref[0][3] <= 0).sum()) >= 0
    for name in ("means2D", "language_feature_precomp"):
        assert_grad_close(f"tail vs plain backward {name}", ref[1][name].cpu().numpy(), plain_grads[name].cpu().numpy())
    for fill in FILLS:
        tag = f"{'deferred' if defer else 'direct'} skip {skip} fill {fill:#04x}"
        reset_binning_hint()
        with guarded_allocations(monkeypatch, _native, fill) as rec:
            out, g, t, block = run(fill)
        rec.check_all()
        assert_same_forward(c, ref[0], out, tag)
        assert_same_grads({"tail": ref[1]}, {"tail": g}, tag, fill, rec)
        assert torch.equal(t[3][:, :9], rec0[:, :9]), f"{tag}: a record word outside the language slots changed"
        f = t[0]
        torch.testing.assert_close(t[3][:, 9:], f / (f.norm(dim=-1, keepdim=True) + 1e-9), rtol=1e-6, atol=1e-7)
        assert int(block[0]) == 3 + (0 if skip else 1) and int(block[_native.ADAM_WORD_SKIPPED]) == skip
        assert block[_native.ADAM_WORD_LR:].view(torch.float64)[0].item() == LR
        if skip:
            assert all(torch.equal(a, b) for a, b in zip(t[:3], (lang0, m0, v0))), f"{tag}: a skipped step wrote"
        else:
            assert_adam_close(t[:3], torch_adam(lang0, g["language_feature_precomp"], m0, v0, LR, BETAS, EPS, 3), tag)


# ---- loss, decode and the small kernels ------------------------------------------------------------------

@pytest.mark.parametrize("offset", [None, "pred", "gt", "grad_pred", "mask"])
@pytest.mark.parametrize("mask_kind", ["bool", "float"])
def test_masked_l1(mask_kind, offset):
    """lsr_masked_l1_forward / _backward: HW with every float4 tail, C beside the compiled C = 3, then one
    of the pointers off by one element (the scalar path).  The scratch is lsr_masked_l1_scratch_bytes,
    zeroed once before its first use as the header asks, and reused by the second forward."""
    lib = _native.load()
    for HW in (1, 3, 4, 5, 35, 4100):
        for C in (1, 3, 4):
            pred, gt = _rand((C, HW), HW + C), _rand((C, HW), HW + C + 50)
            gt[:, ::3] = pred[:, ::3]  # sign 0
            mask = torch.rand((HW,), generator=torch.Generator().manual_seed(HW)).to(DEV) > 0.3
            mask = mask if mask_kind == "bool" else mask.float() * 0.5
            grad_loss = torch.tensor([0.7], device=DEV)
            # autograd's gradient and the fp64 value of l1_loss(pred * mask, gt * mask)
            x = pred.clone().requires_grad_(True)
            mf = mask.to(torch.float32)
            torch.abs(x * mf - gt * mf).mean().backward(torch.tensor(0.7, device=DEV))
            value = ((pred.double() * mf.double() - gt.double() * mf.double()).abs().sum() / (C * HW)).float()
            el = 4 if mask_kind == "float" else 1
            mis = {k: (4 if k == offset else 0) for k in ("pred", "gt", "grad_pred")}
            mis["mask"] = el if offset == "mask" else 0
            vector = HW % 4 == 0 and offset is None
            for fill in FILLS:
                tag = f"HW {HW} C {C} {mask_kind} offset {offset} fill {fill:#04x}"
                gp, gg, gm = (holding(pred, fill, mis["pred"], "pred"), holding(gt, fill, mis["gt"], "gt"),
                              holding(mask, fill, mis["mask"], "mask"))
                out = Guarded((C, HW), torch.float32, DEV, fill=fill, misalign=mis["grad_pred"], name="grad_pred")
                lossv = Guarded((1,), torch.float32, DEV, fill=fill, name="loss")
                scratch = Guarded((int(lib.lsr_masked_l1_scratch_bytes(C, HW)),), torch.uint8, DEV, fill=0x00,
                                  name="scratch")
                aligned = all(t.data_ptr() % 16 == 0 for t in (gp.tensor, gg.tensor, out.tensor)) and \
                    gm.tensor.data_ptr() % (16 if mask_kind == "float" else 4) == 0
                assert (HW % 4 == 0 and aligned) == vector, tag  # the path
                for _ in range(2):
                    lossv.refill()
                    _native._check(lib.lsr_masked_l1_forward(C, HW, _p(gp.tensor), _p(gg.tensor), _p(gm.tensor),
                                                             int(mask_kind == "float"), _p(lossv.tensor),
                                                             _p(scratch.tensor), _stream()), "lsr_masked_l1_forward")
                    _sync()
                    torch.testing.assert_close(lossv.tensor[0], value, rtol=1e-6, atol=0, msg=lambda m: f"{tag}: {m}")
                _native._check(lib.lsr_masked_l1_backward(C, HW, _p(gp.tensor), _p(gg.tensor), _p(gm.tensor),
                                                          int(mask_kind == "float"), _p(grad_loss), _p(out.tensor),
                                                          _stream()), "lsr_masked_l1_backward")
                _sync()
                check(gp, gg, gm, out, lossv, scratch)
                assert fill != 0xFF or out.unwritten() == 0, f"{tag}: grad_pred was not fully written"
                assert torch.equal(out.tensor, x.grad), f"{tag}: grad_pred differs from autograd's"


@pytest.mark.parametrize("H,W", [(1, 1), (37, 53)])
def test_decode_language_feature(H, W, monkeypatch):
    L, N, D = 3, 17, 3
    g = torch.Generator().manual_seed(H * W)
    seg = torch.randint(-1, N, (L, H, W), generator=g).to(DEV)
    seg[1, 0, 0] = -1
    fm = _rand((N, D), 7)
    want = fm[seg[1]].permute(2, 0, 1).contiguous()
    ref = loss_module.decode_language_feature(seg, fm, 1)
    assert torch.equal(ref[0], want) and torch.equal(ref[1][0], seg[1] != -1)
    for fill in FILLS:
        with guarded_allocations(monkeypatch, loss_module, fill) as rec:
            out, mask = loss_module.decode_language_feature(seg, fm, 1)
            _sync()
        rec.check_all()
        assert len(rec.guards) == 2 and rec.of(out).nbytes == 4 * D * H * W and rec.of(mask).nbytes == H * W
        assert fill != 0xFF or (rec.of(out).unwritten() == 0 and unwritten(mask.view(torch.uint8)) == 0)
        assert torch.equal(out, ref[0]) and torch.equal(mask, ref[1])


@pytest.mark.parametrize("missing", [None, 0, 1, 2], ids=["all", "no max_radii2D", "no accum", "no denom"])
def test_densification_stats(missing):
    for P in (1, 255, 257):
        g = torch.Generator().manual_seed(P)
        radii = torch.randint(-1, 40, (P,), generator=g, dtype=torch.int32).clamp_min(0).to(DEV)
        radii[0] = 3
        dm2 = _rand((P, 3), P + 1)
        src = [(torch.rand((P,), generator=g) * 30).to(DEV), torch.rand((P, 1), generator=g).to(DEV),
               torch.randint(0, 5, (P, 1), generator=g).float().to(DEV)]
        vis = radii > 0
        want = [t.clone() for t in src]
        want[0][vis] = torch.max(want[0][vis], radii[vis])
        want[1][vis] += torch.norm(dm2[vis, :2], dim=-1, keepdim=True)
        want[2][vis] += 1
        for fill in FILLS:
            gs = [holding(t, fill, name=nm) for t, nm in zip(src, ("max_radii2D", "xyz_gradient_accum", "denom"))]
            args = [None if k == missing else g_.tensor for k, g_ in enumerate(gs)]
            _native.densification_stats(radii, dm2, *args)
            _sync()
            check(*gs)
            for k, g_ in enumerate(gs):
                if k == missing:
                    assert torch.equal(g_.tensor, src[k]), f"P {P}: a NULL output's tensor changed"
                else:
                    torch.testing.assert_close(g_.tensor, want[k], rtol=1e-6 if k == 1 else 0, atol=0)
                    assert torch.equal(g_.tensor[~vis], src[k][~vis])


@pytest.mark.parametrize("plane", [False, True])
def test_fill_language(plane):
    """lsr_fill_language / _plane at P = 257: the language slots of the visible Gaussians' records, word b
    of {b, f0, f1, f2} and every other word left alone."""
    P = 257
    words = 4 if plane else 12
    rec0, feat = _rand((P, words), 1), _rand((P, 3), 2)
    radii = (torch.arange(P, device=DEV, dtype=torch.int32) % 3) - 1  # -1, 0, 1, ...
    radii[P - 1] = 5
    vis = radii > 0
    for raw in (0, _native.RAW_LANGUAGE):
        want = feat / (feat.norm(dim=-1, keepdim=True) + 1e-9) if raw else feat
        for fill in FILLS:
            rec = holding(rec0, fill, name="records")
            _native.fill_language(feat, raw, radii, rec.tensor.data_ptr(), plane=plane)
            _sync()
            rec.check()
            assert torch.equal(rec.tensor[:, :words - 3], rec0[:, :words - 3]), "a word outside the slots changed"
            assert torch.equal(rec.tensor[~vis], rec0[~vis]), "a culled Gaussian's record changed"
            torch.testing.assert_close(rec.tensor[vis][:, words - 3:], want[vis], rtol=1e-6 if raw else 0,
                                       atol=1e-7 if raw else 0)


@pytest.mark.parametrize("P", [1, 257])
def test_mark_visible(P, monkeypatch):
    st, inp = posed_scene("inside", P, 64, 48, 6)
    std, ind = to_device(st, inp, DEV)
    ref = _native.mark_visible(ind["means3D"], std.viewmatrix, std.projmatrix)
    assert P == 1 or (bool(ref.any()) and not bool(ref.all()))
    for fill in FILLS:
        with guarded_allocations(monkeypatch, _native, fill) as rec:
            vis = _native.mark_visible(ind["means3D"], std.viewmatrix, std.projmatrix)
            _sync()
        rec.check_all()
        assert len(rec.guards) == 1 and rec.guards[0].nbytes == P
        assert torch.equal(vis, ref)


@pytest.mark.parametrize("N", [1, 2, 5, 3000])
def test_dist_cuda2(N, monkeypatch):
    """lsr_dist_cuda2: its scratch comes through the allocator callback (GuardedBuffers), its output from
    the binding's torch.empty (the proxy)."""
    pts = torch.from_numpy(np.random.default_rng(N).uniform(-1, 1, (N, 3)).astype(np.float32)).to(DEV)
    ref = knn.dist_cuda2(pts)
    np.testing.assert_array_equal(ref.cpu().numpy(), oracle.knn_mean_dist3(pts.cpu().numpy()))
    for fill in FILLS:
        gb = GuardedBuffers(fill)
        with gb, guarded_allocations(monkeypatch, knn, fill) as rec:
            out = knn.dist_cuda2(pts)
            _sync()
        gb.check_all()
        rec.check_all()
        assert gb.requested(BACKWARD) is not None and len(rec.guards) == 1 and rec.guards[0].nbytes == 4 * N
        assert fill != 0xFF or N < 4 or rec.guards[0].unwritten() == 0
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"N {N} fill {fill:#04x}"


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 7), (3, TH + 1, TW + 1)], ids=str)
def test_rgb_loss(shape):
    """lsr_rgb_loss_forward / _backward with the terms, the three maps per plane, the SSIM map, the
    gradient and the scratch (lsr_rgb_loss_scratch_bytes: it needs no initialisation) guarded."""
    planes, H, W = shape
    lib = _native.load()
    x, y = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(DEV), \
        torch.rand(shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    dl = torch.tensor([1.7], device=DEV)
    nbytes = int(lib.lsr_rgb_loss_scratch_bytes(planes, H, W))
    assert nbytes > 0

    def run(bufs):
        terms, maps, smap, grad, scratch = bufs
        a = _native.LsrRgbLossArgs(planes, H, W, 0.2, x.data_ptr(), y.data_ptr(), terms.data_ptr(), maps.data_ptr(),
                                   smap.data_ptr(), scratch.data_ptr())
        _native._check(lib.lsr_rgb_loss_forward(ctypes.byref(a), _stream()), "lsr_rgb_loss_forward")
        b = _native.LsrRgbLossBwdArgs(planes, H, W, 0.2, x.data_ptr(), y.data_ptr(), maps.data_ptr(), dl.data_ptr(),
                                      grad.data_ptr())
        _native._check(lib.lsr_rgb_loss_backward(ctypes.byref(b), _stream()), "lsr_rgb_loss_backward")
        _sync()

    shapes = ((3,), (3, planes, H, W), (planes, H, W), (planes, H, W))
    ref = [torch.empty(s, device=DEV) for s in shapes] + [torch.empty((nbytes,), dtype=torch.uint8, device=DEV)]
    run(ref)
    assert all(bool(torch.isfinite(t).all()) for t in ref[:4])
    for fill in FILLS:
        gs = [Guarded(s, torch.float32, DEV, fill=fill, name=nm)
              for s, nm in zip(shapes, ("out_terms", "out_maps", "out_ssim_map", "out_dL_dimage"))]
        gs.append(Guarded((nbytes,), torch.uint8, DEV, fill=fill, name="scratch"))
        run([g.tensor for g in gs])
        check(*gs)
        for g, r in zip(gs[:4], ref[:4]):
            assert fill != 0xFF or g.unwritten() == 0, f"{shape}: {g.name} was not fully written"
            assert torch.equal(g.tensor, r), f"{shape} fill {fill:#04x}: {g.name} differs"
