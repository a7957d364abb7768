"""All language levels in one rasterizer pass (include/lsr.h lsr_forward_levels, langsplat_amd.levels).

The yardstick is exact: the blend weights w = alpha T of the wide walk are the single-level walk's,
and every channel is its own fma(f, w, acc) chain, so level l's map must be bit-identical
(torch.equal, no tolerance) to what the single-level inference forward produces for level l's
features -- and the colour image, radii and num_rendered to that forward's.

Level l's features are normalize(randn(P, 3), seed = 100 + l): every level and channel differs, so
a swapped level or channel cannot pass."""
import numpy as np
import pytest
import torch

import bench
from langsplat_amd import _native, levels
from langsplat_amd.synthetic import make_cameras, make_gaussians
from oracle import oracle
from tests.scenes import posed_scene, scene, settings_for, to_device

pytestmark = pytest.mark.gpu
DEV = "cuda"


def level_features(L, P, device=DEV):
    out = [torch.nn.functional.normalize(torch.randn((P, 3), generator=torch.Generator().manual_seed(100 + l)))
           for l in range(L)]
    return torch.stack(out).to(device) if L else torch.empty((0, P, 3), device=device)


def _args(ind):
    return (ind["means3D"], ind.get("shs"), ind.get("colors_precomp"))


def run_levels(std, ind, feats, **kw):
    return _native.rasterize_gaussians_levels(std, *_args(ind), feats, ind["opacities"], ind.get("scales"),
                                              ind.get("rotations"), ind.get("cov3D_precomp"), **kw)


def run_single(std, ind, feat, **kw):
    return _native.rasterize_gaussians(std, *_args(ind), feat.contiguous(), ind["opacities"], ind.get("scales"),
                                       ind.get("rotations"), ind.get("cov3D_precomp"),
                                       flags=_native.FWD_NO_BACKWARD, **kw)


def check_against_single(st, inp, feats):
    """Every output of the levels call against the single-level inference forward of each level."""
    std, ind = to_device(st, inp, DEV)
    nr, color, langs, radii = run_levels(std, ind, feats)
    L = feats.shape[0]
    assert langs.shape == (L, 3, st.image_height, st.image_width)
    for l in range(L):
        ref = run_single(std, ind, feats[l])
        assert nr == ref[0]
        assert torch.equal(color, ref[1]), f"colour differs from level {l}'s forward"
        assert torch.equal(langs[l], ref[2]), f"level {l} differs"
        assert torch.equal(radii, ref[3])
    torch.cuda.synchronize()
    return nr, color, langs, radii


SCENES = {
    "ring": lambda: scene(P=3000, W=96, H=64, seed=4, scale_range=(0.03, 0.2)),
    # a width that is no tile multiple, near-plane culls, radii larger than the image
    "inside": lambda: posed_scene("inside", P=1500, W=100, H=70, seed=7, scale_range=(0.03, 0.2)),
    "subtile": lambda: scene(P=50, W=9, H=5, seed=0),
}


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_levels_are_bit_identical_to_the_single_level_forward(L, name):
    st, inp = SCENES[name]()
    nr, color, langs, radii = check_against_single(st, inp, level_features(L, inp["means3D"].shape[0]))
    if name != "subtile":
        assert nr > 0 and float(langs.abs().max()) > 0


def test_aliased_and_zero_levels():
    """Level 2 holding level 0's values, and an all-zero level: neither disturbs its neighbours."""
    st, inp = SCENES["ring"]()
    P = inp["means3D"].shape[0]
    f = level_features(3, P)
    alias = torch.stack([f[0], f[1], f[0].clone()])
    _, _, langs, _ = check_against_single(st, inp, alias)
    assert torch.equal(langs[2], langs[0]) and not torch.equal(langs[1], langs[0])
    zero = torch.stack([f[0], torch.zeros_like(f[1]), f[2]])
    _, _, langs, _ = check_against_single(st, inp, zero)
    assert float(langs[1].abs().max()) == 0.0 and float(langs[2].abs().max()) > 0


def test_multi_batch_tiles_dense_scene():
    """Tiles that composite past list entries 256, 512 and 768 (several LDS batches), L = 3."""
    st, inp = scene(P=40000, W=96, H=80, seed=21, scale_range=(0.02, 0.12))
    std, ind = to_device(st, inp, DEV)
    train = _native.rasterize_gaussians(std, *_args(ind), ind["language_feature_precomp"], ind["opacities"],
                                        ind["scales"], ind["rotations"], None)
    nr, image = train[0], train[6]
    lay = _native.state_layout(40000, 96, 80, nr)
    n_contrib = image[lay["n_contrib"]:lay["n_contrib"] + 4 * 96 * 80].view(torch.int32)
    assert int(n_contrib.max()) > 768
    check_against_single(st, inp, level_features(3, 40000))


def test_very_long_tile_lists_four_levels():
    """More than 8192 instances in one tile (test_gpu_parity's dense cluster), L = 4."""
    P = 12000
    g = torch.Generator().manual_seed(9)
    W = H = 32
    st = settings_for(make_cameras(1, W, H)[0], sh_degree=0)
    inp = dict(means3D=(torch.rand((P, 3), generator=g) - 0.5) * 0.05,
               opacities=torch.rand((P, 1), generator=g) * 0.05 + 0.004,
               colors_precomp=torch.rand((P, 3), generator=g),
               language_feature_precomp=torch.nn.functional.normalize(torch.randn((P, 3), generator=g)),
               scales=torch.full((P, 3), 0.01), rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1))
    nr, _, _, _ = check_against_single(st, inp, level_features(4, P))
    assert nr > 8192


def test_levels_match_the_oracle():
    st, inp = scene(P=600, W=64, H=48, seed=21, scale_range=(0.03, 0.2))
    feats = level_features(3, 600, device="cpu")
    std, ind = to_device(st, inp, DEV)
    nr, color, langs, radii = run_levels(std, ind, feats.to(DEV))
    for l in range(3):
        run = oracle.forward(st, **dict(inp, language_feature_precomp=feats[l].contiguous()))
        assert nr == run.num_rendered
        np.testing.assert_array_equal(langs[l].cpu().numpy(), run.language)
        np.testing.assert_array_equal(color.cpu().numpy(), run.color)
        np.testing.assert_array_equal(radii.cpu().numpy(), run.radii)


def _model(P, seed=0):
    return bench.Model(make_gaussians(P, seed=seed, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12)).to(DEV),
                       include_feature=True)


def _render_each(cam, model, pipe, bg, feats, **kw):
    """render() under no_grad with _language_feature set to each level in turn."""
    from langsplat_amd.render import render
    out = []
    keep = model._language_feature
    try:
        for l in range(feats.shape[0]):
            model._language_feature = torch.nn.Parameter(feats[l].clone().contiguous())
            with torch.no_grad():
                out.append(render(cam, model, pipe, bg, bench.Opt, **kw))
    finally:
        model._language_feature = keep
    return out


class _PipeSH:
    convert_SHs_python = True
    compute_cov3D_python = False
    debug = False


@pytest.mark.parametrize("form", ["fused", "convert_shs", "override_color"])
def test_render_levels_equals_render_per_level(form):
    """The glue on a bench.Model-style model with RAW features: P = 3001 (the fill's vector path has
    a tail), one raw row exactly zero (must render as 0), the input a non-contiguous view."""
    P, W, H, L = 3001, 96, 64, 3
    model = _model(P)
    cam = make_cameras(1, W, H, device=DEV)[0]
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    wide = torch.empty((L, P, 6), device=DEV)
    wide[..., :3] = level_features(L, P) * torch.linspace(0.5, 4.0, P, device=DEV)[None, :, None]  # raw: any norm
    feats = wide[..., :3]
    assert not feats.is_contiguous()
    with torch.no_grad():
        radii0 = levels.render_levels(cam, model, bench.Pipe, bg, bench.Opt, feats)["radii"]
    seen = int(torch.nonzero(radii0 > 0)[0])
    wide[1, seen, :3] = 0.0  # a visible Gaussian whose level-1 raw feature is exactly zero
    pipe = _PipeSH if form == "convert_shs" else bench.Pipe
    kw = {"override_color": torch.rand((P, 3), generator=torch.Generator().manual_seed(5)).to(DEV)} \
        if form == "override_color" else {}
    pkg = levels.render_levels(cam, model, pipe, bg, bench.Opt, feats, **kw)
    refs = _render_each(cam, model, pipe, bg, feats, **kw)
    torch.cuda.synchronize()
    assert sorted(pkg) == ["language_feature_images", "radii", "render", "visibility_filter"]
    assert not torch.isnan(pkg["language_feature_images"]).any()
    for l, ref in enumerate(refs):
        assert torch.equal(pkg["language_feature_images"][l], ref["language_feature_image"]), (form, l)
        assert torch.equal(pkg["render"], ref["render"])
        assert torch.equal(pkg["radii"], ref["radii"])
        assert torch.equal(pkg["visibility_filter"], ref["visibility_filter"])
    assert int(pkg["visibility_filter"].sum()) > 0.3 * P
    assert float(pkg["language_feature_images"][1].abs().max()) > 0


def test_empty_and_fully_culled_scenes_give_zero_levels():
    """P == 0 and a fully culled scene (test_gpu_parity's) with bg = 0.3: every level's map is exactly
    zero.  The colour image is lsr_forward's for the same input, as the contract says: the background
    for the culled scene, and for P == 0 the zero image lsr_forward leaves there (upstream renders
    nothing into a zero-initialised image when there is nothing to draw; test_gpu_parity pins that
    against the oracle), not the background."""
    st, inp = scene(P=50, W=32, H=32, seed=0)
    st = st._replace(bg=torch.tensor([0.3, 0.3, 0.3]))
    bgimg = torch.full((3, 32, 32), 0.3, device=DEV)
    for L in (1, 3, 4):
        std, ind = to_device(st, {k: v[:0] for k, v in inp.items()}, DEV)
        nr, color, langs, radii = run_levels(std, ind, level_features(L, 0))
        ref = run_single(std, ind, torch.empty((0, 3), device=DEV))
        assert nr == 0 and radii.numel() == 0
        assert torch.equal(color, ref[1]) and torch.equal(color, torch.zeros_like(color))
        assert langs.shape == (L, 3, 32, 32) and float(langs.abs().max()) == 0.0
        culled = dict(inp)
        culled["means3D"] = inp["means3D"] * 0.01 + torch.tensor([0.0, 0.0, -3.9])  # behind the near plane
        std, ind = to_device(st, culled, DEV)
        nr, color, langs, radii = run_levels(std, ind, level_features(L, 50))
        assert nr == 0 and int(radii.abs().max()) == 0 and torch.equal(color, bgimg)
        assert float(langs.abs().max()) == 0.0


def test_deterministic_across_calls_and_streams():
    st, inp = SCENES["ring"]()
    std, ind = to_device(st, inp, DEV)
    feats = level_features(3, 3000)
    a = run_levels(std, ind, feats, with_visibility=True)
    b = run_levels(std, ind, feats, with_visibility=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run_levels(std, ind, feats, with_visibility=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert a[0] == b[0] == c[0]
    for x, y, z in zip(a[1:], b[1:], c[1:]):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a[4], a[3] > 0)


def test_outputs_never_require_grad():
    P, W, H = 500, 64, 48
    model = _model(P)
    for p in (model._xyz, model._features_dc, model._features_rest, model._opacity, model._scaling, model._rotation):
        p.requires_grad_(True)
    cam = make_cameras(1, W, H, device=DEV)[0]
    feats = level_features(2, P).requires_grad_(True)
    assert torch.is_grad_enabled()
    pkg = levels.render_levels(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, feats)
    for k, v in pkg.items():
        assert not v.requires_grad and v.grad_fn is None, k
    ref = _render_each(cam, model, bench.Pipe, torch.zeros(3, device=DEV), feats.detach())
    assert torch.equal(pkg["language_feature_images"][1], ref[1]["language_feature_image"])


def test_render_levels_relevancy_equals_relevancy_of_stacked_renders():
    from langsplat_amd import render_levels_relevancy
    from langsplat_amd.query import Decoder, relevancy_map
    from tests import query_ref
    P, W, H, L, n_pos, n_neg = 2000, 64, 48, 3, 3, 4
    c = query_ref.make_case([16, 32, 32], 1, n_pos, n_neg, 7)
    dec = Decoder.from_arrays(c["weights"], c["biases"], device=DEV)
    pos, neg = torch.from_numpy(c["pos"]).to(DEV), torch.from_numpy(c["neg"]).to(DEV)
    model = _model(P)
    cam = make_cameras(1, W, H, device=DEV)[0]
    bg = torch.zeros(3, device=DEV)
    feats = level_features(L, P)
    pkg = render_levels_relevancy(cam, model, bench.Pipe, bg, bench.Opt, feats, dec, pos, neg)
    stacked = torch.stack([r["language_feature_image"] for r in _render_each(cam, model, bench.Pipe, bg, feats)])
    assert pkg["relevancy"].shape == (L, n_pos, H, W)
    assert torch.equal(pkg["language_feature_images"], stacked)
    assert torch.equal(pkg["relevancy"], relevancy_map(stacked, dec, pos, neg))


def test_level_buffer_request_is_what_the_abi_reports(monkeypatch):
    """The LSR_BUF_LEVELS request equals lsr_levels_bytes(P, L) (none at L = 1), beside the geometry and
    image requests lsr_forward makes."""
    lib = _native.load()
    made = []

    class Spy(_native._Allocator):
        def __init__(self, device):
            super().__init__(device)
            made.append(self)
    monkeypatch.setattr(_native, "_Allocator", Spy)
    P, W, H = 3001, 160, 120
    st, inp = scene(P=P, W=W, H=H, seed=3, scale_range=(0.03, 0.2))
    std, ind = to_device(st, inp, DEV)
    for L in (1, 2, 3, 4):
        made.clear()
        run_levels(std, ind, level_features(L, P))
        (a,) = made
        assert a.get(_native.LSR_BUF_GEOM).numel() == lib.lsr_geom_bytes(P, W, H)
        assert a.get(_native.LSR_BUF_IMAGE).numel() == lib.lsr_image_bytes(W, H)
        if L == 1:
            assert _native.LSR_BUF_LEVELS not in a.buffers
        else:
            assert a.buffers[_native.LSR_BUF_LEVELS].numel() == lib.lsr_levels_bytes(P, L) >= 16 * ((3 * L) // 4) * P
    torch.cuda.synchronize()
