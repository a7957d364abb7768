"""The language gradient of all levels in one pass (include/lsr.h lsr_backward_levels) and the training
side of langsplat_amd.levels (render_levels_train, LevelsStep).

Yardstick of every gradient: tests.test_gpu_parity.assert_grad_close, the project's 1e-4 bar with its
1e-2 max floor, outliers = 0, against
    oracle.forward(st, **inputs_with_level_l_features).backward(zeros, g_l)["language_feature_precomp"].
Level l's features are test_gpu_levels.level_features', its seed grad_seed(H, W, seed=7 + l)[1]: every
level and channel differs, so a swapped level or channel cannot pass.  The oracle runs once per scene
and level (cached) and is shared by the tests of that scene."""
import functools

import numpy as np
import pytest
import torch

import bench
from langsplat_amd import _native, levels
from langsplat_amd.loss import masked_l1_loss
from langsplat_amd.optim import Adam
from langsplat_amd.render import render
from langsplat_amd.synthetic import make_cameras, make_gaussians
from oracle import oracle
from tests.scenes import grad_seed, scene, settings_for, to_device
from tests.test_gpu_captured_forms import assert_states_close
from tests.test_gpu_levels import SCENES, _PipeSH, level_features
from tests.test_gpu_parity import GRAD_FLOOR, assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _long_list_scene():
    """test_gpu_levels.test_very_long_tile_lists_four_levels' scene: > 8192 instances in one tile."""
    P = 12000
    g = torch.Generator().manual_seed(9)
    st = settings_for(make_cameras(1, 32, 32)[0], sh_degree=0)
    inp = dict(means3D=(torch.rand((P, 3), generator=g) - 0.5) * 0.05,
               opacities=torch.rand((P, 1), generator=g) * 0.05 + 0.004,
               colors_precomp=torch.rand((P, 3), generator=g),
               language_feature_precomp=torch.nn.functional.normalize(torch.randn((P, 3), generator=g)),
               scales=torch.full((P, 3), 0.01), rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1))
    return st, inp


ALL_SCENES = dict(SCENES,
                  base=lambda: scene(P=600, W=64, H=48, seed=21, scale_range=(0.03, 0.2)),
                  dense=lambda: scene(P=40000, W=96, H=80, seed=21, scale_range=(0.02, 0.12)),
                  long=_long_list_scene)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return ALL_SCENES[name]()


def seeds_for(L, H, W):
    return torch.stack([grad_seed(H, W, seed=7 + l)[1] for l in range(L)]) if L else torch.empty((0, 3, H, W))


def oracle_grad(st, inp, feat, seed):
    """dL/d(activated features) of one level for the map gradient `seed` (3, H, W): (P, 3) float32."""
    run = oracle.forward(st, **dict(inp, language_feature_precomp=feat.contiguous()))
    zeros = torch.zeros((3, st.image_height, st.image_width))
    return run.backward(zeros, seed.contiguous())["language_feature_precomp"]


@functools.lru_cache(maxsize=None)
def reference(name, l):
    """The oracle's gradient of level l of scene `name` under the standard features and seeds."""
    st, inp = _scene(name)
    P = inp["means3D"].shape[0]
    feat = level_features(l + 1, P, device="cpu")[l]
    return oracle_grad(st, inp, feat, grad_seed(st.image_height, st.image_width, seed=7 + l)[1])


def _args(ind):
    return (ind["means3D"], ind.get("shs"), ind.get("colors_precomp"))


def forward(std, ind, feats, raw=0):
    """(num_rendered, color, maps, radii, geom, binning, image) of the levels forward, state kept."""
    return _native.rasterize_gaussians_levels(std, *_args(ind), feats, ind["opacities"], ind.get("scales"),
                                              ind.get("rotations"), ind.get("cov3D_precomp"), raw=raw, keep_state=True)


def backward(std, feats, fwd, raw=0, **seeds):
    nr, _, _, radii, geom, binning, image = fwd
    return _native.rasterize_gaussians_levels_backward(std, feats, radii, nr, geom, binning, image, raw=raw, **seeds)


def run_standard(name, L):
    """The ABI pair on scene `name` with the standard features and seeds: (gradient (L, P, 3), radii)."""
    st, inp = _scene(name)
    std, ind = to_device(st, inp, DEV)
    feats = level_features(L, inp["means3D"].shape[0])
    fwd = forward(std, ind, feats)
    grad = backward(std, feats, fwd, grad_images=seeds_for(L, st.image_height, st.image_width).to(DEV))
    torch.cuda.synchronize()
    return grad, fwd[3]


def check_standard(name, L):
    grad, radii = run_standard(name, L)
    assert grad.shape == (L, radii.shape[0], 3)
    culled = (radii <= 0).cpu().numpy()
    for l in range(L):
        got = grad[l].cpu().numpy()
        assert_grad_close(f"{name} level {l}", got, reference(name, l))
        assert not got[culled].any(), f"{name} level {l}: a culled Gaussian has a gradient"
    return grad, radii


# ---- 1. oracle parity at the ABI -------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_oracle_parity_levels(L):
    grad, radii = check_standard("base", L)
    assert float(grad.abs().max()) > 0 and int((radii > 0).sum()) > 0


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_parity_scenes(name):
    grad, radii = check_standard(name, 3)
    if name == "inside":  # near-plane culls: some rows are exactly zero by the radius gate
        assert int((radii <= 0).sum()) > 0
    if name != "subtile":
        assert float(grad.abs().max()) > 0


# ---- 2., 3. several batches, very long lists -------------------------------------------------------

def test_several_batches_dense_scene():
    """Pixels composite past list entries 256, 512 and 768 (test_gpu_levels pins that for this scene)."""
    check_standard("dense", 3)


def test_very_long_tile_lists_four_levels():
    st, inp = _scene("long")
    std, ind = to_device(st, inp, DEV)
    assert forward(std, ind, level_features(4, 12000))[0] > 8192
    check_standard("long", 4)


# ---- 4. level isolation ----------------------------------------------------------------------------

def test_zero_seed_level_is_exactly_zero_and_leaves_its_neighbours():
    st, inp = _scene("base")
    std, ind = to_device(st, inp, DEV)
    feats = level_features(3, 600)
    seeds = seeds_for(3, 48, 64)
    seeds[1] = 0.0
    grad = backward(std, feats, forward(std, ind, feats), grad_images=seeds.to(DEV))
    assert not grad[1].any()
    for l in (0, 2):
        assert_grad_close(f"level {l}", grad[l].cpu().numpy(), reference("base", l))


def test_aliased_level_gets_the_aliased_gradient():
    st, inp = _scene("base")
    std, ind = to_device(st, inp, DEV)
    f = level_features(3, 600)
    feats = torch.stack([f[0], f[1], f[0].clone()])
    seeds = seeds_for(3, 48, 64)
    seeds[2] = seeds[0]
    grad = backward(std, feats, forward(std, ind, feats), grad_images=seeds.to(DEV))
    for l, ref in ((0, 0), (1, 1), (2, 0)):
        assert_grad_close(f"level {l}", grad[l].cpu().numpy(), reference("base", ref))


# ---- 5. raw chain ----------------------------------------------------------------------------------

def test_raw_features_chain_the_normalisation():
    st, inp = _scene("base")
    std, ind = to_device(st, inp, DEV)
    L, P = 3, 600
    factor = torch.rand((P, 1), generator=torch.Generator().manual_seed(3)) * 1.5 + 0.5
    raw = (level_features(L, P, device="cpu") * factor).contiguous()
    fwd = forward(std, ind, raw.to(DEV), raw=_native.RAW_LANGUAGE)
    grad = backward(std, raw.to(DEV), fwd, raw=_native.RAW_LANGUAGE, grad_images=seeds_for(L, 48, 64).to(DEV))
    culled = (fwd[3] <= 0).cpu().numpy()
    for l in range(L):
        act = torch.from_numpy(oracle.activate(oracle.RAW_LANGUAGE, language=raw[l])[3])
        g_act = oracle_grad(st, inp, act, grad_seed(48, 64, seed=7 + l)[1])
        ref = oracle.activate_backward(oracle.RAW_LANGUAGE, (None, None, None, raw[l]), (None, None, None, g_act))[3]
        got = grad[l].cpu().numpy()
        assert_grad_close(f"raw level {l}", got, ref)
        assert not got[culled].any()
        # the chain rule was applied: the raw gradient is orthogonal-ish to the raw feature, the activated is not
        assert not np.allclose(got, g_act, rtol=1e-3, atol=0)


# ---- 6. fused seed ---------------------------------------------------------------------------------

def _fused_case():
    """Base scene, L = 3: targets are the maps of other features, masks ~30 % false, and one 8 x 8
    block where the target equals the map exactly and the mask is set (sign 0)."""
    st, inp = _scene("base")
    std, ind = to_device(st, inp, DEV)
    L, P, H, W = 3, 600, 48, 64
    feats = level_features(L, P)
    fwd = forward(std, ind, feats)
    maps = fwd[2]
    gts = forward(std, ind, torch.roll(level_features(4, P), 1, dims=0)[:L].contiguous())[2].clone()
    masks = (torch.rand((L, H, W), generator=torch.Generator().manual_seed(11)) > 0.3).to(DEV)
    block = (slice(None), slice(16, 24), slice(24, 32))
    gts[:, :, 16:24, 24:32] = maps[:, :, 16:24, 24:32]
    masks[block] = True
    assert float(maps[:, :, 16:24, 24:32].abs().max()) > 0  # the block is drawn: zero there means sign 0, not no entry
    dl = torch.tensor([0.7, -1.3, 2.1], device=DEV)
    return st, inp, std, feats, fwd, gts, masks, block, dl


def _autograd_seed(maps, gts, masks, dl):
    f = maps.detach().clone().requires_grad_(True)
    loss = sum(dl[l] * torch.nn.functional.l1_loss(f[l] * masks[l], gts[l] * masks[l]) for l in range(f.shape[0]))
    return torch.autograd.grad(loss, f)[0]


def test_fused_seed_matches_autograd_of_the_masked_l1():
    st, inp, std, feats, fwd, gts, masks, block, dl = _fused_case()
    seed = _autograd_seed(fwd[2], gts, masks, dl)
    assert not seed[:, :, 16:24, 24:32].any() and float(seed.abs().max()) > 0
    fused = dict(images=fwd[2], targets=gts, masks=masks, grad_losses=dl)
    grad = backward(std, feats, fwd, **fused)
    extra = seeds_for(3, 48, 64).to(DEV)
    both = backward(std, feats, fwd, grad_images=extra, **fused)
    for l in range(3):
        feat = feats[l].cpu()
        assert_grad_close(f"fused level {l}", grad[l].cpu().numpy(), oracle_grad(st, inp, feat, seed[l].cpu()))
        assert_grad_close(f"both seeds level {l}", both[l].cpu().numpy(),
                          oracle_grad(st, inp, feat, (seed[l] + extra[l]).cpu()))


def test_pixels_whose_target_equals_the_map_contribute_exactly_nothing():
    st, inp, std, feats, fwd, gts, masks, block, dl = _fused_case()
    only = torch.zeros_like(masks)
    only[block] = True
    grad = backward(std, feats, fwd, images=fwd[2], targets=gts, masks=only, grad_losses=dl)
    assert grad.shape == (3, 600, 3) and not grad.any()
    # the same masks with a target that differs in the block do contribute
    grad = backward(std, feats, fwd, images=fwd[2], targets=gts + 0.25, masks=only, grad_losses=dl)
    assert float(grad.abs().max()) > 0


# ---- 7. Python -------------------------------------------------------------------------------------

def _model(P, seed=0):
    return bench.Model(make_gaussians(P, seed=seed, sh_degree=3, extent=1.0, scale_range=(0.02, 0.12)).to(DEV),
                       include_feature=True)


def _targets(cam, model, pipe, bg, L, P, H, W, seed=11):
    other = torch.roll(level_features(4, P), 1, dims=0)[:L].contiguous()
    gts = levels.render_levels(cam, model, pipe, bg, bench.Opt, other)["language_feature_images"].clone()
    masks = (torch.rand((L, H, W), generator=torch.Generator().manual_seed(seed)) > 0.3).to(DEV)
    return gts, masks


@pytest.mark.parametrize("form", ["fused", "unfused"])
def test_render_levels_train(form):
    P, W, H, L = 3000, 96, 64, 3
    model = _model(P)
    cam = make_cameras(1, W, H, device=DEV)[0]
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    pipe = bench.Pipe if form == "fused" else _PipeSH
    feats = (level_features(L, P) * torch.linspace(0.5, 2.0, P, device=DEV)[None, :, None]).requires_grad_(True)
    gts, masks = _targets(cam, model, pipe, bg, L, P, H, W)
    pkg = levels.render_levels_train(cam, model, pipe, bg, bench.Opt, feats, language_targets=(gts, masks))
    ref = levels.render_levels(cam, model, pipe, bg, bench.Opt, feats)
    assert sorted(pkg) == ["language_feature_images", "language_l1", "radii", "render", "visibility_filter"]
    assert torch.equal(pkg["language_feature_images"], ref["language_feature_images"])
    assert torch.equal(pkg["render"], ref["render"]) and not pkg["render"].requires_grad
    assert torch.equal(pkg["radii"], ref["radii"]) and torch.equal(pkg["visibility_filter"], ref["visibility_filter"])
    for v in ref.values():
        assert not v.requires_grad and v.grad_fn is None
    assert pkg["language_l1"].shape == (L,) and pkg["language_l1"].requires_grad
    for l in range(L):
        want = masked_l1_loss(pkg["language_feature_images"][l].detach(), gts[l], masks[l])
        assert torch.equal(pkg["language_l1"][l].detach(), want), l
    (grad,) = torch.autograd.grad(pkg["language_l1"].sum(), feats)
    assert grad.shape == (L, P, 3)
    keep = model._language_feature
    try:
        for l in range(L):
            model._language_feature = torch.nn.Parameter(feats[l].detach().clone().contiguous())
            one = render(cam, model, pipe, bg, bench.Opt, language_target=(gts[l], masks[l][None]))
            one["language_l1"].backward()
            want = model._language_feature.grad.double()
            # both sides are GPU results, each held to 1e-4 against the oracle: the bar between them is the sum
            floor = GRAD_FLOOR * float(want.abs().max())
            assert floor > 0
            bad = (grad[l].double() - want).abs() > 2e-4 * (want.abs() + floor)
            assert not bad.any(), f"{form} level {l}: {int(bad.sum())} / {bad.numel()} entries off"
    finally:
        model._language_feature = keep


def test_gradient_through_the_images_and_through_both():
    """A loss on the maps uses dL_dout; one on maps and language_l1 adds the two seeds.  Reference:
    autograd through masked_l1_loss of the same maps (its gradient image fed back as dL_dout)."""
    P, W, H, L = 3000, 96, 64, 2
    model = _model(P)
    cam = make_cameras(1, W, H, device=DEV)[0]
    bg = torch.zeros(3, device=DEV)
    feats = level_features(L, P).requires_grad_(True)
    gts, masks = _targets(cam, model, bench.Pipe, bg, L, P, H, W)
    weight = torch.randn((L, 3, H, W), generator=torch.Generator().manual_seed(2)).to(DEV)

    def run(with_images, with_l1):
        pkg = levels.render_levels_train(cam, model, bench.Pipe, bg, bench.Opt, feats, language_targets=(gts, masks))
        loss = 0.0
        if with_images:
            loss = loss + (pkg["language_feature_images"] * weight).sum()
        if with_l1:
            loss = loss + pkg["language_l1"].sum()
        return torch.autograd.grad(loss, feats)[0].double()

    a, b, both = run(True, False), run(False, True), run(True, True)
    want = a + b
    floor = GRAD_FLOOR * float(want.abs().max())
    assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0
    assert not ((both - want).abs() > 2e-4 * (want.abs() + floor)).any()


def test_frozen_geometry_is_required_while_grad_is_enabled():
    P, W, H = 500, 64, 48
    model = _model(P)
    cam = make_cameras(1, W, H, device=DEV)[0]
    feats = level_features(2, P).requires_grad_(True)
    model._scaling.requires_grad_(True)
    with pytest.raises(ValueError, match="_scaling"):
        levels.render_levels_train(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, feats)
    with torch.no_grad():
        pkg = levels.render_levels_train(cam, model, bench.Pipe, torch.zeros(3, device=DEV), bench.Opt, feats)
    assert not pkg["language_feature_images"].requires_grad


# ---- 8. step ---------------------------------------------------------------------------------------

def test_levels_step_is_adam_on_the_gradient_it_produced():
    P, W, H, L = 3000, 96, 64, 3
    model = _model(P)
    cam = make_cameras(1, W, H, device=DEV)[0]
    bg = torch.zeros(3, device=DEV)
    feats = torch.nn.Parameter(level_features(L, P).clone())
    gts, masks = _targets(cam, model, bench.Pipe, bg, L, P, H, W)
    opt = Adam([{"params": [feats], "lr": 0.0025, "name": "language_feature"}], lr=0.0, eps=1e-15)
    twin = feats.detach().clone().requires_grad_(True)
    topt = torch.optim.Adam([twin], lr=0.0025, eps=1e-15)
    seen = []
    feats.register_hook(lambda g: seen.append(g.detach().clone()))
    losses = levels.LevelsStep(model, feats, opt).step(cam, bench.Pipe, bg, bench.Opt, gts, masks)
    assert losses.shape == (L,) and not losses.requires_grad and feats.grad is None
    assert len(seen) == 1 and float(seen[0].abs().max()) > 0
    twin.grad = seen[0]
    topt.step()
    st, tst = opt.state[feats], topt.state[twin]
    assert_states_close((feats.detach(), st["exp_avg"], st["exp_avg_sq"]),
                        (twin.detach(), tst["exp_avg"], tst["exp_avg_sq"]), "levels step")
    assert int(st["step"].item()) == 1


def test_twenty_steps_on_two_cameras_lower_every_levels_loss():
    P, W, H, L = 3000, 96, 64, 3
    model = _model(P)
    cams = make_cameras(2, W, H, device=DEV)
    bg = torch.zeros(3, device=DEV)
    feats = torch.nn.Parameter(level_features(L, P).clone())
    targets = [_targets(cam, model, bench.Pipe, bg, L, P, H, W, seed=11 + k) for k, cam in enumerate(cams)]
    opt = Adam([{"params": [feats], "lr": 0.01, "name": "language_feature"}], lr=0.0, eps=1e-15)
    step = levels.LevelsStep(model, feats, opt)
    history = [[], []]
    for i in range(20):
        k = i % 2
        history[k].append(step.step(cams[k], bench.Pipe, bg, bench.Opt, *targets[k]).cpu())
    for k in (0, 1):
        first, last = history[k][0], history[k][-1]
        assert (last < first).all(), (k, first, last)
    parts = levels.split_levels(feats)
    assert len(parts) == L and torch.equal(torch.stack(parts), feats.detach())


# ---- 9. empty and fully culled scenes, P == 0, another stream --------------------------------------

def test_empty_and_fully_culled_scenes_give_zero_gradients():
    st, inp = scene(P=50, W=32, H=32, seed=0)
    for L in (1, 3, 4):
        seeds = seeds_for(L, 32, 32).to(DEV)
        std, ind = to_device(st, {k: v[:0] for k, v in inp.items()}, DEV)
        feats = level_features(L, 0)
        fwd = forward(std, ind, feats)
        grad = backward(std, feats, fwd, grad_images=seeds)
        assert fwd[0] == 0 and grad.shape == (L, 0, 3)
        culled = dict(inp)
        culled["means3D"] = inp["means3D"] * 0.01 + torch.tensor([0.0, 0.0, -3.9])  # behind the near plane
        std, ind = to_device(st, culled, DEV)
        feats = level_features(L, 50)
        fwd = forward(std, ind, feats)
        assert fwd[0] == 0 and int(fwd[3].abs().max()) == 0
        grad = backward(std, feats, fwd, raw=_native.RAW_LANGUAGE, grad_images=seeds, images=fwd[2],
                        targets=torch.ones_like(fwd[2]), masks=torch.ones((L, 32, 32), dtype=torch.bool, device=DEV),
                        grad_losses=torch.ones((L,), device=DEV))
        torch.cuda.synchronize()
        assert grad.shape == (L, 50, 3) and not grad.any()


def test_works_on_another_stream():
    st, inp = _scene("base")
    std, ind = to_device(st, inp, DEV)
    feats = level_features(3, 600)
    seeds = seeds_for(3, 48, 64).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        grad = backward(std, feats, forward(std, ind, feats), grad_images=seeds)
    side.synchronize()
    for l in range(3):
        assert_grad_close(f"side stream level {l}", grad[l].cpu().numpy(), reference("base", l))
