"""All language levels of a scene in one rasterizer pass (include/lsr.h lsr_forward_levels).

LangSplat trains its semantic levels from one RGB checkpoint with the geometry frozen
(scene/gaussian_model.py:203-217; train.py:222 writes <model>_1/_2/_3), so the level models differ
only in `_language_feature`, and evaluation stacks their rendered maps
(eval/evaluate_iou_loc.py:258-266).  stack_levels checks that and stacks the features;
render_levels is render()'s glue for one inference forward that returns every level's map, each
bit-identical to render()'s for that level.

Training (include/lsr.h lsr_backward_levels): the level runs differ only in `_language_feature` and in
the target and mask of their feature_level (train.py:97-98), so render_levels_train is one autograd
function over the (L, P, 3) features that shares the geometry pass, the compositing walk and one
gradient walk among the levels, and LevelsStep is one joint step with Adam; split_levels undoes the
stacking.  render_levels itself stays inference only.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

from typing import Sequence

import torch

from . import _native
from .render import _fusable, camera_settings, unfused_inputs

_GEOMETRY = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def stack_levels(models: Sequence):
    """The shared geometry of level checkpoints plus their stacked features.

    Every model's _xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation (torch.equal) and
    active_sh_degree must equal the first model's: ValueError names the first field that differs.
    Returns (models[0], language_features): the first model serves as the geometry, and
    language_features is the (L, P, 3) stack of the raw _language_feature tensors."""
    models = list(models)
    if not 1 <= len(models) <= _native.MAX_LEVELS:
        raise ValueError(f"stack_levels: 1 to {_native.MAX_LEVELS} level models, got {len(models)}")
    first = models[0]
    for i, m in enumerate(models[1:], start=1):
        for name in _GEOMETRY:
            a, b = getattr(first, name), getattr(m, name)
            if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device or not torch.equal(a, b):
                raise ValueError(f"stack_levels: level model {i} differs from level model 0 in {name}; the levels "
                                 "must come from one RGB checkpoint with the geometry frozen")
        if int(m.active_sh_degree) != int(first.active_sh_degree):
            raise ValueError(f"stack_levels: level model {i} differs from level model 0 in active_sh_degree")
    P = int(first._xyz.shape[0])
    feats = [m._language_feature.detach() for m in models]
    for i, f in enumerate(feats):
        if tuple(f.shape) != (P, 3):
            raise ValueError(f"stack_levels: level model {i} has a _language_feature of shape {tuple(f.shape)}, "
                             f"expected ({P}, 3)")
    return first, torch.stack(feats, dim=0)


def _f32(t):
    return None if t is None else _native._f32c(t.detach())


@torch.no_grad()
def render_levels(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, opt, language_features: torch.Tensor,
                  scaling_modifier=1.0, override_color=None):
    """render() (gaussian_renderer/__init__.py:19-115) for L levels at once, without a backward.

    language_features: the (L, P, 3) raw level features (stack_levels); pc supplies the geometry (its
    own language feature is not read).  Returns {"render" (3, H, W), "language_feature_images"
    (L, 3, H, W), "radii", "visibility_filter"}; level l's image equals render()'s
    "language_feature_image" under torch.no_grad() with pc._language_feature = language_features[l].
    Always runs under torch.no_grad(): no output requires grad."""
    xyz = pc.get_xyz
    P = int(xyz.shape[0])
    _native.check_level_features(language_features, P)
    if xyz.device.type != "cuda" or language_features.device.type != "cuda":
        raise RuntimeError("render_levels: inputs must be on a ROCm GPU device "
                           f"(got {xyz.device}, {language_features.device}); there is no CPU implementation")
    if not opt.include_feature:
        raise ValueError("render_levels: needs opt.include_feature")
    rs = camera_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, True)
    lf = language_features.detach()
    if _fusable(pc, pipe, override_color, xyz.device):
        raw = _native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS | _native.RAW_LANGUAGE
        rest = pc._features_rest if pc._features_rest.numel() > 0 else None
        _, color, langs, radii, visible = _native.rasterize_gaussians_levels(
            rs, _f32(xyz), _f32(pc._features_dc), None, lf, _f32(pc._opacity), _f32(pc._scaling), _f32(pc._rotation),
            None, raw=raw, shs_rest=_f32(rest), with_visibility=True)
        return {"render": color, "language_feature_images": langs, "radii": radii, "visibility_filter": visible}

    # the unfused call of render(): activated inputs, the language normalisation in torch
    _, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp = unfused_inputs(
        viewpoint_camera, pc, pipe, scaling_modifier, override_color)
    # per level, on a contiguous (P, 3) tensor: the very operations (and reduction shapes) of render()
    lf = torch.stack([x / (x.norm(dim=-1, keepdim=True) + 1e-9) for x in _f32(lf)], dim=0)
    _, color, langs, radii = _native.rasterize_gaussians_levels(
        rs, _f32(xyz), _f32(shs), _f32(colors_precomp), lf, _f32(opacity), _f32(scales), _f32(rotations),
        _f32(cov3D_precomp), raw=0)
    return {"render": color, "language_feature_images": langs, "radii": radii, "visibility_filter": radii > 0}


def split_levels(language_features: torch.Tensor):
    """The L (P, 3) level features of an (L, P, 3) stack, detached contiguous copies: the inverse of
    stack_levels' second result, for writing <model>_1/_2/_3 (train.py:222)."""
    if not isinstance(language_features, torch.Tensor) or language_features.dim() != 3 \
            or int(language_features.shape[2]) != 3:
        raise ValueError("split_levels: language_features must have shape (L, P, 3)")
    return [f.detach().clone().contiguous() for f in language_features]


class _LevelsTrain(torch.autograd.Function):
    """lsr_forward_levels and its one backward, lsr_backward_levels, over the (L, P, 3) level features
    (raw iff raw has RAW_LANGUAGE).  Outputs: the maps, the (L,) masked-L1 losses (empty without
    targets) and, without gradients, the colour image, radii and visibility."""

    @staticmethod
    def forward(ctx, feats, rs, inputs, raw, gts, masks):
        out = _native.rasterize_gaussians_levels(rs, *inputs[:3], feats, *inputs[3:7], raw=raw, shs_rest=inputs[7],
                                                 with_visibility=True, keep_state=True)
        nr, color, langs, radii, visible, geom, binning, image = out
        L = int(langs.shape[0])
        if gts is not None:
            from .loss import masked_l1_loss  # the stand-alone kernel: masked_l1_loss's value bit for bit
            l1 = torch.stack([masked_l1_loss(langs[l], gts[l], masks[l]) for l in range(L)])
        else:
            l1 = langs.new_empty((0,))
        ctx.save_for_backward(feats, langs, radii, geom, binning, image, gts, masks)
        ctx.call = (rs, nr, raw)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(color, radii, visible)
        return langs, l1, color, radii, visible

    @staticmethod
    def backward(ctx, g_langs, g_l1, *_unused):
        feats, langs, radii, geom, binning, image, gts, masks = ctx.saved_tensors
        rs, nr, raw = ctx.call
        fused = g_l1 is not None and gts is not None
        if g_langs is None and not fused:
            return (None,) * 6
        grad = _native.rasterize_gaussians_levels_backward(
            rs, feats, radii, nr, geom, binning, image, raw=raw, grad_images=g_langs,
            images=langs if fused else None, targets=gts if fused else None, masks=masks if fused else None,
            grad_losses=g_l1 if fused else None)
        return (grad,) + (None,) * 5


def _check_targets(language_targets, L, H, W, device):
    if not isinstance(language_targets, (tuple, list)) or len(language_targets) != 2:
        raise ValueError("render_levels_train: language_targets must be (gts, masks)")
    gts, masks = language_targets
    if tuple(gts.shape) != (L, 3, H, W) or gts.dtype != torch.float32:
        raise ValueError(f"render_levels_train: gts must be fp32 of shape ({L}, 3, {H}, {W}), got {tuple(gts.shape)}")
    if masks.numel() != L * H * W or masks.dtype != torch.bool:
        raise ValueError(f"render_levels_train: masks must be bool of shape ({L}, {H}, {W}), got {tuple(masks.shape)}")
    if gts.device != device or masks.device != device:
        raise RuntimeError("render_levels_train: the targets must be on the features' device")
    return gts.detach().contiguous(), masks.detach().reshape(L, H, W).contiguous()


def render_levels_train(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, opt, language_features: torch.Tensor,
                        scaling_modifier=1.0, override_color=None, language_targets=None):
    """render(..., language_target=...) for L levels at once, differentiable in language_features alone.

    language_features: the (L, P, 3) raw level features, the leaf that requires grad; pc supplies the
    frozen geometry (its own language feature is not read).  Returns {"render" (3, H, W), detached,
    "language_feature_images" (L, 3, H, W), bit-identical to render_levels', "radii",
    "visibility_filter"}, and with language_targets = (gts (L, 3, H, W), masks (L, H, W) bool) also
    "language_l1" (L,): language_l1[l] equals loss.masked_l1_loss(images[l], gts[l], masks[l]) bit for
    bit.  A backward through language_l1 forms the loss's gradient inside the gradient kernel (no
    (L, 3, H, W) gradient image); one through the images passes theirs; both add.  One geometry pass,
    one compositing walk and one gradient walk serve every level (include/lsr.h lsr_backward_levels).

    Raises ValueError for a wrong shape or if a geometry parameter of pc requires grad while grad is
    enabled (the geometry is frozen: nothing here produces its gradient), RuntimeError for CPU tensors."""
    xyz = pc.get_xyz
    P = int(xyz.shape[0])
    L = _native.check_level_features(language_features, P)
    if xyz.device.type != "cuda" or language_features.device.type != "cuda":
        raise RuntimeError("render_levels_train: inputs must be on a ROCm GPU device "
                           f"(got {xyz.device}, {language_features.device}); there is no CPU implementation")
    if torch.is_grad_enabled():
        for name in _GEOMETRY:
            t = getattr(pc, name, None)
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f"render_levels_train: pc.{name} requires grad, but the geometry is frozen in the "
                                 "language stage and no gradient is produced for it; detach it or call "
                                 "requires_grad_(False)")
    if not opt.include_feature:
        raise ValueError("render_levels_train: needs opt.include_feature")
    rs = camera_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, True)
    H, W = int(rs.image_height), int(rs.image_width)
    gts, masks = (None, None) if language_targets is None else _check_targets(language_targets, L, H, W, xyz.device)
    lf = language_features
    if lf.dtype != torch.float32 or not lf.is_contiguous():
        lf = lf.to(torch.float32).contiguous()
    if _fusable(pc, pipe, override_color, xyz.device):
        raw = _native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS | _native.RAW_LANGUAGE
        rest = pc._features_rest if pc._features_rest.numel() > 0 else None
        inputs = (_f32(xyz), _f32(pc._features_dc), None, _f32(pc._opacity), _f32(pc._scaling), _f32(pc._rotation),
                  None, _f32(rest))
    else:
        raw = 0
        _, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp = unfused_inputs(
            viewpoint_camera, pc, pipe, scaling_modifier, override_color)
        inputs = (_f32(xyz), _f32(shs), _f32(colors_precomp), _f32(opacity), _f32(scales), _f32(rotations),
                  _f32(cov3D_precomp), None)
        # render_levels' normalisation, per level on a contiguous (P, 3) tensor; autograd chains it
        lf = torch.stack([x / (x.norm(dim=-1, keepdim=True) + 1e-9) for x in lf], dim=0)
    langs, l1, color, radii, visible = _LevelsTrain.apply(lf, rs, inputs, raw, gts, masks)
    pkg = {"render": color, "language_feature_images": langs, "radii": radii, "visibility_filter": visible}
    if language_targets is not None:
        pkg["language_l1"] = l1
    return pkg


class LevelsStep:
    """One joint training step of all levels: render_levels_train, the summed per-level losses'
    backward, Adam, zero_grad.  language_features is the one (L, P, 3) torch.nn.Parameter of
    `optimizer`, a langsplat_amd.optim.Adam; Adam is element-wise, so the step is each level's own
    Adam step (scene/gaussian_model.py:203-217 per level model).  Eager: one host wait per step."""

    def __init__(self, pc, language_features: torch.nn.Parameter, optimizer):
        from .optim import Adam
        if not isinstance(language_features, torch.nn.Parameter):
            raise ValueError("LevelsStep: language_features must be a torch.nn.Parameter")
        _native.check_level_features(language_features, int(pc.get_xyz.shape[0]))
        if not isinstance(optimizer, Adam):
            raise ValueError("LevelsStep: optimizer must be a langsplat_amd.optim.Adam")
        params = [p for g in optimizer.param_groups for p in g["params"]]
        if len(params) != 1 or params[0] is not language_features:
            raise ValueError("LevelsStep: language_features must be the optimizer's one parameter")
        self.pc, self.language_features, self.optimizer = pc, language_features, optimizer

    def step(self, camera, pipe, bg, opt, gts, masks) -> torch.Tensor:
        """One step on one view; returns the (L,) losses before the update, detached."""
        pkg = render_levels_train(camera, self.pc, pipe, bg, opt, self.language_features,
                                  language_targets=(gts, masks))
        losses = pkg["language_l1"]
        losses.sum().backward()
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        return losses.detach()


__all__ = ["stack_levels", "split_levels", "render_levels", "render_levels_train", "LevelsStep"]
