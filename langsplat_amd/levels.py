"""All language levels of a scene in one rasterizer pass (include/lsr.h lsr_forward_levels).

LangSplat trains its semantic levels from one RGB checkpoint with the geometry frozen
(scene/gaussian_model.py:203-217; train.py:222 writes <model>_1/_2/_3), so the level models differ
only in `_language_feature`, and evaluation stacks their rendered maps
(eval/evaluate_iou_loc.py:258-266).  stack_levels checks that and stacks the features;
render_levels is render()'s glue for one inference forward that returns every level's map, each
bit-identical to render()'s for that level.

Inference only: there is no backward.  There is no CPU path: a CPU tensor raises.
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


__all__ = ["stack_levels", "render_levels"]
