"""LERF evaluation on the GPU -- activate_stream and lerf_localization of eval/evaluate_iou_loc.py:90-217
over liblsr.so, from get_max_across's relevancy (langsplat_amd.query.relevancy_map) onwards.

The reference takes every (level, prompt) map to the host for cv2.filter2D with a 30 x 30 mean kernel,
back for the blend and the normalisation, and to the host again for eval/utils.py's smooth(), a Python
loop over every pixel.  Here that is two kernels per frame (include/lsr.h lsr_eval_filter and
lsr_eval_masks) over all maps at once; the level choice, the IoU and the localisation coordinates are
a few small torch ops on their outputs.  Only lerf_localization brings anything to the host: the
arg-max coordinates and the chosen levels, for the box test.

The heat-map and composite images, colour maps, PNG writing, the JSON / polygon ground-truth loader
and the text encoder stay the caller's.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _native
from .query import Decoder, _require_gpu, relevancy_map


def _maps4(valid_map: torch.Tensor, what: str) -> torch.Tensor:
    _require_gpu(valid_map, what)
    if valid_map.dim() != 4:
        raise ValueError(f"{what}: expected get_max_across's (levels, n_prompts, H, W) relevancy, "
                         f"got {tuple(valid_map.shape)}")
    if valid_map.shape[2] < 2 or valid_map.shape[3] < 2:
        raise ValueError(f"{what}: H and W must be at least 2")
    return _native._f32c(valid_map.detach())


def _filter(maps: torch.Tensor, want_avg: bool, want_blend: bool, out=None) -> Dict[str, torch.Tensor]:
    """lsr_eval_filter over maps (..., H, W), fp32 contiguous on the GPU.  `out`: preallocated flat
    (avg, blend, stats) buffers (the tests' canaries)."""
    lead, (H, W) = tuple(maps.shape[:-2]), maps.shape[-2:]
    n = int(np.prod(lead, dtype=np.int64))
    dev = maps.device
    if out is None:
        avg = torch.empty(maps.shape, dtype=torch.float32, device=dev) if want_avg else None
        blend = torch.empty(maps.shape, dtype=torch.float32, device=dev) if want_blend else None
        stats = torch.empty((n, 4), dtype=torch.float32, device=dev)
    else:
        avg, blend, stats = out
    a = _native.LsrEvalFilterArgs()
    a.n_maps, a.H, a.W = n, int(H), int(W)
    a.maps = maps.data_ptr()
    a.out_avg = avg.data_ptr() if avg is not None else None
    a.out_blend = blend.data_ptr() if blend is not None else None
    a.out_stats = stats.data_ptr()
    with _native._on_device(dev):
        _native._check(_native.load().lsr_eval_filter(ctypes.byref(a), _native._stream(dev)), "lsr_eval_filter")
    rec = stats.view(-1)[:4 * n].view(n, 4)
    flat = rec.view(torch.int32)[:, 3].to(torch.int64)
    return {"avg": avg, "blend": blend, "stats": stats,
            "blend_min": rec[:, 0].reshape(lead), "blend_max": rec[:, 1].reshape(lead),
            "avg_max": rec[:, 2].reshape(lead),
            "avg_argmax": torch.stack([flat // W, flat % W], dim=-1).reshape(lead + (2,))}


def _masks(blend: torch.Tensor, stats: torch.Tensor, thresh: float, gt: Optional[torch.Tensor], want_raw: bool,
           out=None):
    """lsr_eval_masks over blend (..., H, W) -> (mask, raw mask or None, counts or None)."""
    lead, (H, W) = tuple(blend.shape[:-2]), blend.shape[-2:]
    n = int(np.prod(lead, dtype=np.int64))
    dev = blend.device
    if out is None:
        mask = torch.empty(blend.shape, dtype=torch.uint8, device=dev)
        raw = torch.empty(blend.shape, dtype=torch.uint8, device=dev) if want_raw else None
        counts = torch.empty((n, 2), dtype=torch.int64, device=dev) if gt is not None else None
    else:
        mask, raw, counts = out
    a = _native.LsrEvalMaskArgs()
    a.n_maps, a.H, a.W = n, int(H), int(W)
    a.blend, a.stats, a.thresh = blend.data_ptr(), stats.data_ptr(), float(thresh)
    a.n_prompts = int(gt.shape[0]) if gt is not None else 0
    a.gt_mask = gt.data_ptr() if gt is not None else None
    a.out_mask = mask.data_ptr()
    a.out_mask_raw = raw.data_ptr() if raw is not None else None
    a.out_counts = counts.data_ptr() if counts is not None else None
    with _native._on_device(dev):
        _native._check(_native.load().lsr_eval_masks(ctypes.byref(a), _native._stream(dev)), "lsr_eval_masks")
    return mask, raw, counts


def _first_argmax_over_levels(score: torch.Tensor) -> torch.Tensor:
    """argmax over dim 0 of (levels, n_prompts) scores, the FIRST level on ties."""
    L = score.shape[0]
    idx = torch.arange(L, device=score.device)[:, None].expand_as(score)
    return torch.where(score == score.amax(dim=0, keepdim=True), idx, L).amin(dim=0)


def _gt_bytes(gt_masks: torch.Tensor, vm: torch.Tensor, what: str) -> torch.Tensor:
    _require_gpu(gt_masks, what)
    if gt_masks.device != vm.device or tuple(gt_masks.shape) != tuple(vm.shape[1:]):
        raise ValueError(f"{what}: gt_masks must be (n_prompts, H, W) = {tuple(vm.shape[1:])} on the map's device, "
                         f"got {tuple(gt_masks.shape)}")
    g = gt_masks if gt_masks.dtype in (torch.uint8, torch.bool) else gt_masks != 0
    return g.contiguous().view(torch.uint8)  # a bool's byte is 0 / 1


def smooth_relevancy(valid_map: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The mean-filtered maps and their blend (eval/evaluate_iou_loc.py:107-112) of (..., H, W) maps:
    avg = cv2.filter2D(map, -1, ones((30, 30)) / 900), blend = 0.5 * (avg + map), and per map
    blend_min, blend_max, avg_max and avg_argmax = the first (y, x) at which avg has its maximum."""
    _require_gpu(valid_map, "smooth_relevancy")
    if valid_map.dim() < 2 or valid_map.shape[-2] < 2 or valid_map.shape[-1] < 2:
        raise ValueError("smooth_relevancy: expected (..., H, W) maps with H, W >= 2")
    f = _filter(_native._f32c(valid_map.detach()), True, True)
    del f["stats"]
    return f


def _activate(vm: torch.Tensor, f: Dict[str, torch.Tensor], gt: Optional[torch.Tensor], thresh: float):
    mask, _, counts = _masks(f["blend"], f["stats"], thresh, gt, False)
    levels = _first_argmax_over_levels(f["blend_max"])
    out = {"levels": levels, "masks": mask}
    if gt is not None:
        L, P = vm.shape[:2]
        counts = counts.view(L, P, 2)
        iou_levels = counts[..., 0].double() / counts[..., 1].double()  # 0 / 0 = nan, as the reference's
        out.update(counts=counts, iou_levels=iou_levels, iou=iou_levels.gather(0, levels[None])[0])
    return out


def activate_stream(valid_map: torch.Tensor, gt_masks: Optional[torch.Tensor] = None, thresh: float = 0.4):
    """activate_stream (eval/evaluate_iou_loc.py:90-159) without its images, on get_max_across's
    (levels, n_prompts, H, W) relevancy.  Returns a dictionary of GPU tensors:
      levels  (n_prompts,) the level with the largest max(blend), the first on ties (:146-150)
      masks   (levels, n_prompts, H, W) uint8, the thresholded and smooth()ed masks of every level
    and with gt_masks ((n_prompts, H, W), non-zero = set):
      iou         (n_prompts,) float64 intersection / union of the chosen level (nan for an empty union)
      iou_levels  (levels, n_prompts), counts (levels, n_prompts, 2) int64 intersection and union
    thresh defaults to the reference's --mask_thresh.  valid_map is not modified (the reference
    overwrites it with the blend); no host synchronisation."""
    vm = _maps4(valid_map, "activate_stream")
    gt = _gt_bytes(gt_masks, vm, "activate_stream") if gt_masks is not None else None
    return _activate(vm, _filter(vm, False, True), gt, thresh)


def _localize(vm: torch.Tensor, f: Dict[str, torch.Tensor], bboxes: Sequence):
    L, P, H, W = vm.shape
    if len(bboxes) != P:
        raise ValueError(f"lerf_localization: {len(bboxes)} box lists for {P} prompts")
    levels = _first_argmax_over_levels(f["avg_max"])
    k = torch.arange(P, device=vm.device)
    sel = f["avg"][levels, k]                                        # (P, H, W): the chosen level's avg
    kyx = torch.nonzero(sel == f["avg_max"][levels, k][:, None, None])  # rows (prompt, y, x), sorted
    kyx, levels_h = kyx.cpu().numpy(), levels.cpu().numpy()
    coords, hits = [], []
    for p in range(P):
        xy = kyx[kyx[:, 0] == p][:, :0:-1]                            # (n, 2) as (x, y) (:187)
        coords.append(np.ascontiguousarray(xy))
        hit = False
        for x1, y1, x2, y2 in np.asarray(bboxes[p]).reshape(-1, 4):
            x_min, x_max, y_min, y_max = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
            if ((xy[:, 0] >= x_min) & (xy[:, 0] <= x_max) & (xy[:, 1] >= y_min) & (xy[:, 1] <= y_max)).any():
                hit = True
                break
        hits.append(hit)
    return {"levels": levels_h, "coords": coords, "hits": np.asarray(hits, dtype=bool), "acc_num": int(sum(hits))}


def lerf_localization(valid_map: torch.Tensor, bboxes: Sequence):
    """lerf_localization (eval/evaluate_iou_loc.py:162-217) without its images.  Per prompt the level
    with the largest max(avg) (the first on ties, :189), ALL coordinates (x, y) at which that level's avg
    equals its maximum (:185-187) and whether one of them lies inside one of the prompt's boxes (bounds
    inclusive, corners in either order, :192-204).  bboxes: per prompt an (n, 4) array of x1 y1 x2 y2.
    Returns host values: levels (n_prompts,), coords (a list of (n, 2) arrays), hits (n_prompts,) bool
    and acc_num, the number of hits."""
    vm = _maps4(valid_map, "lerf_localization")
    return _localize(vm, _filter(vm, True, False), bboxes)


def evaluate_frame(sem_map: torch.Tensor, decoder: Decoder, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor,
                   gt_masks: Optional[torch.Tensor], bboxes: Sequence, thresh: float = 0.4, layout: str = "hwc"):
    """One frame of evaluate() (eval/evaluate_iou_loc.py:258-272): relevancy_map, then activate_stream
    and lerf_localization on one filter pass.  sem_map: (levels, H, W, 3), the renders_npy layout
    (layout="hwc"), or (levels, 3, H, W) (layout="chw").  Returns relevancy, chosen_level, masks, (with
    gt_masks) iou, iou_levels and counts, and loc_level, coords, hits, acc_num."""
    vm = relevancy_map(sem_map, decoder, pos_embeds, neg_embeds, layout=layout)
    gt = _gt_bytes(gt_masks, vm, "evaluate_frame") if gt_masks is not None else None
    f = _filter(vm, True, True)
    a = _activate(vm, f, gt, thresh)
    loc = _localize(vm, f, bboxes)
    out = {"relevancy": vm, "chosen_level": a.pop("levels"), "loc_level": loc.pop("levels")}
    out.update(a)
    out.update(loc)
    return out
