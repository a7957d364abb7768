"""Open-vocabulary queries on rendered language maps -- eval/evaluate_iou_loc.py:258-266 over liblsr.so.

The reference decodes the rendered (levels, H, W, 3) maps with Autoencoder.decode
(autoencoder/model.py:42-46) into (levels, H, W, 512) CLIP-space vectors and hands them to
OpenCLIPNetwork.get_max_across (eval/openclip_encoder.py:96-112).  Here both steps are one HIP
kernel per level (include/lsr.h lsr_query_relevancy): the decoded vectors never reach HBM.  The text
encoder stays the caller's open_clip model; its unit-norm `pos_embeds` / `neg_embeds` are passed in.

get_semantic_map (eval/openclip_encoder.py:82-94), the open-vocabulary segmentation, is a second
consumer of the same on-chip similarities (lsr_query_semantic -> semantic_map: one label per pixel and
level, -1 where a canonical negative wins), and label_stats (lsr_label_stats) counts a label map
against ground truth per class on the device.

There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes
import re
from typing import Dict, Mapping, Optional, Sequence

import torch

from . import _native

MAX_LAYERS, MAX_WIDTH, MAX_PHRASES = 8, 512, 64  # include/lsr.h lsr_query_relevancy


class Decoder:
    """The autoencoder's decoder (Linear, [ReLU, Linear]*) as the one packed fp32 buffer the kernel
    reads: per layer W (out x in, row-major, nn.Linear's) then b (out)."""

    def __init__(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], device="cuda"):
        if len(weights) != len(biases) or not 1 <= len(weights) <= MAX_LAYERS:
            raise ValueError(f"Decoder: 1 to {MAX_LAYERS} layers, each with a weight and a bias")
        fan_in, parts, widths = 3, [], []
        for l, (w, b) in enumerate(zip(weights, biases)):
            w = torch.as_tensor(w).detach().to(torch.float32)
            b = torch.as_tensor(b).detach().to(torch.float32)
            if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
                raise ValueError(f"Decoder: layer {l} needs a (out, in) weight and a (out,) bias")
            out, inp = int(w.shape[0]), int(w.shape[1])
            if inp != fan_in:
                raise ValueError(f"Decoder: layer {l} has input width {inp}, expected {fan_in}"
                                 + (" (the rendered map has 3 channels)" if l == 0 else ""))
            if out % 16 != 0 or not 16 <= out <= MAX_WIDTH:
                raise ValueError(f"Decoder: layer {l} has width {out}; widths are multiples of 16, at most {MAX_WIDTH}")
            parts += [w.reshape(-1), b]
            widths.append(out)
            fan_in = out
        self.widths = widths
        self.dim = widths[-1]
        self.packed = torch.cat(parts).to(device).contiguous()
        self._widths_c = (ctypes.c_int32 * len(widths))(*widths)

    @classmethod
    def from_arrays(cls, weights, biases, device="cuda") -> "Decoder":
        """From per-layer (out, in) weight and (out,) bias arrays (numpy or torch)."""
        return cls(list(weights), list(biases), device=device)

    @classmethod
    def from_state_dict(cls, sd: Mapping[str, torch.Tensor], device="cuda") -> "Decoder":
        """From the reference checkpoint: keys decoder.{0,2,4,...}.{weight,bias} (the ModuleList's
        Linears; ReLUs sit at the odd indices, autoencoder/model.py:18-25).  The whole Autoencoder
        state dict may be passed; encoder.* is ignored."""
        idx = sorted({int(m.group(1)) for k in sd for m in [re.fullmatch(r"decoder\.(\d+)\.(weight|bias)", k)] if m})
        if not idx:
            raise ValueError("Decoder.from_state_dict: no decoder.N.weight / decoder.N.bias keys")
        if idx != list(range(0, 2 * len(idx), 2)):
            raise ValueError(f"Decoder.from_state_dict: expected Linears at decoder.0, 2, 4, ...; found {idx}")
        weights, biases = [], []
        for i in idx:
            for kind, dst in (("weight", weights), ("bias", biases)):
                key = f"decoder.{i}.{kind}"
                if key not in sd:
                    raise ValueError(f"Decoder.from_state_dict: missing {key}")
                dst.append(sd[key])
        return cls(weights, biases, device=device)


def _require_gpu(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: tensors must be on a ROCm GPU device; there is no CPU path")


def _launch(decoder: Decoder, feature: torch.Tensor, offset: int, N: int, channel_stride: int, pixel_stride: int,
            phrases: torch.Tensor, n_pos: int, n_neg: int, out: torch.Tensor, out_offset: int,
            decoded: Optional[torch.Tensor] = None):
    device = feature.device
    if N == 0:
        return
    if decoder.packed.device != device:
        raise ValueError("the decoder and the map must be on the same device")
    a = _native.LsrQueryArgs()
    a.N = N
    a.feature = feature.data_ptr() + 4 * offset
    a.channel_stride, a.pixel_stride = channel_stride, pixel_stride
    a.n_layers = len(decoder.widths)
    a.widths = decoder._widths_c
    a.weights = decoder.packed.data_ptr()
    a.n_pos, a.n_neg = n_pos, n_neg
    a.phrases = phrases.data_ptr()
    a.out_relevancy = out.data_ptr() + 4 * out_offset
    a.out_decoded = decoded.data_ptr() if decoded is not None else None
    with _native._on_device(device):
        _native._check(_native.load().lsr_query_relevancy(ctypes.byref(a), _native._stream(device)),
                       "lsr_query_relevancy")


def _launch_semantic(decoder: Decoder, feature: torch.Tensor, offset: int, N: int, channel_stride: int,
                     pixel_stride: int, phrases: torch.Tensor, n_labels: int, n_neg: int, label: torch.Tensor,
                     label_offset: int, score: Optional[torch.Tensor] = None, score_offset: int = 0):
    device = feature.device
    if N == 0:
        return
    if decoder.packed.device != device:
        raise ValueError("the decoder and the map must be on the same device")
    a = _native.LsrQuerySemanticArgs()
    a.N = N
    a.feature = feature.data_ptr() + 4 * offset
    a.channel_stride, a.pixel_stride = channel_stride, pixel_stride
    a.n_layers = len(decoder.widths)
    a.widths = decoder._widths_c
    a.weights = decoder.packed.data_ptr()
    a.n_labels, a.n_neg = n_labels, n_neg
    a.phrases = phrases.data_ptr()
    a.out_label = label.data_ptr() + 4 * label_offset
    a.out_score = score.data_ptr() + 4 * score_offset if score is not None else None
    with _native._on_device(device):
        _native._check(_native.load().lsr_query_semantic(ctypes.byref(a), _native._stream(device)),
                       "lsr_query_semantic")


def _phrases(decoder: Decoder, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor, device) -> torch.Tensor:
    # get_relevancy's torch.cat([pos, neg]).to(embed.dtype) (eval/openclip_encoder.py:44-45)
    pos = torch.as_tensor(pos_embeds).to(device=device, dtype=torch.float32)
    neg = torch.as_tensor(neg_embeds).to(device=device, dtype=torch.float32)
    if pos.dim() != 2 or neg.dim() != 2 or pos.shape[1] != decoder.dim or neg.shape[1] != decoder.dim:
        raise ValueError(f"pos_embeds / neg_embeds must be (n, {decoder.dim}) matrices of unit-norm rows")
    if pos.shape[0] < 1 or neg.shape[0] < 1 or pos.shape[0] + neg.shape[0] > MAX_PHRASES:
        raise ValueError(f"at least one positive and one negative phrase, at most {MAX_PHRASES} in all")
    return torch.cat([pos, neg], dim=0).contiguous()


def relevancy_map(sem_map: torch.Tensor, decoder: Decoder, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor,
                  layout: str = "chw") -> torch.Tensor:
    """OpenCLIPNetwork.get_max_across(Autoencoder.decode(sem_map)) -> (levels, n_pos, H, W) fp32.

    sem_map: (levels, 3, H, W), the rasterizer's layout (layout="chw"), or (levels, H, W, 3), the
    layout of the reference's renders_npy files (layout="hwc"); a single 3-D map is one level.
    One kernel launch per level on the current stream; no host synchronisation."""
    _require_gpu(sem_map, "relevancy_map")
    if layout not in ("chw", "hwc"):
        raise ValueError('relevancy_map: layout is "chw" or "hwc"')
    m = sem_map.detach()
    if m.dim() == 3:
        m = m[None]
    c_axis = 1 if layout == "chw" else 3
    if m.dim() != 4 or m.shape[c_axis] != 3:
        raise ValueError(f"relevancy_map: expected a (levels, 3, H, W) map (chw) or (levels, H, W, 3) (hwc), "
                         f"got {tuple(sem_map.shape)}")
    m = _native._f32c(m)
    levels = int(m.shape[0])
    H, W = (int(m.shape[2]), int(m.shape[3])) if layout == "chw" else (int(m.shape[1]), int(m.shape[2]))
    N = H * W
    phrases = _phrases(decoder, pos_embeds, neg_embeds, m.device)
    n_pos = int(torch.as_tensor(pos_embeds).shape[0])
    n_neg = int(phrases.shape[0]) - n_pos
    out = torch.empty((levels, n_pos, H, W), dtype=torch.float32, device=m.device)
    cs, ps = (N, 1) if layout == "chw" else (1, 3)
    for i in range(levels):
        _launch(decoder, m, 3 * N * i, N, cs, ps, phrases, n_pos, n_neg, out, n_pos * N * i)
    return out


def semantic_map(sem_map: torch.Tensor, decoder: Decoder, label_embeds: torch.Tensor, neg_embeds: torch.Tensor,
                 layout: str = "chw", return_score: bool = False, dtype: torch.dtype = torch.int64):
    """OpenCLIPNetwork.get_semantic_map(Autoencoder.decode(sem_map)) -> (levels, H, W) labels: per pixel
    the label whose embedding is most similar, -1 where one of the negatives is (the first index wins a tie).

    sem_map and layout as in relevancy_map; label_embeds (n_labels, D) and neg_embeds (n_neg, D) are
    unit-norm rows (the reference's semantic_embeds and neg_embeds).  dtype: torch.int64 (the reference's
    .long()) or torch.int32, the kernel's own buffer without a conversion.  return_score: also the
    (levels, H, W) fp32 softmax value of the winner.  One kernel launch per level on the current
    stream; no host synchronisation."""
    _require_gpu(sem_map, "semantic_map")
    if layout not in ("chw", "hwc"):
        raise ValueError('semantic_map: layout is "chw" or "hwc"')
    if dtype not in (torch.int64, torch.int32):
        raise ValueError("semantic_map: dtype is torch.int64 or torch.int32")
    m = sem_map.detach()
    if m.dim() == 3:
        m = m[None]
    c_axis = 1 if layout == "chw" else 3
    if m.dim() != 4 or m.shape[c_axis] != 3:
        raise ValueError(f"semantic_map: expected a (levels, 3, H, W) map (chw) or (levels, H, W, 3) (hwc), "
                         f"got {tuple(sem_map.shape)}")
    m = _native._f32c(m)
    levels = int(m.shape[0])
    H, W = (int(m.shape[2]), int(m.shape[3])) if layout == "chw" else (int(m.shape[1]), int(m.shape[2]))
    N = H * W
    phrases = _phrases(decoder, label_embeds, neg_embeds, m.device)
    n_labels = int(torch.as_tensor(label_embeds).shape[0])
    n_neg = int(phrases.shape[0]) - n_labels
    label = torch.empty((levels, H, W), dtype=torch.int32, device=m.device)
    score = torch.empty((levels, H, W), dtype=torch.float32, device=m.device) if return_score else None
    cs, ps = (N, 1) if layout == "chw" else (1, 3)
    for i in range(levels):
        _launch_semantic(decoder, m, 3 * N * i, N, cs, ps, phrases, n_labels, n_neg, label, N * i, score, N * i)
    if dtype != torch.int32:
        label = label.to(dtype)
    return (label, score) if return_score else label


def label_stats(pred: torch.Tensor, gt: torch.Tensor, n_classes: int) -> Dict[str, torch.Tensor]:
    """Per-class counts of predicted label maps against ground truth (include/lsr.h lsr_label_stats).

    pred: (maps, H, W) integer labels, or a single (H, W) map; gt: one (H, W) map (shared by all maps)
    or (maps, H, W).  A pixel counts only where 0 <= gt < n_classes (any other value is an
    ignore label); a prediction outside the classes (-1) on such a pixel is a miss.  Returns
    counts (maps, n_classes, 3) int64 = intersection, predicted, ground truth; totals (maps, 2) int64 =
    correct, valid; iou (maps, n_classes) float64, NaN where the union is 0; miou (maps,), the mean over
    the classes with a non-zero union; accuracy (maps,) = correct / valid.  No host synchronisation."""
    _require_gpu(pred, "label_stats")
    _require_gpu(gt, "label_stats")
    if pred.device != gt.device:
        raise ValueError("label_stats: pred and gt must be on the same device")
    if not 1 <= int(n_classes) <= MAX_PHRASES:
        raise ValueError(f"label_stats: n_classes is 1 to {MAX_PHRASES}")
    if pred.dtype.is_floating_point or gt.dtype.is_floating_point:
        raise ValueError("label_stats: pred and gt hold integer labels")
    if pred.dim() == 2:
        pred = pred[None]
    if pred.dim() != 3 or tuple(gt.shape) not in (tuple(pred.shape), tuple(pred.shape[1:])):
        raise ValueError(f"label_stats: pred is (maps, H, W) or (H, W) and gt one (H, W) map or pred's shape, "
                         f"got {tuple(pred.shape)} and {tuple(gt.shape)}")
    maps = int(pred.shape[0])
    gt_maps = maps if gt.dim() == 3 else 1
    p = pred.detach().to(torch.int32).contiguous()
    g = gt.detach().to(torch.int32).contiguous()
    N = p.numel() // maps if maps else 0
    dev = p.device
    if maps == 0 or N == 0:  # the call enqueues nothing
        counts = torch.zeros((maps, n_classes, 3), dtype=torch.int64, device=dev)
        totals = torch.zeros((maps, 2), dtype=torch.int64, device=dev)
    else:
        counts = torch.empty((maps, n_classes, 3), dtype=torch.int64, device=dev)
        totals = torch.empty((maps, 2), dtype=torch.int64, device=dev)
        _label_stats_into(p, g, N, maps, gt_maps, int(n_classes), counts, totals)
    out = {"counts": counts, "totals": totals}
    out.update(label_metrics(counts, totals))
    return out


def _label_stats_into(pred: torch.Tensor, gt: torch.Tensor, N: int, maps: int, gt_maps: int, n_classes: int,
                      counts: torch.Tensor, totals: torch.Tensor):
    a = _native.LsrLabelStatsArgs()
    a.N, a.n_maps, a.gt_maps, a.n_classes = N, maps, gt_maps, n_classes
    a.pred, a.gt = pred.data_ptr(), gt.data_ptr()
    a.out_counts, a.out_totals = counts.data_ptr(), totals.data_ptr()
    with _native._on_device(pred.device):
        _native._check(_native.load().lsr_label_stats(ctypes.byref(a), _native._stream(pred.device)),
                       "lsr_label_stats")


def label_metrics(counts: torch.Tensor, totals: torch.Tensor) -> Dict[str, torch.Tensor]:
    """iou, miou and accuracy (float64) from lsr_label_stats' count tensors, on their device."""
    inter, predicted, truth = (counts[..., i].to(torch.float64) for i in range(3))
    union = predicted + truth - inter
    seen = union > 0
    nan = torch.full_like(union, float("nan"))
    iou = torch.where(seen, inter / torch.where(seen, union, torch.ones_like(union)), nan)
    miou = torch.where(seen, iou, torch.zeros_like(iou)).sum(dim=-1) / seen.sum(dim=-1).to(torch.float64)
    accuracy = totals[..., 0].to(torch.float64) / totals[..., 1].to(torch.float64)
    return {"iou": iou, "miou": miou, "accuracy": accuracy}


def decode(features: torch.Tensor, decoder: Decoder) -> torch.Tensor:
    """Autoencoder.decode of (N, 3) features -> (N, D) unit vectors, through the query kernel's
    out_decoded.  The small-N / debugging path: it writes N x D floats, which the fused query
    exists to avoid."""
    _require_gpu(features, "decode")
    f = _native._f32c(features.detach())
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("decode: expected (N, 3) features")
    N = int(f.shape[0])
    out = torch.empty((N, decoder.dim), dtype=torch.float32, device=f.device)
    phrases = torch.zeros((2, decoder.dim), dtype=torch.float32, device=f.device)  # unused similarities
    scratch = torch.empty((1, max(N, 1)), dtype=torch.float32, device=f.device)
    _launch(decoder, f, 0, N, 1, 3, phrases, 1, 1, scratch, 0, decoded=out)
    return out


def render_relevancy(viewpoint_camera, pc, pipe, bg_color, opt, decoder: Decoder, pos_embeds, neg_embeds,
                     scaling_modifier=1.0):
    """render() without a backward (the LSR_FWD_NO_BACKWARD forward) followed by relevancy_map on its
    language_feature_image: the render package plus "relevancy", (1, n_pos, H, W)."""
    from .render import render
    with torch.no_grad():
        pkg = render(viewpoint_camera, pc, pipe, bg_color, opt, scaling_modifier=scaling_modifier)
        pkg["relevancy"] = relevancy_map(pkg["language_feature_image"], decoder, pos_embeds, neg_embeds)
    return pkg


def render_levels_relevancy(viewpoint_camera, pc, pipe, bg_color, opt, language_features, decoder: Decoder,
                            pos_embeds, neg_embeds, scaling_modifier=1.0):
    """levels.render_levels (every level's map from one rasterizer pass) followed by relevancy_map on
    them: the render_levels package plus "relevancy", (L, n_pos, H, W) -- what
    eval/evaluate_iou_loc.py:258-266 computes from the level checkpoints' rendered maps."""
    from .levels import render_levels
    with torch.no_grad():
        pkg = render_levels(viewpoint_camera, pc, pipe, bg_color, opt, language_features,
                            scaling_modifier=scaling_modifier)
        pkg["relevancy"] = relevancy_map(pkg["language_feature_images"], decoder, pos_embeds, neg_embeds)
    return pkg


def _put_semantic(pkg, images, decoder, label_embeds, neg_embeds, return_score, dtype):
    got = semantic_map(images, decoder, label_embeds, neg_embeds, return_score=return_score, dtype=dtype)
    if return_score:
        pkg["semantic"], pkg["semantic_score"] = got
    else:
        pkg["semantic"] = got
    return pkg


def render_semantic(viewpoint_camera, pc, pipe, bg_color, opt, decoder: Decoder, label_embeds, neg_embeds,
                    scaling_modifier=1.0, return_score=False, dtype=torch.int64):
    """render_relevancy's forward followed by semantic_map on its language_feature_image: the render
    package plus "semantic", (1, H, W) labels, and with return_score "semantic_score", (1, H, W)."""
    from .render import render
    with torch.no_grad():
        pkg = render(viewpoint_camera, pc, pipe, bg_color, opt, scaling_modifier=scaling_modifier)
        return _put_semantic(pkg, pkg["language_feature_image"], decoder, label_embeds, neg_embeds, return_score, dtype)


def render_levels_semantic(viewpoint_camera, pc, pipe, bg_color, opt, language_features, decoder: Decoder,
                           label_embeds, neg_embeds, scaling_modifier=1.0, return_score=False, dtype=torch.int64):
    """levels.render_levels followed by semantic_map on every level's map: the render_levels package
    plus "semantic", (L, H, W) labels, and with return_score "semantic_score", (L, H, W)."""
    from .levels import render_levels
    with torch.no_grad():
        pkg = render_levels(viewpoint_camera, pc, pipe, bg_color, opt, language_features,
                            scaling_modifier=scaling_modifier)
        return _put_semantic(pkg, pkg["language_feature_images"], decoder, label_embeds, neg_embeds, return_score,
                             dtype)
