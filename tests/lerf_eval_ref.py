"""CPU references for the LERF evaluation kernels (lsr_eval_filter / lsr_eval_masks, include/lsr.h):
what eval/evaluate_iou_loc.py:90-217 and eval/utils.py:46-55 compute after get_max_across.

  box_f64            cv2.filter2D(map, -1, ones((30, 30)) / 900) restated in fp64: a correlation with
                     the anchor at 15 (taps -15 .. +14 in both axes), BORDER_REFLECT_101 with the
                     general period 2 (n - 1)
  box_torch32        the fp32 yardstick: reflect F.pad (15, 14, 15, 14) + conv2d with a 1/900 kernel
  normalise_threshold_f32   the reference's fp32 normalise / clip / threshold sequence (:129-135)
  smooth_closed_form        eval/utils.py smooth() in closed form, quirks included
  pipeline_f64       activate_stream + lerf_localization on fp64 maps
  relevancy_like     the seeded generator of relevancy-like maps
"""
from functools import lru_cache

import numpy as np

KSIZE, ANCHOR = 30, 15  # tap offsets -ANCHOR .. KSIZE - 1 - ANCHOR = -15 .. +14


def reflect101(i, n):
    """BORDER_REFLECT_101 of index (array) i into [0, n): gfedcb|abcdefgh|gfedcba, period 2 (n - 1)."""
    i = np.asarray(i, dtype=np.int64)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def pad_reflect(x):
    """x (..., H, W) -> (..., H + 29, W + 29): 15 reflected samples before, 14 after, on both axes."""
    H, W = x.shape[-2:]
    iy = reflect101(np.arange(-ANCHOR, H + KSIZE - 1 - ANCHOR), H)
    ix = reflect101(np.arange(-ANCHOR, W + KSIZE - 1 - ANCHOR), W)
    return x[..., iy[:, None], ix[None, :]]


def box_f64(x):
    """The 30 x 30 mean filter of x (..., H, W) in fp64: 900 taps summed directly, scaled once."""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    pad = pad_reflect(x)
    acc = np.zeros_like(x)
    for dy in range(KSIZE):
        for dx in range(KSIZE):
            acc += pad[..., dy:dy + H, dx:dx + W]
    return acc / float(KSIZE * KSIZE)


def box_torch32(x):
    """The fp32 yardstick (torch, CPU).  F.pad's reflect mode needs a pad smaller than the axis, so
    maps with an axis under 16 are reflected by index first."""
    import torch
    import torch.nn.functional as F
    x = np.ascontiguousarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    t = torch.from_numpy(x).reshape(-1, 1, H, W)
    if H >= 16 and W >= 16:
        t = F.pad(t, (ANCHOR, KSIZE - 1 - ANCHOR, ANCHOR, KSIZE - 1 - ANCHOR), mode="reflect")
    else:
        t = torch.from_numpy(np.ascontiguousarray(pad_reflect(x))).reshape(-1, 1, H + KSIZE - 1, W + KSIZE - 1)
    k = torch.full((1, 1, KSIZE, KSIZE), 1.0 / (KSIZE * KSIZE), dtype=torch.float32)
    return F.conv2d(t, k).reshape(x.shape).numpy()


def normalise_threshold_f32(blend, mn, mx, thresh):
    """eval/evaluate_iou_loc.py:129-135 in numpy float32 on one map: subtract the minimum, divide by
    (max + 1e-9), map to [-1, 1], clip to [0, 1], compare with the threshold (as float32)."""
    f = np.float32
    o = np.asarray(blend, dtype=f) - f(mn)
    o = o / f(f(f(mx) - f(mn)) + f(1e-9))
    o = o * f(2.0) + f(-1.0)
    o = np.clip(o, f(0), f(1))
    assert o.dtype == np.float32
    return (o > f(thresh)).astype(np.uint8)


def smooth_closed_form(mask):
    """eval/utils.py smooth(): pixel (i, j) becomes the majority of rows max(0, i-3) .. min(i+4, H-1) - 1
    and the same column range (the upper bound exclusive and clipped to H - 1, so the last row and
    column are never inside a window); 1 exactly when 2 * ones > window size."""
    m = np.asarray(mask)
    H, W = m.shape
    ii = np.zeros((H + 1, W + 1), dtype=np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(m.astype(np.int64), axis=0), axis=1)
    r0 = np.maximum(0, np.arange(H) - 3)[:, None]
    r1 = np.minimum(np.arange(H) + 4, H - 1)[:, None]
    c0 = np.maximum(0, np.arange(W) - 3)[None, :]
    c1 = np.minimum(np.arange(W) + 4, W - 1)[None, :]
    ones = ii[r1, c1] - ii[r0, c1] - ii[r1, c0] + ii[r0, c0]
    size = (r1 - r0) * (c1 - c0)
    return (2 * ones > size).astype(m.dtype)


def relevancy_like(H, W, seed, n_maps=1):
    """(n_maps, H, W) float32 maps that look like relevancies: a base of 0.3, a few Gaussian bumps of
    amplitude 0.3-0.6 and sigma 4-12 px, noise of 0.05, clipped to (0.01, 0.99)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n_maps, H, W), dtype=np.float32)
    for m in range(n_maps):
        v = np.full((H, W), 0.3)
        for _ in range(int(rng.integers(2, 5))):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            amp, sig = rng.uniform(0.3, 0.6), rng.uniform(4.0, 12.0)
            v += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sig * sig))
        v += 0.05 * rng.standard_normal((H, W))
        out[m] = np.clip(v, 0.01, 0.99).astype(np.float32)
    return out


@lru_cache(maxsize=None)
def filter_case(H, W, seed, n_maps=1):
    """One seeded input with its references, computed once and shared (treat as read-only):
    maps, avg64 / blend64 (fp64), avg32 (the fp32 yardstick) and e_ref = max |avg32 - avg64|."""
    maps = relevancy_like(H, W, seed, n_maps)
    avg64 = box_f64(maps)
    avg32 = box_torch32(maps)
    c = {"maps": maps, "avg64": avg64, "blend64": 0.5 * (avg64 + maps.astype(np.float64)), "avg32": avg32,
         "e_ref": float(np.abs(avg32.astype(np.float64) - avg64).max())}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def normalised_f64(blend64):
    """The normalised map in [-1, 1] of one fp64 blend, before the clip."""
    mn, mx = blend64.min(), blend64.max()
    return (blend64 - mn) / ((mx - mn) + 1e-9) * 2.0 - 1.0


def pipeline_f64(valid_map, gt_masks, thresh, bboxes):
    """activate_stream and lerf_localization (eval/evaluate_iou_loc.py:90-217) on fp64 maps.
    valid_map (levels, n_prompts, H, W); gt_masks (n_prompts, H, W) uint8; bboxes: per prompt (n, 4)
    x1 y1 x2 y2.  The threshold is the float32 value the reference's comparison uses."""
    vm = np.asarray(valid_map, dtype=np.float64)
    L, P, H, W = vm.shape
    avg = box_f64(vm)
    blend = 0.5 * (avg + vm)
    t = float(np.float32(thresh))
    masks = np.zeros((L, P, H, W), dtype=np.uint8)
    counts = np.zeros((L, P, 2), dtype=np.int64)
    for i in range(L):
        for k in range(P):
            raw = (np.clip(normalised_f64(blend[i, k]), 0.0, 1.0) > t).astype(np.uint8)
            masks[i, k] = smooth_closed_form(raw)
            g = gt_masks[k].astype(bool)
            counts[i, k, 0] = np.logical_and(g, masks[i, k]).sum()
            counts[i, k, 1] = np.logical_or(g, masks[i, k]).sum()
    levels = blend.reshape(L, P, -1).max(axis=2).argmax(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.array([counts[levels[k], k, 0] / counts[levels[k], k, 1] for k in range(P)], dtype=np.float64)
    loc_levels = avg.reshape(L, P, -1).max(axis=2).argmax(axis=0)
    hits, coords = [], []
    for k in range(P):
        a = avg[loc_levels[k], k]
        ys, xs = np.nonzero(a == a.max())
        xy = np.stack([xs, ys], axis=1)
        coords.append(xy)
        hits.append(point_in_boxes(xy, bboxes[k]))
    return {"avg": avg, "blend": blend, "masks": masks, "counts": counts, "levels": levels, "iou": iou,
            "loc_levels": loc_levels, "coords": coords, "hits": np.array(hits, dtype=bool)}


def point_in_boxes(xy, boxes):
    """Some (x, y) lies inside some box, bounds inclusive, corners in either order (:192-204)."""
    for x1, y1, x2, y2 in np.asarray(boxes).reshape(-1, 4):
        x_min, x_max, y_min, y_max = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
        for x, y in xy:
            if x_min <= x <= x_max and y_min <= y <= y_max:
                return True
    return False
