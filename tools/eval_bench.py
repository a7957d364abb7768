"""LERF evaluation: the fused kernels against a composition of torch ops (measurement aid).

    python3 tools/eval_bench.py [--out profiles/eval_bench.json]

At 832x1264 (the reference's evaluation size) and 1920x1080, 3 levels x {1, 8} prompts, on the same GPU
in the same run, activate_stream + lerf_localization of one frame's relevancy:
  fused   langsplat_amd.lerf_eval (lsr_eval_filter + lsr_eval_masks, then a few small torch ops)
  torch   the same results from torch ops: reflect F.pad (15, 14, 15, 14) + avg_pool2d(30, stride 1);
          elementwise ops with amin / amax for the blend, the normalisation and the threshold; the
          majority filter as avg_pool2d(7, stride 1) over the zero-padded raw mask with its last row
          and column cleared (they are in no window), compared with the precomputed window sizes;
          sums for the counts.  The level choice, torch.nonzero and the host box test are the
          fused path's own code in both.
Each: 5 warm-up calls, then the median of 20 calls timed with device events (both paths end with
lerf_localization's copy of the coordinates to the host).  filter_call / masks_call are one
lsr_eval_filter (avg and blend written) and one lsr_eval_masks (with counts) over all maps, through
the binding.  Also reports how many mask pixels differ
(a pixel within rounding of the threshold may: avg_pool2d sums in another order).
The reference's own host path (cv2.filter2D and the Python loop of smooth()) is not measured here.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, CALLS = 5, 20


def window_sizes(H, W, device):
    """smooth()'s window size per pixel: rows max(0, i-3) .. min(i+4, H-1) - 1, the same for columns."""
    import torch
    i, j = torch.arange(H, device=device), torch.arange(W, device=device)
    rows = torch.clamp(i + 4, max=H - 1) - torch.clamp(i - 3, min=0)
    cols = torch.clamp(j + 4, max=W - 1) - torch.clamp(j - 3, min=0)
    return (rows[:, None] * cols[None, :]).to(torch.float32)


def torch_composition(vm, gt, thresh, bboxes, sizes):
    import torch
    import torch.nn.functional as F
    from langsplat_amd import lerf_eval
    L, P, H, W = vm.shape
    x = vm.reshape(L * P, 1, H, W)
    avg = F.avg_pool2d(F.pad(x, (15, 14, 15, 14), mode="reflect"), 30, stride=1)
    blend = 0.5 * (avg + x)
    mn, mx = blend.amin(dim=(2, 3), keepdim=True), blend.amax(dim=(2, 3), keepdim=True)
    o = (blend - mn) / ((mx - mn) + 1e-9)
    o = torch.clip(o * 2.0 + (-1.0), 0, 1)
    raw = (o > thresh).to(torch.float32)
    raw[:, :, H - 1, :] = 0
    raw[:, :, :, W - 1] = 0
    ones = F.avg_pool2d(F.pad(raw, (3, 3, 3, 3)), 7, stride=1) * 49.0
    masks = (2.0 * torch.round(ones) > sizes).view(L, P, H, W)
    g = (gt != 0)[None]
    counts = torch.stack([(g & masks).sum(dim=(2, 3)), (g | masks).sum(dim=(2, 3))], dim=-1)
    levels = lerf_eval._first_argmax_over_levels(mx.view(L, P))
    iou_levels = counts[..., 0].double() / counts[..., 1].double()
    act = {"levels": levels, "masks": masks.to(torch.uint8), "counts": counts,
           "iou": iou_levels.gather(0, levels[None])[0]}
    f = {"avg": avg.view(L, P, H, W), "avg_max": avg.amax(dim=(2, 3)).view(L, P)}
    return act, lerf_eval._localize(vm, f, bboxes)


def measure(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from langsplat_amd import lerf_eval
    dev = torch.device("cuda", 0)
    rows, L, thresh = [], 3, 0.4
    for (W, H) in ((1264, 832), (1920, 1080)):
        for P in (1, 8):
            gen = torch.Generator().manual_seed(3)
            # relevancy-like: a smooth field (a small random map upsampled) plus noise, in (0, 1)
            low = torch.rand((L * P, 1, H // 32 + 2, W // 32 + 2), generator=gen)
            vm = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
            vm = (0.15 + 0.7 * vm + 0.05 * torch.randn((L * P, 1, H, W), generator=gen)).clamp(0.01, 0.99)
            vm = vm.view(L, P, H, W).to(dev).contiguous()
            gt = torch.zeros((P, H, W), dtype=torch.uint8, device=dev)
            gt[:, H // 4:H // 2, W // 4:W // 2] = 1
            bboxes = [np.array([[W // 4, H // 4, W // 2, H // 2]])] * P
            sizes = window_sizes(H, W, dev)

            def fused():
                return lerf_eval.activate_stream(vm, gt, thresh), lerf_eval.lerf_localization(vm, bboxes)

            def composed():
                return torch_composition(vm, gt, thresh, bboxes, sizes)

            with torch.no_grad():
                f_med, f_min, (fa, fl) = measure(fused)
                t_med, t_min, (ta, tl) = measure(composed)
                # the two kernels alone, into preallocated outputs (binding included)
                f = lerf_eval._filter(vm, True, True)
                bufs = (f["avg"], f["blend"], f["stats"])
                mbufs = (torch.empty_like(fa["masks"]), None, torch.empty_like(fa["counts"]).view(-1, 2))
                k_filter, _, _ = measure(lambda: lerf_eval._filter(vm, True, True, out=bufs))
                k_masks, _, _ = measure(lambda: lerf_eval._masks(f["blend"], f["stats"], thresh, gt, False, out=mbufs))
            row = {"width": W, "height": H, "levels": L, "n_prompts": P, "thresh": thresh,
                   "fused_ms_median": round(f_med, 4), "fused_ms_min": round(f_min, 4),
                   "torch_ms_median": round(t_med, 4), "torch_ms_min": round(t_min, 4),
                   "fused_no_slower": bool(f_med <= t_med),
                   "filter_call_ms_median": round(k_filter, 4), "masks_call_ms_median": round(k_masks, 4),
                   "mask_pixels_differing": int((fa["masks"] != ta["masks"]).sum()),
                   "mask_pixels_set": int(fa["masks"].sum()),
                   "levels_equal": bool(torch.equal(fa["levels"], ta["levels"])),
                   "hits_equal": bool((fl["hits"] == tl["hits"]).all()),
                   "warmup": WARMUP, "calls": CALLS}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del vm, fa, ta
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")
    assert np.isfinite([r["fused_ms_median"] for r in rows]).all()


if __name__ == "__main__":
    main()
