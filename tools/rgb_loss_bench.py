"""The RGB stage's loss: the fused kernels against the torch composition (measurement aid).

    python3 tools/rgb_loss_bench.py [--out profiles/rgb_loss_bench.json] [--steps 40]

On the same GPU in the same run:
 (a) the loss forward + backward alone at 1920x1080, 1264x832 and 1280x720 (C = 3), image a leaf
     that requires grad:
       fused   langsplat_amd.rgb_loss (lsr_rgb_loss_forward + lsr_rgb_loss_backward)
       torch   0.8 * L1 + 0.2 * (1 - bench.ssim) and autograd, under
               torch.backends.cudnn.flags(enabled=False) (bench.RGBStep's loss as it stands)
     5 warm-up calls, then the median of 20 calls timed with device events; each path's peak
     allocated bytes above what is live before the call; the fused forward alone (no gradient);
     the fused calls again as the replay of a captured HIP graph (the kernels without the host work
     between them); the kernels' byte model (44 B per pixel for the pair) over the
     fused times.
 (b) the whole RGB step at C3 (1M Gaussians, 1920x1080): bench.RGBStep as it stands against a
     subclass whose loss is rgb_loss, with bench.py's timing loop for that step (3 warm-up steps,
     synchronize, wall clock over --steps steps, synchronize).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, CALLS = 5, 20
SIZES = ((1920, 1080), (1264, 832), (1280, 720))
LAMBDA = 0.2
# lsr_rgb_loss_forward reads image + target (8) and writes three maps (12); the backward reads the
# maps (12) and both images (8) and writes the gradient (4)
BYTES_PER_PIXEL = {"forward": 8, "forward_with_maps": 20, "backward": 24}


def measure(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def captured(fn):
    """fn captured in a HIP graph on a side stream (after two eager calls there): the replay."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g.replay


def peak_bytes(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def loss_rows(dev):
    import torch

    import bench
    from langsplat_amd import rgb_loss
    rows = []
    for (W, H) in SIZES:
        gen = torch.Generator().manual_seed(11)
        image = torch.rand((3, H, W), generator=gen).to(dev).requires_grad_(True)
        gt = torch.rand((3, H, W), generator=gen).to(dev)

        def fused():
            image.grad = None
            loss = rgb_loss(image, gt, LAMBDA)
            loss.backward()
            return loss

        def composed():
            image.grad = None
            with torch.backends.cudnn.flags(enabled=False):
                loss = (1.0 - LAMBDA) * torch.abs(image - gt).mean() + LAMBDA * (1.0 - bench.ssim(image, gt))
                loss.backward()
            return loss

        def fused_forward():
            with torch.no_grad():
                return rgb_loss(image, gt, LAMBDA)

        lf = float(fused().detach())
        gf = image.grad.clone()
        lt = float(composed().detach())
        gdiff = float((gf - image.grad).abs().max() * image.numel())
        f_med, f_min = measure(fused)
        t_med, t_min = measure(composed)
        ff_med, _ = measure(fused_forward)
        g_med, g_min = measure(captured(fused))       # the kernels alone: no host work between them
        gf_med, _ = measure(captured(fused_forward))
        f_peak, t_peak = peak_bytes(fused), peak_bytes(composed)
        px = 3 * H * W
        pair_bytes = px * (BYTES_PER_PIXEL["forward_with_maps"] + BYTES_PER_PIXEL["backward"])
        row = {"width": W, "height": H, "channels": 3, "lambda_dssim": LAMBDA,
               "fused_ms_median": round(f_med, 4), "fused_ms_min": round(f_min, 4),
               "torch_ms_median": round(t_med, 4), "torch_ms_min": round(t_min, 4),
               "fused_no_slower": bool(f_med <= t_med),
               "fused_forward_only_ms_median": round(ff_med, 4),
               "fused_graph_replay_ms_median": round(g_med, 4), "fused_graph_replay_ms_min": round(g_min, 4),
               "fused_forward_only_graph_replay_ms_median": round(gf_med, 4),
               "fused_peak_bytes": f_peak, "torch_peak_bytes": t_peak,
               "model_bytes_pair": pair_bytes,
               "achieved_gb_s_pair": round(pair_bytes / (f_med * 1e-3) / 1e9, 1),
               "achieved_gb_s_pair_graph_replay": round(pair_bytes / (g_med * 1e-3) / 1e9, 1),
               "achieved_gb_s_forward_only_graph_replay": round(px * BYTES_PER_PIXEL["forward"] / (gf_med * 1e-3) / 1e9, 1),
               "loss_fused": lf, "loss_torch": lt, "max_abs_N_grad_difference": gdiff,
               "warmup": WARMUP, "calls": CALLS}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del image, gt, gf
    return rows


def step_row(dev, steps, cfg="C3"):
    import torch

    import bench
    from langsplat_amd import _native, rgb_loss
    from langsplat_amd.synthetic import CONFIGS, make_cameras, make_gaussians

    class FusedRGBStep(bench.RGBStep):
        """bench.RGBStep with the loss of train.py:100-103 as rgb_loss (one rank)."""

        def __call__(self):
            pkg = bench.render(self.cam, self.model, bench.Pipe, self.bg, bench.OptRGB)
            loss = rgb_loss(pkg["render"], self.gt, bench.OptRGB.lambda_dssim)
            loss.backward()
            _native.densification_stats(pkg["radii"], pkg["viewspace_points"].grad, self.max_radii2D,
                                        self.xyz_gradient_accum, self.denom)
            self.optim.step()
            self.optim.zero_grad(set_to_none=True)
            return loss

    c = CONFIGS[cfg]
    P, W, H = c["P"], c["width"], c["height"]
    cam = make_cameras(c["views"], W, H, device=dev)[0]
    gtimg = torch.rand((3, H, W), generator=torch.Generator().manual_seed(200)).to(dev)
    out = {"config": cfg, "P": P, "width": W, "height": H, "steps": steps}
    for name, cls in (("torch", bench.RGBStep), ("fused", FusedRGBStep)):
        rgb = cls(make_gaussians(P, seed=0, sh_degree=c["sh_degree"]).to(dev), cam, gtimg)
        for _ in range(3):
            loss = rgb()
        torch.cuda.synchronize()
        out[f"loss_after_warmup_{name}"] = float(loss)
        t0 = time.perf_counter()
        for _ in range(steps):
            rgb()
        torch.cuda.synchronize()
        out[f"ms_per_step_rgb_{name}"] = round(1000.0 * (time.perf_counter() - t0) / steps, 4)
        del rgb
    out["fused_no_slower"] = bool(out["ms_per_step_rgb_fused"] <= out["ms_per_step_rgb_torch"])
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_loss_bench.json"))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--config", default="C3")
    args = ap.parse_args(argv)
    import torch
    dev = torch.device("cuda", 0)
    rows = loss_rows(dev)
    step = step_row(dev, args.steps, args.config)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "loss": rows, "step": step}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
