"""The joint training step of all language levels against one eager step per level (measurement aid).

    python3 tools/levels_train_bench.py [--out profiles/levels_train_bench.json] [--configs C3 C2]

On the same model (bench.Model over the synthetic scene of the config, one camera, bench.py's targets
and Adam settings), on the same GPU in the same process, for L = 1, 2, 3, 4:
  joint   langsplat_amd.levels.LevelsStep.step: one geometry pass, one compositing walk carrying 3 L
          channels, L stand-alone masked-L1 kernels, one gradient walk (lsr_backward_levels, the loss
          seed formed inside it), one Adam launch over the (L, P, 3) parameter
  eager   L single-level steps as bench.py's eager step makes them: render(..., language_target=...)
          (fused loss), backward, Adam, zero_grad -- each level its own parameter and optimiser
  kernel  the gradient kernel's own launch (the profiler's events around "render levels grad"), in
          separate joint steps so the events are outside the timed ones
Each: 5 warm-up steps, then the median of 20 steps timed with device events around the whole step (the
forward's one host wait is inside both forms).  The forms alternate per L, and the joint form is
measured again after the eager one, so a clock or thermal drift shows.  Per L also: the accumulator's
bytes, an upper bound of the atomic-add bytes of one launch (every list instance flushing a full row:
num_rendered x 12 L bytes; only the pairs some lane blended are flushed) and the time that bound takes
at the chip-wide float-atomic rate of 1.3 TB/s.

At C3, as information, both sides of the linearity identity per level in float64,
    sum_k a[l][k] . dL/da[l][k]  =  sum_pixels I[l] . g[l]
(a the activated features, I their maps, g a random map gradient): the gradient is linear in a and the
maps are sum_k w_k a_k, so the two agree up to fp32 rounding -- a full-size check that needs no oracle.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, STEPS = 5, 20
ATOMIC_RATE = 1.3e12  # bytes / s of global float atomic adds, chip-wide (MI355X)


def measure(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_train_bench.json"))
    ap.add_argument("--configs", nargs="+", default=["C3", "C2"])
    args = ap.parse_args(argv)
    import torch

    import bench
    from langsplat_amd import _native
    from langsplat_amd.levels import LevelsStep
    from langsplat_amd.optim import Adam
    from langsplat_amd.render import camera_settings, render
    from langsplat_amd.synthetic import CONFIGS, make_cameras, make_gaussians
    dev = torch.device("cuda", 0)
    lib = _native.load()
    rows, identity = [], []
    for name in args.configs:
        c = CONFIGS[name]
        P, W, H = c["P"], c["width"], c["height"]
        model = bench.Model(make_gaussians(P, seed=0).to(dev), include_feature=True)
        cam = make_cameras(1, W, H, device=dev)[0]
        bg = torch.zeros(3, device=dev)
        LMAX = _native.MAX_LEVELS
        feats = torch.stack([torch.randn((P, 3), generator=torch.Generator().manual_seed(100 + l))
                             for l in range(LMAX)]).to(dev)
        gen = torch.Generator().manual_seed(100)  # bench.py's targets, one set per level
        gts = torch.nn.functional.normalize(torch.randn((LMAX, 3, H, W), generator=gen), dim=1).to(dev)
        masks = (torch.rand((LMAX, H, W), generator=gen) < 0.9).to(dev)

        # one forward with its state kept: the view's instance count, and the identity's inputs below
        rs = camera_settings(cam, model, bench.Pipe, bg, 1.0, True)
        act = torch.stack([x / (x.norm(dim=-1, keepdim=True) + 1e-9) for x in feats[:3]])
        with torch.no_grad():
            state = _native.rasterize_gaussians_levels(
                rs, model._xyz.detach(), model._features_dc.detach(), None, act, model._opacity.detach(),
                model._scaling.detach(), model._rotation.detach(), None,
                raw=_native.RAW_OPACITY | _native.RAW_SCALES | _native.RAW_ROTATIONS,
                shs_rest=model._features_rest.detach(), keep_state=True)
        nr = state[0]

        def adam(p):  # scene/gaussian_model.py:203-229 as bench.py sets it
            return Adam([{"params": [p], "lr": 0.0025, "name": "language_feature"}], lr=0.0, eps=1e-15)

        for L in (3, 1, 2, 4):
            joint_p = torch.nn.Parameter(feats[:L].clone())
            joint = LevelsStep(model, joint_p, adam(joint_p))
            g_l, m_l = gts[:L].contiguous(), masks[:L].contiguous()
            eager_p = [torch.nn.Parameter(feats[l].clone()) for l in range(L)]
            eager_o = [adam(p) for p in eager_p]

            def joint_step():
                return joint.step(cam, bench.Pipe, bg, bench.Opt, g_l, m_l)

            def eager_steps():
                for l in range(L):
                    model._language_feature = eager_p[l]
                    loss = render(cam, model, bench.Pipe, bg, bench.Opt,
                                  language_target=(gts[l], masks[l][None]))["language_l1"]
                    loss.backward()
                    eager_o[l].step()
                    eager_o[l].zero_grad(set_to_none=True)

            j_med, j_min, j_max = measure(joint_step)
            e_med, e_min, e_max = measure(eager_steps)
            j_med2, j_min2, j_max2 = measure(joint_step)
            _native.profile_enable(True, stages=["render levels grad", "levels grad epilogue"])
            for _ in range(STEPS):
                joint_step()
            torch.cuda.synchronize()
            rep = _native.profile_report()
            _native.profile_enable(False)
            bound = nr * 12 * L
            row = {"config": name, "P": P, "width": W, "height": H, "levels": L,
                   "joint_ms_median": round(j_med, 4), "joint_ms_min": round(j_min, 4), "joint_ms_max": round(j_max, 4),
                   "joint_again_ms_median": round(j_med2, 4),
                   "eager_ms_median": round(e_med, 4), "eager_ms_min": round(e_min, 4), "eager_ms_max": round(e_max, 4),
                   "eager_over_joint": round(e_med / max(j_med, j_med2), 3),
                   "joint_faster": bool(max(j_med, j_med2) < e_med),
                   "grad_kernel_ms": round(rep.get("render levels grad", {}).get("avg_ms", float("nan")), 4),
                   "grad_epilogue_ms": round(rep.get("levels grad epilogue", {}).get("avg_ms", float("nan")), 4),
                   "num_rendered": int(nr), "accumulator_bytes": int(lib.lsr_backward_levels_bytes(P, L)),
                   "atomic_bytes_upper_bound": int(bound),
                   "atomic_bound_ms_at_1p3_TBps": round(bound / ATOMIC_RATE * 1e3, 4),
                   "warmup": WARMUP, "steps": STEPS}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del joint, joint_p, eager_p, eager_o

        if name == "C3":  # the linearity identity, on the activated features (raw = 0 for the language)
            L = 3
            _, _, maps, radii, geom, binning, image = state
            with torch.no_grad():
                g = torch.randn((L, 3, H, W), generator=torch.Generator().manual_seed(7)).to(dev)
                grad = _native.rasterize_gaussians_levels_backward(rs, act, radii, nr, geom, binning, image,
                                                                   grad_images=g)
            for l in range(L):
                lhs = float((act[l].double() * grad[l].double()).sum())
                rhs = float((maps[l].double() * g[l].double()).sum())
                identity.append({"config": name, "level": l, "sum_a_dLda": lhs, "sum_I_g": rhs,
                                 "relative_difference": abs(lhs - rhs) / max(abs(rhs), 1e-30)})
                print(json.dumps(identity[-1]), flush=True)
        del model, feats, gts, masks
        torch.cuda.empty_cache()
    rows.sort(key=lambda r: (args.configs.index(r["config"]), r["levels"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows, "linearity_identity": identity}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
