"""The captured joint levels step against the eager one (measurement aid).

    python3 tools/levels_graph_bench.py [--out profiles/levels_graph_bench.json] [--configs C3 C2]

tools/levels_train_bench.py's setting (bench.Model over the synthetic scene of the config, one camera,
bench.py's targets and Adam settings), on the same GPU in the same process, for L = 1, 2, 3, 4:
  eager    langsplat_amd.levels.LevelsStep.step, measured twice (before and after the captured forms: the
           spread between its two rounds is what a difference has to exceed)
  graph    langsplat_amd.levels_graph.GraphedLevelsStep.replay: G_geo + G_step, no host wait
  cached   the same with view_cache=True in its steady state (every visit a hit: one restore + G_step)
  pipe x3  L = 3 only: three PipelinedGraphStep(view_cache=True) single-level steps, one per level, each
           with its own parameter and optimiser (the strongest per-level form the package has)
Each: 5 warm-up steps, then the median of 20 steps timed with device events around the whole step.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, STEPS = 5, 20


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
    return round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_graph_bench.json"))
    ap.add_argument("--configs", nargs="+", default=["C3", "C2"])
    args = ap.parse_args(argv)
    import torch

    import bench
    from langsplat_amd import _native
    from langsplat_amd.levels import LevelsStep
    from langsplat_amd.levels_graph import GraphedLevelsStep, LevelsViewSlot
    from langsplat_amd.optim import Adam
    from langsplat_amd.pipeline import PipelinedGraphStep
    from langsplat_amd.render import render
    from langsplat_amd.synthetic import CONFIGS, make_cameras, make_gaussians
    dev = torch.device("cuda", 0)
    rows = []
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

        def adam(p):  # scene/gaussian_model.py:203-229 as bench.py sets it
            return Adam([{"params": [p], "lr": 0.0025, "name": "language_feature"}], lr=0.0, eps=1e-15)

        for L in (3, 1, 2, 4):
            g_l, m_l = gts[:L].contiguous(), masks[:L].contiguous()
            eager_p = torch.nn.Parameter(feats[:L].clone())
            eager = LevelsStep(model, eager_p, adam(eager_p))
            row = {"config": name, "P": P, "width": W, "height": H, "levels": L, "warmup": WARMUP, "steps": STEPS}

            def put(key, t):
                row[key + "_ms_median"], row[key + "_ms_min"], row[key + "_ms_max"] = t

            put("eager", measure(lambda: eager.step(cam, bench.Pipe, bg, bench.Opt, g_l, m_l)))
            for key, cached in (("graph", False), ("cached", True)):
                p = torch.nn.Parameter(feats[:L].clone())
                step = GraphedLevelsStep(model, p, adam(p), LevelsViewSlot(cam, g_l, m_l), bench.Pipe, bg, bench.Opt,
                                         view_cache=cached).capture()
                put(key, measure(step.replay))
                assert step.check(), "a bench view overflowed its capacities"
                row[key + "_geometry_replays"] = step.geo_replays
                del step, p
            if L == 3:
                pgs = []
                for l in range(L):
                    m = copy.copy(model)
                    m._language_feature = torch.nn.Parameter(feats[l].clone())
                    fwd = (lambda m=m, l=l: render(cam, m, bench.Pipe, bg, bench.Opt,
                                                   language_target=(gts[l], masks[l][None]))["language_l1"])
                    pgs.append(PipelinedGraphStep(fwd, [m._language_feature], adam(m._language_feature), model=m,
                                                  view_cache=True).capture())

                def pipelined():
                    for pg in pgs:
                        pg.replay()

                put("pipelined_x3", measure(pipelined))
                for pg in pgs:
                    pg.synchronize()
                row["pipelined_x3_view_cache"] = [pg.view_cache_stats() for pg in pgs]
                del pgs
            put("eager_again", measure(lambda: eager.step(cam, bench.Pipe, bg, bench.Opt, g_l, m_l)))
            e1, e2 = row["eager_ms_median"], row["eager_again_ms_median"]
            row["eager_spread_ms"] = round(abs(e1 - e2), 4)
            row["eager_over_cached"] = round(min(e1, e2) / row["cached_ms_median"], 3)
            row["cached_faster_than_eager_by_more_than_the_spread"] = bool(
                min(e1, e2) - row["cached_ms_median"] > abs(e1 - e2))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del eager, eager_p
            torch.cuda.empty_cache()
        del model, feats, gts, masks
        torch.cuda.empty_cache()
    rows.sort(key=lambda r: (args.configs.index(r["config"]), r["levels"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
