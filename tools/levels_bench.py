"""All language levels in one rasterizer pass against one render() per level (measurement aid).

    python3 tools/levels_bench.py [--out profiles/levels_bench.json] [--configs C3 C2]

On the same model (bench.Model over the synthetic scene of the config, one camera), on the same GPU
in the same process, under torch.no_grad():
  levels   langsplat_amd.levels.render_levels with L stacked raw level features (one preprocess, depth
           order and binning, the level fill, one compositing walk carrying 3 L language channels)
  renders  L calls of render() (the LSR_FWD_NO_BACKWARD inference forward), the model's
           _language_feature set to each level in turn before the timed region
for L = 1, 2, 3, 4.  Each: 5 warm-up calls, then the median of 20 calls timed with device events around
the whole call (so the forward's one host wait is inside both).  The two forms alternate per L, so a
clock or thermal drift reaches both.  Also reports, per L, the compositing kernel's workgroups per CU
as the HIP runtime grants them (lsr_debug_levels_occupancy), the level buffer's bytes, and that the
maps of the two forms are bit-identical.  The condition of the form: at L = 3 `levels` is faster than
`renders` at every size (it does a strict subset of their work).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, CALLS = 5, 20


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
    return statistics.median(times), min(times), max(times), r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_bench.json"))
    ap.add_argument("--configs", nargs="+", default=["C3", "C2"])
    args = ap.parse_args(argv)
    import torch

    import bench
    from langsplat_amd import _native
    from langsplat_amd.levels import render_levels
    from langsplat_amd.render import render
    from langsplat_amd.synthetic import CONFIGS, make_cameras, make_gaussians
    dev = torch.device("cuda", 0)
    lib = _native.load()
    rows = []
    for name in args.configs:
        c = CONFIGS[name]
        P, W, H = c["P"], c["width"], c["height"]
        model = bench.Model(make_gaussians(P, seed=0).to(dev), include_feature=True)
        cam = make_cameras(1, W, H, device=dev)[0]
        bg = torch.zeros(3, device=dev)
        feats = torch.stack([torch.randn((P, 3), generator=torch.Generator().manual_seed(100 + l))
                             for l in range(_native.MAX_LEVELS)]).to(dev)
        params = [torch.nn.Parameter(feats[l].clone()) for l in range(_native.MAX_LEVELS)]

        for L in (3, 1, 2, 4):
            def levels_form():
                return render_levels(cam, model, bench.Pipe, bg, bench.Opt, feats[:L])

            def renders_form():
                out = []
                for l in range(L):
                    model._language_feature = params[l]
                    out.append(render(cam, model, bench.Pipe, bg, bench.Opt)["language_feature_image"])
                return out

            with torch.no_grad():
                l_med, l_min, l_max, pkg = measure(levels_form)
                r_med, r_min, r_max, refs = measure(renders_form)
                l_med2, l_min2, l_max2, _ = measure(levels_form)  # again, after the other form: drift shows here
            same = all(torch.equal(pkg["language_feature_images"][l], refs[l]) for l in range(L))
            row = {"config": name, "P": P, "width": W, "height": H, "levels": L,
                   "levels_ms_median": round(l_med, 4), "levels_ms_min": round(l_min, 4),
                   "levels_ms_max": round(l_max, 4), "levels_again_ms_median": round(l_med2, 4),
                   "renders_ms_median": round(r_med, 4), "renders_ms_min": round(r_min, 4),
                   "renders_ms_max": round(r_max, 4),
                   "speedup": round(r_med / l_med, 3), "levels_faster": bool(max(l_med, l_med2) < r_med),
                   "bit_identical": bool(same),
                   "workgroups_per_cu": int(lib.lsr_debug_levels_occupancy(L)),
                   "level_buffer_bytes": int(lib.lsr_levels_bytes(P, L)),
                   "visible": int(pkg["visibility_filter"].sum()),
                   "warmup": WARMUP, "calls": CALLS}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del pkg, refs
        del model, feats, params
        torch.cuda.empty_cache()
    rows.sort(key=lambda r: (args.configs.index(r["config"]), r["levels"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")
    bad = [r for r in rows if not r["bit_identical"]]
    assert not bad, bad


if __name__ == "__main__":
    main()
