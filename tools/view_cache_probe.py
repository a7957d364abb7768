"""lsr_view_save / lsr_view_restore alone (the view cache): pack bytes, bytes moved
and solo time of one restore (and one save) of a bench.py configuration's view.

    python tools/view_cache_probe.py [--config C3] [--reps 200]

One geometry-phase forward in capacity mode fills a static buffer set; the set is saved once and
restored `reps` times back to back on one stream between two events.  A restore reads the pack and
writes the same bytes into the set (plus the cleared loss words and counters).  Where the library has
lsr_view_bind, the bind that replaces the restore on a hit is timed the same way.

    python tools/view_cache_probe.py --first-epoch [--config C3] [--steps 300]

times bench.py's pipelined graph step (its model, view, target and optimizer) with every visit a
miss, as in a run's first epoch: each visit gets a key of its own, so the geometry graph, the counter
kernel and -- once its counters have arrived -- the evicted view's save run every time and nothing
is ever restored or bound.  The host runs ahead of the device, so few counters have arrived at a
set's next visit (few saves), as in bench.py's loop.  Prints the milliseconds per step and the
cache's statistics.  Works on a tree without lsr_view_bind too.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from langsplat_amd import _native  # noqa: E402
from langsplat_amd.render import GaussianRasterizationSettings  # noqa: E402
from langsplat_amd.synthetic import CONFIGS, activated_inputs, make_cameras, make_gaussians  # noqa: E402


def first_epoch(args):
    import itertools
    import time

    import bench
    from langsplat_amd.optim import Adam
    from langsplat_amd.pipeline import PipelinedGraphStep
    from langsplat_amd.render import render

    c = CONFIGS[args.config]
    P, W, H = c["P"], c["width"], c["height"]
    dev = torch.device("cuda")
    model = bench.Model(make_gaussians(P, seed=0, sh_degree=c["sh_degree"]).to(dev), include_feature=True)
    cam = make_cameras(c["views"], W, H, device=dev)[0]
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator().manual_seed(100)
    gt = torch.nn.functional.normalize(torch.randn((3, H, W), generator=gen), dim=0).to(dev)
    mask = (torch.rand((1, H, W), generator=gen) < 0.9).to(dev)
    optim = Adam([{"params": [model._language_feature], "lr": 0.0025, "name": "language_feature"}], lr=0.0, eps=1e-15)
    pg = PipelinedGraphStep(lambda: render(cam, model, bench.Pipe, bg, bench.Opt, language_target=(gt, mask))["language_l1"],
                            model.trainable(), optim, model=model, view_cache_bytes=args.budget_gb << 30)
    serial = itertools.count()
    pg._view_key = lambda r: (("visit", next(serial)), None)  # no view is ever seen twice
    pg.capture()

    def run(n):
        for _ in range(n):
            pg.replay()
    run(100)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    pg.synchronize()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / args.steps
    assert pg.check()
    st = pg.view_cache_stats()
    assert st["hits"] == 0, st
    print(f"{args.config} first epoch (host ahead): {ms:.4f} ms per step, "
          f"bound={getattr(pg, 'bound', False)}, view cache {st}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--first-epoch", action="store_true")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--budget-gb", type=int, default=40, help="--first-epoch: the packs' byte budget")
    args = ap.parse_args()
    if args.first_epoch:
        return first_epoch(args)
    c = CONFIGS[args.config]
    P, W, H = c["P"], c["width"], c["height"]
    dev = torch.device("cuda")
    params = make_gaussians(P, seed=0, sh_degree=c["sh_degree"]).to(dev)
    cam = make_cameras(c["views"], W, H, device=dev)[0]
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        inp = activated_inputs(params)
    st = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center,
                                       False, False, True)
    call = (st, inp["means3D"], inp["shs"], None, inp["language_feature_precomp"], inp["opacities"], inp["scales"],
            inp["rotations"], None)
    _native.rasterize_gaussians(*call)
    torch.cuda.synchronize()
    rendered, entries = _native.LAST_COUNTS[(P, W, H)]
    bufs = _native.static_buffers()
    overflow = torch.zeros((), dtype=torch.int32, device=dev)
    with _native.capacity(int(rendered * 1.125) + 1024, int(entries * 1.125) + 1024, overflow), bufs, \
            _native.forward_phase(_native.forward_phase.GEOMETRY):
        _native.rasterize_gaussians(*call)
    nbytes = _native.view_pack_bytes(P, W, H, rendered)
    pack = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    a = _native.view_args(bufs, rendered, pack)
    s = torch.cuda.current_stream()
    _native.view_save(a, s)
    _native.view_restore(a, s)
    torch.cuda.synchronize()
    assert int(overflow.item()) == 0
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    free, total = torch.cuda.mem_get_info(dev)
    print(f"{args.config}: P={P} {W}x{H} num_rendered={rendered} pack={nbytes} B ({nbytes / 1e6:.1f} MB); "
          f"half of the free memory ({free / 2e9:.0f} GB) holds {free // 2 // nbytes} such views")
    forms = [("restore", _native.view_restore, 2 * nbytes + 8 * tiles + 4 * 144), ("save", _native.view_save, 2 * nbytes)]
    if getattr(_native, "has_view_bind", lambda: False)():
        # recb read, the plane's touched lines, radii read + written, ranges and the class lists read + written
        forms.append(("bind", _native.view_bind, 4 * P + 16 * P + 8 * P + 2 * 12 * tiles + 8 * tiles + 4 * 144))
    for name, fn, moved in forms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(args.reps):
            fn(a, s)
        e1.record(s)
        torch.cuda.synchronize()
        us = 1000.0 * e0.elapsed_time(e1) / args.reps
        print(f"{name}: {us:.1f} us per launch back to back, {moved / 1e6:.1f} MB moved (read + write), "
              f"{moved / us / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()
