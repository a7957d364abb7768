"""lsr_view_save / lsr_view_restore alone (the view cache): pack bytes, bytes moved
and solo time of one restore (and one save) of a bench.py configuration's view.

    python tools/view_cache_probe.py [--config C3] [--reps 200]

One geometry-phase forward in capacity mode fills a static buffer set; the set is saved once and
restored `reps` times back to back on one stream between two events.  A restore reads the pack and
writes the same bytes into the set (plus the cleared loss words and counters).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
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
    for name, fn, extra in (("restore", _native.view_restore, 8 * tiles + 4 * 144), ("save", _native.view_save, 0)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(args.reps):
            fn(a, s)
        e1.record(s)
        torch.cuda.synchronize()
        us = 1000.0 * e0.elapsed_time(e1) / args.reps
        moved = 2 * nbytes + extra
        print(f"{name}: {us:.1f} us per launch back to back, {moved / 1e6:.1f} MB moved (read + write), "
              f"{moved / us / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()
