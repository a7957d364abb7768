"""Generate tests/golden/lerf_eval.npz from the reference's own smooth() (eval/utils.py:46-55).

Run where a checkout of the reference is available (LANGSPLAT_REFERENCE, default /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lerf_eval_golden.py

eval/utils.py imports cv2, mediapy, matplotlib and colormaps at module level, which smooth() does not
use: where they are not importable, empty stand-in modules are registered first.  The output is a
plain .npz data file: per shape and density a seeded random uint8 mask (`mask_HxW_dD`) and smooth()'s
output for it (`smooth_HxW_dD`).
"""
import importlib
import os
import sys
import types

import numpy as np

REF = os.environ.get("LANGSPLAT_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SHAPES = [(2, 2), (2, 9), (5, 3), (8, 8), (17, 31), (33, 65)]
DENSITIES = [0.0, 0.3, 0.5, 0.7, 1.0]
SEED = 20250


def _import_smooth():
    for name in ("cv2", "mediapy", "matplotlib", "matplotlib.patches", "matplotlib.pyplot", "colormaps"):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            sys.modules[name] = mod
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], mod)
    sys.path.insert(0, os.path.join(REF, "eval"))
    from utils import smooth
    return smooth


def main():
    smooth = _import_smooth()
    rng = np.random.default_rng(SEED)
    out = {}
    for (H, W) in SHAPES:
        for d in DENSITIES:
            mask = (rng.random((H, W)) < d).astype(np.uint8)
            key = f"{H}x{W}_d{int(round(d * 10))}"
            out[f"mask_{key}"] = mask
            out[f"smooth_{key}"] = smooth(mask).astype(np.uint8)
    np.savez_compressed(os.path.join(OUT, "lerf_eval.npz"), **out)
    print(len(out), "arrays")


if __name__ == "__main__":
    main()
