"""Generate tests/golden/query.npz from the reference's own decoder and relevancy code.

Run in the build container only (the reference is not on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_query_golden.py

Imports from /root/reference:
  - autoencoder/model.py: Autoencoder (decode)
  - eval/openclip_encoder.py: OpenCLIPNetwork (get_max_across / get_relevancy).  Its module imports
    open_clip and torchvision, which only its constructor uses: where they are not importable, empty
    stand-in modules are registered first, and the network object is created with __new__ and given
    only positives, negatives, pos_embeds and neg_embeds.
The decoder weights, phrases and pixels come from tests/query_ref.py's seeded generators and are loaded
into Autoencoder with load_state_dict.  The output is a plain .npz data file: per configuration the
seed, the 64 input pixels, get_max_across's output for them (1 level, the pixels viewed as 8 x 8) and
8 decoded rows.
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import query_ref  # noqa: E402

CONFIGS = {"canonical": dict(widths=query_ref.CANONICAL, n_pos=3, n_neg=4, seed=20240),
           "small": dict(widths=[16, 32, 32], n_pos=3, n_neg=4, seed=20241)}
ENCODER_DIMS = [256, 128, 64, 32, 3]  # the reference's default encoder; only its last width matters here


def _import_reference():
    for name in ("open_clip", "torchvision"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, os.path.join(REF, "autoencoder"))
    sys.path.insert(0, os.path.join(REF, "eval"))
    from model import Autoencoder
    from openclip_encoder import OpenCLIPNetwork
    return Autoencoder, OpenCLIPNetwork


def main():
    Autoencoder, OpenCLIPNetwork = _import_reference()
    out = {}
    for name, cfg in CONFIGS.items():
        case = query_ref.make_case(cfg["widths"], 64, cfg["n_pos"], cfg["n_neg"], cfg["seed"])
        with contextlib.redirect_stdout(io.StringIO()):  # the constructor prints its module lists
            model = Autoencoder(ENCODER_DIMS, cfg["widths"])
        sd = model.state_dict()
        sd.update(query_ref.state_dict_of(case["weights"], case["biases"]))
        model.load_state_dict(sd)
        model.eval()
        net = OpenCLIPNetwork.__new__(OpenCLIPNetwork)
        net.positives = tuple(f"positive {i}" for i in range(cfg["n_pos"]))
        net.negatives = tuple(f"negative {i}" for i in range(cfg["n_neg"]))
        net.pos_embeds = torch.from_numpy(case["pos"])
        net.neg_embeds = torch.from_numpy(case["neg"])
        with torch.no_grad():
            decoded = model.decode(torch.from_numpy(case["pixels"]))           # (64, D)
            relev = net.get_max_across(decoded.view(1, 8, 8, -1))                # (1, n_pos, 8, 8)
        out[f"{name}_seed"] = np.int64(cfg["seed"])
        out[f"{name}_widths"] = np.asarray(cfg["widths"], np.int64)
        out[f"{name}_n_pos"] = np.int64(cfg["n_pos"])
        out[f"{name}_n_neg"] = np.int64(cfg["n_neg"])
        out[f"{name}_pixels"] = case["pixels"]
        out[f"{name}_relevancy"] = relev.numpy().astype(np.float32)
        out[f"{name}_decoded"] = decoded[:8].numpy().astype(np.float32)
    np.savez(os.path.join(OUT, "query.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
